"""Child process of tests/test_hip_metrics_trainer.py: the native metrics against the torch metrics on the same round, and a recorded native
round against an eager one, with the convolution library in DETERMINISTIC mode.  Results go as JSON to ``sys.argv[1]``; with a second
argument, the distances of the float32 torch metrics from the float64 restatement are also written there as text (how
profiles/r18/test_figures.txt was made: a measurement, not a threshold).

Part 1.  Trainers A (metrics="torch", diagnostics on), B (metrics="native", diagnostics on) and C (metrics="native", diagnostics off) run one
round on the default float32 update path from the same seeds.  A's per-minibatch records are collected on the way (the arrays
``ippmarl.metrics`` was given, the actions of each minibatch, the probabilities the actor's forward returned, the gradients at the time of
the call) and the float64 restatement (tests/metrics_native_ref.py) is evaluated on them.

Part 2.  Two trainers with metrics="native", graphs=True from identical training state: one runs two rounds launch by launch, the other
replays them from ``capture_graphs()``; both with diagnostics on.

Why a process of its own: as tests/adam_recorded_rounds.py -- the library's deterministic mode depends on environment variables that the
library reads once per process, so they are set here before anything is imported."""
import hashlib
import json
import os
import sys

for _v in ("FWD", "BWD", "WRW"):
    os.environ[f"MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_{_v}"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("tests", "oracle", "ipp-marl_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.backends.cudnn.deterministic = True


def digest(net):
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    return hashlib.sha256(flat.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _np(t):
    return t.detach().cpu().numpy()


def watch(tr):
    """Collects what trainer ``tr`` (metrics="torch") hands to ippmarl.metrics during its diagnostics round -> the dict that fills."""
    from ippmarl import metrics, optim_native
    seen = dict(actions=[], probs=[])
    real_backward = tr.critic_learner.backward

    def backward(states, actions, td):
        if tr.critic_learner.collect:
            seen["actions"].append(_np(actions).copy())
        return real_backward(states, actions, td)

    tr.critic_learner.backward = backward
    tr.actor.register_forward_hook(lambda mod, args, out: seen["probs"].append(_np(out[0]).copy())
                                   if tr.actor_learner.collect and torch.is_grad_enabled() else None)
    real_critic, real_actor = metrics.critic_metrics, metrics.actor_metrics

    def critic_metrics(steps, critic):
        seen["critic_steps"] = [{k: _np(v).copy() for k, v in s.items()} for s in steps]
        seen["critic_grads"] = [_np(p.grad).copy() for p in optim_native.used_parameters(critic)]
        return real_critic(steps, critic)

    def actor_metrics(steps, actor, after):
        seen["actor_steps"] = [{k: _np(v).copy() for k, v in s.items()} for s in steps]
        seen["after"] = [_np(x).copy() for x in after]
        seen["actor_grads"] = [_np(p.grad).copy() for p in optim_native.used_parameters(actor)]
        return real_actor(steps, actor, after)

    metrics.critic_metrics, metrics.actor_metrics = critic_metrics, actor_metrics
    return seen, lambda: (setattr(metrics, "critic_metrics", real_critic), setattr(metrics, "actor_metrics", real_actor))


def part_one():
    import metrics_native_ref as R
    from ippmarl import metrics_native
    from test_hip_adam_trainer import _trainer
    a, b, c = (_trainer(seed=11, n_envs=2, metrics=m) for m in ("torch", "native", "native"))
    seen, restore = watch(a)
    for tr, diag in ((a, True), (b, True), (c, False)):
        torch.manual_seed(12)
        assert tr.rollout("train")["faults"] == 0
        stats = tr.update(diagnostics=diag)
        assert np.isfinite(stats["critic_loss"]) and np.isfinite(stats["actor_loss"])
    restore()
    torch.cuda.synchronize()
    nb = a.batch_number
    assert len(seen["actions"]) == len(seen["probs"]) == len(seen["critic_steps"]) == len(seen["actor_steps"]) == nb
    cs, as_ = seen["critic_steps"], seen["actor_steps"]
    crit = dict(loss=[s["loss"] for s in cs], q_chosen=[s["q_chosen"] for s in cs], td=[s["td"] for s in cs],
                disc=[s["discounted"] for s in cs], q_new=[s["q_new"] for s in cs], action=seen["actions"])
    act = dict(loss=[s["loss"] for s in as_], adv=[s["adv"] for s in as_], probs=seen["probs"], action=seen["actions"],
               hidden0=[s["hidden0"] for s in as_], probs_after=seen["after"])
    ref = R.all_scalars(crit, act, seen["critic_grads"], seen["actor_grads"])
    scale = R.scales(crit, act, seen["critic_grads"], seen["actor_grads"])
    keys = list(metrics_native.KEYS)
    assert list(a.last_diagnostics) == keys == list(b.last_diagnostics) and c.last_diagnostics is None
    return dict(keys=keys, ref=ref.tolist(), bound=R.bound(ref, scale).tolist(), torch=[a.last_diagnostics[k] for k in keys],
                native=[b.last_diagnostics[k] for k in keys], shape=[nb, int(seen["actions"][0].shape[0]), a.A],
                digests={net: [digest(getattr(tr, net)) for tr in (a, b, c)] for net in ("critic", "actor")})


def part_two():
    from test_hip_adam_trainer import _copy_training_state, _trainer
    eager, rec = (_trainer(seed=11, n_envs=2, graphs=True, metrics="native") for _ in range(2))
    for tr in (eager, rec):           # first round launch by launch (kernel selection, allocator)
        torch.manual_seed(12)
        tr.rollout("train")
        tr.update(diagnostics=True)
    _copy_training_state(eager, rec)
    rec.capture_graphs()
    rounds = []
    for r in range(2):
        row = {}
        for name, tr in (("eager", eager), ("recorded", rec)):
            torch.manual_seed(20 + r)
            assert tr.rollout("train")["faults"] == 0
            tr.last_diagnostics = None
            tr.update(diagnostics=True)
            torch.cuda.synchronize()
            row[name] = dict(scalars=[float(v).hex() for v in tr.last_diagnostics.values()], keys=list(tr.last_diagnostics),
                             finite=bool(np.isfinite(list(tr.last_diagnostics.values())).all()),
                             critic=digest(tr.critic), actor=digest(tr.actor))
        rounds.append(row)
    assert rec._update_graph is not None and eager._update_graph is None
    # a recorded round without diagnostics replays the same graph and reads nothing
    torch.manual_seed(30)
    rec.rollout("train")
    rec.last_diagnostics = None
    rec.update()
    return dict(rounds=rounds, silent=rec.last_diagnostics is None)


def main():
    for v in ("IPPMARL_ADAM", "IPPMARL_HEAD_UPDATE", "IPPMARL_TRUNK_UPDATE", "IPPMARL_CONV2_UPDATE", "IPPMARL_ACTOR_INFERENCE",
              "IPPMARL_CRITIC_INFERENCE", "IPPMARL_BUFFER", "IPPMARL_METRICS"):
        os.environ.pop(v, None)
    one = part_one()
    two = part_two()
    with open(sys.argv[1], "w") as f:
        json.dump({"one": one, "two": two}, f)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            nb, B, A = one["shape"]
            f.write(f"# one diagnostics round, {nb} minibatches of {B} rows, {A} actions, float32 update path, deterministic convolutions\n")
            f.write("# |value - float64 restatement on the round's float32 records|: metrics=\"torch\" (float32 reductions), "
                    "metrics=\"native\", the derived bound\n")
            for k, r, t, n, bd in zip(one["keys"], one["ref"], one["torch"], one["native"], one["bound"]):
                f.write(f"{k:48s} ref {r: .17e}  torch {abs(t - r):.3e}  native {abs(n - r):.3e}  bound {bd:.3e}\n")


if __name__ == "__main__":
    main()
