#!/usr/bin/env python
"""Digests of whole ``COMATrainer`` rounds, for comparing two versions of the HOST code that sequences a round (ippmarl/trainer.py and
what it is built from) bit for bit and launch for launch over the same libippmarl.so: the existing tests bound errors and compare one
switch at a time, so a reordered or doubled launch in some combination of switches would pass them; two package trees whose digests
agree computed the same bits from the same number of device launches.

One process, deterministic convolutions (the library reads its variables once, so they are set before anything is imported), the ten
IPPMARL_* switch variables removed from the environment.  The smallest shapes at which every branch of the round is taken: 2 UAVs on the
64 x 64 grid, 2 envs, two rounds from fixed torch seeds (DeepQ's 4 UAVs and the two-wave round run 1 env, which keeps their minibatches at
the rows of the others: at twice the rows the float32 update is not reproducible run to run on the MI355X, whatever sequences it).

One JSON line per configuration (``configurations()`` below) with the SHA-256 (its first 64 bits) of each of the four nets' parameters
and of each optimizer's state, of the returns and the five buffers after the last rollout, every ``update()`` result and the values of
``last_diagnostics`` with floats as hex, the rollout log where one is kept, the counters, and the device launches (torch.profiler) of one
``_rollout_step`` and one ``_update_compute`` -- after a capture, the runtime's launch calls of one replayed round instead.

``--package-root`` is the directory that holds the ``ippmarl`` package to run (default: this tree's); the library is the one IPPMARL_LIB
names (default: this tree's lib/libippmarl.so), so a checkout of another commit's ``ipp-marl_amd/ippmarl`` runs over the same library:

    python tools/trainer_round_digests.py --package-root /path/to/parent/ipp-marl_amd > parent.jsonl
    python tools/trainer_round_digests.py > new.jsonl && cmp parent.jsonl new.jsonl"""
import argparse
import hashlib
import json
import os
import sys
import tempfile

for _v in ("FWD", "BWD", "WRW"):
    os.environ[f"MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_{_v}"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH_ENV = ("IPPMARL_ADAM", "IPPMARL_HEAD_UPDATE", "IPPMARL_TRUNK_UPDATE", "IPPMARL_CONV2_UPDATE", "IPPMARL_ACTOR_INFERENCE",
              "IPPMARL_CRITIC_INFERENCE", "IPPMARL_BUFFER", "IPPMARL_METRICS", "IPPMARL_ROLLOUT_LOG", "IPPMARL_SHUFFLE")
for _v in SWITCH_ENV:
    os.environ.pop(_v, None)
_ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
_ap.add_argument("--package-root", default=os.path.join(ROOT, "ipp-marl_amd"))
_ap.add_argument("--only", default="", help="comma-separated configuration names (default: all)")
ARGS = _ap.parse_args()
os.environ.setdefault("IPPMARL_LIB", os.path.join(ROOT, "ipp-marl_amd", "lib", "libippmarl.so"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.abspath(ARGS.package_root))

import torch  # noqa: E402

torch.backends.cudnn.deterministic = True

from configs import make_params  # noqa: E402

# every switch at its non-default value
ON = dict(rollout_log="native", metrics="native", buffer="native", actor_inference="native", critic_inference="native", adam="native",
          head_update="bf16", conv2_update="bf16", trunk_update="bf16", shuffle="native")


def params64(**kw):
    """2 UAVs on a 64 x 64 grid (``_params64`` of tests/test_hip_adam_trainer.py)."""
    return make_params("small", experiment__missions__n_agents=2, sensor__field_of_view__angle_x=99.0, sensor__field_of_view__angle_y=99.0, **kw)


def sha(*tensors):
    """The first 64 bits of the SHA-256 of the tensors' bytes, one after the other (short lines: the files are kept for comparison)."""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:16]


def plain(x):
    """``x`` as JSON: floats as hex, tensors as digests, dict keys as strings."""
    if isinstance(x, torch.Tensor):
        return sha(x)
    if isinstance(x, float):
        return x.hex()
    if isinstance(x, dict):
        return {str(k): plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x


def optimizer_digest(opt):
    """One digest of the optimizer's state_dict(): every entry's tensors in (parameter, key) order, step counters as float64."""
    return sha(*[torch.as_tensor(v).double() if k == "step" else v
                 for _, entry in sorted(opt.state_dict()["state"].items()) for k, v in sorted(entry.items())])


def snapshot(tr, buffers=True):
    torch.cuda.synchronize()
    nets = {"actor": tr.actor, "critic": tr.critic, "target_critic": tr.critic_learner.target_critic, "frozen_target": tr.frozen_target}
    return {"modules": {k: sha(torch.cat([p.detach().reshape(-1) for p in m.parameters()])) for k, m in nets.items()},
            "optimizers": {"actor": optimizer_digest(tr.actor_learner.optimizer), "critic": optimizer_digest(tr.critic_learner.optimizer)},
            "returns": {k: sha(getattr(tr, k)) for k in ("ret", "abs_ret", "team_ret")},
            "buffers": {k: sha(getattr(tr, k)) for k in ("buf_obs", "buf_state", "buf_action", "buf_mask", "buf_reward")} if buffers else None,
            "train_step": tr.train_step, "wave": tr.wave, "step_replays": tr.step_replays}


def one_round(tr, diagnostics):
    """The round's waves and its update -> what they returned, logged and left in ``last_diagnostics``."""
    out = {"rollouts": []}
    for _ in range(tr.waves_per_update):
        stats = tr.rollout("train")
        assert stats["faults"] == 0, stats
        out["rollouts"].append(plain(stats))
    if tr.keep_rollout_log:
        out["log"] = plain(tr.read_rollout_log("train", tr.waves_per_update) if tr.rollout_log == "native" else tr.last_rollout)
    tr.last_diagnostics = None
    out["update"] = plain(tr.update(diagnostics=diagnostics))
    # (the 32 scalars in the order of their sorted tags)
    out["diagnostics"] = None if tr.last_diagnostics is None else [plain(float(v)) for _, v in sorted(tr.last_diagnostics.items())]
    return out


LAUNCH_CALLS = ("hipLaunchKernel", "hipExtLaunchKernel", "hipModuleLaunchKernel", "hipExtModuleLaunchKernel", "hipLaunchCooperativeKernel")


def _profiled(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return prof.events()


def device_launches(fn):
    return sum(1 for e in _profiled(fn) if e.device_type == torch.autograd.DeviceType.CUDA)


def host_launches(fn):
    """The runtime calls of a replayed round: graph launches, and kernel launches outside the graphs.  (The profiler's DEVICE events of
    a replayed graph are not a count: it reports a varying part of a graph's kernels.)"""
    names = [e.name for e in _profiled(fn) if e.device_type != torch.autograd.DeviceType.CUDA]
    return {"graph_launches": names.count("hipGraphLaunch"), "kernel_launch_calls": sum(names.count(n) for n in LAUNCH_CALLS)}


def eager_launches(tr, diagnostics):
    """Device launches of one ``_rollout_step`` and of one ``_update_compute`` (the trainer is not used afterwards)."""
    from ippmarl.parallel import episode_ids
    from ippmarl.vec_env import POLICY_SAMPLE
    eps = tr.eps_dev if tr.graphs else tr.eps
    for _ in range(tr.waves_per_update):
        tr.rollout("train")
    tr.env.reset(episode_ids(tr.first_episode, tr.wave, tr.E, tr.rank, tr.world))
    if tr.keep_rollout_log and tr.rollout_log == "native":
        tr._log_wave = 0                    # (the step writes the native log, as inside rollout())
    step = device_launches(lambda: tr._rollout_step(0, 0, POLICY_SAMPLE, True, eps))
    tr._log_wave = None
    torch.manual_seed(5)
    update = device_launches(lambda: tr._update_compute(None, eps, diagnostics))
    return {"rollout_step": step, "update_compute": update}


def trainer(seed, kw, params=None, n_envs=2, keep_log=False):
    from ippmarl.trainer import COMATrainer
    torch.manual_seed(seed)
    tr = COMATrainer(params or params64(), n_envs=n_envs, first_episode=3, **kw)
    tr.keep_rollout_log = keep_log
    return tr


def plain_rounds(kw, params=None, diagnostics=False, keep_log=False, n_envs=2):
    """Two rounds launch by launch."""
    tr = trainer(11, kw, params, n_envs=n_envs, keep_log=keep_log)
    rounds = []
    for seed in (21, 22):
        torch.manual_seed(seed)
        rounds.append(one_round(tr, diagnostics))
    return {"rounds": rounds, "state": snapshot(tr), "launches": eager_launches(tr, diagnostics)}


def recorded_rounds(kw, diagnostics):
    """graphs=True: one round launch by launch, capture_graphs(), two replayed rounds."""
    tr = trainer(11, dict(kw, graphs=True))
    torch.manual_seed(21)
    eager = {"rounds": [one_round(tr, diagnostics)], "state": snapshot(tr)}
    tr.capture_graphs()
    rounds = []
    for seed in (22, 23):
        torch.manual_seed(seed)
        rounds.append(one_round(tr, diagnostics))
    assert tr.step_replays == 2 * tr.T, tr.step_replays
    recorded = {"rounds": rounds, "state": snapshot(tr)}
    torch.manual_seed(24)
    return {"eager": eager, "recorded": recorded, "launches": {"replayed_round": host_launches(lambda: one_round(tr, diagnostics))}}


def resumed_rounds(kw):
    """One round, save_state, a fresh trainer from other weights loads it and runs one more."""
    a = trainer(11, kw)
    torch.manual_seed(21)
    first = one_round(a, False)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "state.pt")
        a.save_state(path)
        b = trainer(77, kw)
        torch.manual_seed(999)
        b.load_state(path)
    loaded = snapshot(b, buffers=False)        # (no rollout has written this trainer's buffers yet)
    second = one_round(b, False)
    return {"rounds": [first, second], "loaded": loaded, "state": snapshot(b)}


def configurations():
    soft = dict(networks__critic__target_update_mode="soft")
    deepq = lambda: make_params("small", experiment__missions__type="DeepQ")  # noqa: E731  (as tests/test_hip_deepq.py builds it)
    yield "defaults", lambda: plain_rounds({})
    for name, value in ON.items():
        yield f"{name}={value}", lambda name=name, value=value: plain_rounds({name: value})
    yield "all_on", lambda: plain_rounds(ON)
    for metrics in ("torch", "native"):
        for buffer in ("torch", "native"):
            yield f"diagnostics/metrics={metrics}/buffer={buffer}", \
                lambda m=metrics, b=buffer: plain_rounds(dict(metrics=m, buffer=b), diagnostics=True)
    yield "diagnostics/all_on", lambda: plain_rounds(ON, diagnostics=True)
    for base_name, base in (("defaults", {}), ("all_on", ON)):
        yield f"graphs/{base_name}", lambda base=base: recorded_rounds(base, False)
        yield f"graphs/{base_name}/diagnostics", lambda base=base: recorded_rounds(dict(base, metrics="native"), True)
    for log in ("torch", "native"):
        yield f"keep_rollout_log/rollout_log={log}", lambda log=log: plain_rounds(dict(rollout_log=log), keep_log=True)
    for buffer in ("torch", "native"):
        for keep in (False, True):
            yield f"deepq/buffer={buffer}" + ("/keep_rollout_log" if keep else ""), \
                lambda b=buffer, k=keep: plain_rounds(dict(buffer=b), params=deepq(), keep_log=k, n_envs=1)
    for shuffle in ("torch", "native"):
        yield f"team_sizes/shuffle={shuffle}", lambda s=shuffle: plain_rounds(dict(team_sizes=[1, 2], shuffle=s))
    yield "waves_per_update=2", lambda: plain_rounds(dict(waves_per_update=2), n_envs=1)
    yield "quirks=fixed/soft", lambda: plain_rounds(dict(quirks="fixed"), params=params64(**soft))
    for shuffle in ("torch", "native"):
        yield f"resume/shuffle={shuffle}", lambda s=shuffle: resumed_rounds(dict(shuffle=s))


def main():
    import ippmarl
    print(f"ippmarl from {os.path.dirname(ippmarl.__file__)}, library {os.environ['IPPMARL_LIB']}", file=sys.stderr)
    if not torch.cuda.is_available():
        raise SystemExit("trainer_round_digests.py runs whole rounds on the GPU; there is nothing to digest without one")
    only = [n for n in ARGS.only.split(",") if n]
    for name, run in configurations():
        if only and name not in only:
            continue
        print(json.dumps({"config": name, **run()}, sort_keys=True, separators=(",", ":")), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
