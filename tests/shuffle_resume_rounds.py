"""Child process of tests/test_hip_shuffle_trainer.py: whole training rounds that have to agree bit for bit, with the convolution library in
DETERMINISTIC mode.  Results go as JSON to ``sys.argv[1]``; ``sys.argv[2]`` is a scratch directory.

premise   Two eager default trainers from the same seeds agree after a round (without this nothing below means anything).
repro     shuffle="torch" and shuffle="native": two trainers from the same initial weights, DIFFERENT torch seeds set after construction, two
          rounds each.  Native must agree in both nets; torch is recorded for the record (it is why the switch exists).
replay    graphs=True, shuffle="native": one trainer runs two rounds launch by launch, its twin replays them; no manual_seed anywhere.
resume    A runs 4 rounds; B runs 2 and saves; a fresh C (other weights, other torch seed) loads and runs 2: A against C, for adam x shuffle,
          and with C's graphs captured before the load (either Adam: the blob's views, the capturable torch form's state tensors).
mission   A COMAMission stopped after 2 of 3 updates and resumed, beside an uninterrupted one.

Why a process of its own: as tests/rollout_log_recorded_rounds.py -- the library's deterministic mode depends on environment variables that
the library reads once per process, so they are set here before anything is imported."""
import hashlib
import json
import os
import sys

for _v in ("FWD", "BWD", "WRW"):
    os.environ[f"MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_{_v}"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("tests", "oracle", "ipp-marl_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import torch  # noqa: E402

torch.backends.cudnn.deterministic = True

SWITCHES = ("IPPMARL_ADAM", "IPPMARL_HEAD_UPDATE", "IPPMARL_TRUNK_UPDATE", "IPPMARL_CONV2_UPDATE", "IPPMARL_ACTOR_INFERENCE",
            "IPPMARL_CRITIC_INFERENCE", "IPPMARL_BUFFER", "IPPMARL_METRICS", "IPPMARL_ROLLOUT_LOG", "IPPMARL_SHUFFLE")
MODULES = ("actor", "critic", "target_critic", "frozen_target")


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def digest(net):
    return _sha(torch.cat([p.detach().reshape(-1) for p in net.parameters()]))


def modules_of(tr):
    return {"actor": tr.actor, "critic": tr.critic, "target_critic": tr.critic_learner.target_critic, "frozen_target": tr.frozen_target}


def optimizer_digest(opt):
    """The optimizer's state_dict(), entry by entry: {"<param>/<key>": sha}."""
    out = {}
    for i, entry in sorted(opt.state_dict()["state"].items()):
        for k, v in sorted(entry.items()):
            out[f"{i}/{k}"] = _sha(torch.as_tensor(v).double()) if k == "step" else _sha(v)
    return out


def snapshot(tr):
    torch.cuda.synchronize()
    return {"modules": {k: digest(m) for k, m in modules_of(tr).items()},
            "optimizers": {"actor": optimizer_digest(tr.actor_learner.optimizer), "critic": optimizer_digest(tr.critic_learner.optimizer)},
            "wave": tr.wave, "train_step": tr.train_step, "eps": float(tr.eps).hex(), "eps_dev": float(tr.eps_dev).hex(),
            "returns": [_sha(tr.ret), _sha(tr.abs_ret), _sha(tr.team_ret)], "filled": tr.filled}


def run_rounds(tr, n):
    for _ in range(n):
        assert tr.rollout("train")["faults"] == 0
        tr.update()


def _trainer(seed, **kw):
    from test_hip_adam_trainer import _trainer as make
    return make(seed=seed, n_envs=2, **kw)


def premise():
    a, b = (_trainer(11) for _ in range(2))
    for tr in (a, b):
        torch.manual_seed(12)
        run_rounds(tr, 1)
    return [snapshot(a), snapshot(b)]


def repro():
    out = {}
    for mode in ("torch", "native"):
        a, b = (_trainer(11, shuffle=mode) for _ in range(2))
        for seed, tr in ((101, a), (202, b)):
            torch.manual_seed(seed)               # after construction: the weights are the same, the device generator is not
            run_rounds(tr, 2)
        out[mode] = [snapshot(a), snapshot(b)]
    return out


def replay():
    eager, rec = (_trainer(11, graphs=True, shuffle="native") for _ in range(2))
    for tr in (eager, rec):                       # first round launch by launch (kernel selection, allocator)
        run_rounds(tr, 1)
    first = [snapshot(eager), snapshot(rec)]
    rec.capture_graphs()
    rounds = []
    for _ in range(2):
        run_rounds(eager, 1)
        run_rounds(rec, 1)
        rounds.append([snapshot(eager), snapshot(rec)])
    return dict(first=first, rounds=rounds, T=eager.T, replays=[eager.step_replays, rec.step_replays],
                counter=[rec._shuffle.round(), rec.train_step])


def resume(tmp, adam, shuffle, graphs):
    from test_hip_adam_trainer import _params64
    params = lambda: _params64(networks__data_passes=2, networks__copy_rate=3)  # noqa: E731  (a hard target copy on either side of the save)
    kw = dict(adam=adam, shuffle=shuffle, graphs=graphs)
    path = os.path.join(tmp, f"state_{adam}_{shuffle}_{int(graphs)}.pt")
    a = _trainer(11, params=params(), **kw)
    torch.manual_seed(31)
    run_rounds(a, 4)
    b = _trainer(11, params=params(), **kw)
    torch.manual_seed(31)
    run_rounds(b, 2)
    b.save_state(path)
    saved = snapshot(b)
    torch.load(path, weights_only=True)           # a plain file of tensors, numbers and strings
    c = _trainer(77, params=params(), **kw)       # other initial weights, another frozen target
    torch.manual_seed(999)
    if graphs:
        run_rounds(c, 1)
        c.capture_graphs()
    fresh = snapshot(c)
    c.load_state(path)
    loaded = snapshot(c)
    run_rounds(c, 2)
    return dict(a=snapshot(a), c=snapshot(c), saved=saved, loaded=loaded, fresh=fresh, replays=c.step_replays, T=c.T)


class Recorder:
    """A writer that keeps every scalar it is given."""

    def __init__(self):
        self.records = []

    def add_scalar(self, tag, value, step):
        self.records.append((tag, float(value).hex(), int(step)))


def mission(tmp):
    from ippmarl.missions.coma_mission import COMAMission
    from test_hip_adam_trainer import _params64

    def make(name, n_episodes, seed, **kw):
        torch.manual_seed(seed)
        params = _params64(experiment__missions__n_episodes=n_episodes, experiment__missions__patience=1, networks__data_passes=2)
        return COMAMission(params, Recorder(), n_envs=2, log_dir=os.path.join(tmp, name), eval_every=2, eval_episodes=2, first_episode=3,
                           shuffle="native", **kw)

    whole = make("whole", 3, 41)
    whole.execute()
    stopped = make("stopped", 2, 41, state_every=2)
    stopped.execute()
    state = os.path.join(tmp, "stopped", "trainer_state.pt")
    leftovers = [f for f in os.listdir(os.path.join(tmp, "stopped")) if f.endswith(".tmp")]
    resumed = make("resumed", 3, 88, resume=state)             # (other initial weights: everything that matters comes from the file)
    at_resume = [resumed.training_step_idx, resumed.environment_step_idx, len(resumed.episode_returns)]
    resumed.execute()
    return dict(whole=whole.writer.records, stopped=stopped.writer.records, resumed=resumed.writer.records,
                best=[float(whole.max_mean_episode_return).hex(), float(resumed.max_mean_episode_return).hex()],
                returns=[[float(r).hex() for r in m.episode_returns] for m in (whole, resumed)],
                steps=[[m.training_step_idx, m.environment_step_idx] for m in (whole, resumed)], at_resume=at_resume,
                state_exists=os.path.isfile(state), leftovers=leftovers,
                best_model=[os.path.isfile(os.path.join(tmp, n, "best_model.pth")) for n in ("whole", "stopped", "resumed")])


def main():
    for v in SWITCHES:
        os.environ.pop(v, None)
    tmp = sys.argv[2]
    result = {"premise": premise(), "repro": repro(), "replay": replay(), "mission": mission(tmp), "resume": {}}
    for adam in ("torch", "native"):
        for shuffle in ("torch", "native"):
            result["resume"][f"{adam}/{shuffle}"] = resume(tmp, adam, shuffle, False)
    result["resume"]["graphs"] = resume(tmp, "native", "native", True)
    result["resume"]["graphs/torch"] = resume(tmp, "torch", "native", True)      # (copy_ into the capturable torch Adam's state tensors)
    with open(sys.argv[1], "w") as f:
        json.dump(result, f)


if __name__ == "__main__":
    main()
