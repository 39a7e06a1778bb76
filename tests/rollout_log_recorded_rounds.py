"""Child process of tests/test_hip_rollout_log_trainer.py: the native rollout log above the kernels where whole rounds have to agree bit for
bit, with the convolution library in DETERMINISTIC mode.  Results go as JSON to ``sys.argv[1]``.

Part 1 (the log changes nothing).  Trainers from the same seeds with rollout_log="torch" and "native", both keeping the log, run one wave and
one round: the five buffers after the wave and both nets' parameters after the round are digested; the native log is also compared with the
restatement on the torch trainer's ``last_rollout``.

Part 2 (recorded).  Two trainers with graphs=True, rollout_log="native", keep_rollout_log=True from identical training state: one runs two
rounds launch by launch, the other replays its step graphs after ``capture_graphs()`` (counted by ``step_replays``); the log of every wave
is read as bits.

Part 3 (mission).  A COMAMission with rollout_log="torch" and one with "native" (graphs=True, its trainer captured after the first round, so
the later train waves replay), both with a writer that records every scalar, and ``last_counts`` kept after every log.

Why a process of its own: as tests/metrics_recorded_rounds.py -- the library's deterministic mode depends on environment variables that the
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

SWITCHES = ("IPPMARL_ADAM", "IPPMARL_HEAD_UPDATE", "IPPMARL_TRUNK_UPDATE", "IPPMARL_CONV2_UPDATE", "IPPMARL_ACTOR_INFERENCE",
            "IPPMARL_CRITIC_INFERENCE", "IPPMARL_BUFFER", "IPPMARL_METRICS", "IPPMARL_ROLLOUT_LOG")


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def digest(net):
    return _sha(torch.cat([p.detach().reshape(-1) for p in net.parameters()]))


def _hex(values):
    return [float(v).hex() for v in values]


def stats_of(rollouts):
    """The float64 definitions on a torch-logged wave list: (ref [12], scale [12])."""
    cat = lambda key: np.concatenate([r[key].cpu().numpy().astype(np.float64).ravel() for r in rollouts])  # noqa: E731
    ref, scale = [], []
    for x in (cat("absolute_returns"), cat("rewards"), cat("episode_returns")):
        ref += [np.mean(x), np.std(x), np.max(x), np.min(x)]
        scale += [float(np.abs(x).mean())] * 4
    return np.array(ref), np.array(scale)


def part_one():
    import rollout_log_ref as R
    from test_hip_adam_trainer import _trainer
    a, b = (_trainer(seed=11, n_envs=2, rollout_log=m) for m in ("torch", "native"))
    buffers, params = [], []
    for tr in (a, b):
        tr.keep_rollout_log = True
        torch.manual_seed(12)
        assert tr.rollout("train")["faults"] == 0
        buffers.append([_sha(getattr(tr, k)) for k in ("buf_obs", "buf_state", "buf_action", "buf_mask", "buf_reward")])
    scalars, actions, altitudes, bad = b.read_rollout_log("train", 1)
    for tr in (a, b):
        torch.manual_seed(13)          # (the minibatch permutations)
        tr.update()
        params.append([digest(tr.critic), digest(tr.actor)])
    ref, scale = stats_of([a.last_rollout])
    d = a.env.d
    act, alt = a.last_rollout["actions"].cpu().numpy(), a.last_rollout["altitudes"].cpu().numpy()        # [E,T,N]
    cnt = R.counts(act[None], alt[None], a.A, d.min_altitude, d.spacing, d.space_z)
    return dict(buffers=buffers, params=params, torch_has_rollout=a.last_rollout is not None, native_has_rollout=b.last_rollout is not None,
                native=list(scalars.values()), ref=ref.tolist(), bound=R.bound(ref, scale).tolist(),
                counts=[actions, {str(k): v for k, v in altitudes.items()}, bad],
                ref_counts=[R.last_counts(cnt, a.A, d.min_altitude, d.spacing, d.space_z)["actions"],
                            {str(k): v for k, v in R.last_counts(cnt, a.A, d.min_altitude, d.spacing, d.space_z)["altitudes"].items()},
                            int(cnt[64])])


def part_two():
    from test_hip_adam_trainer import _copy_training_state, _trainer
    eager, rec = (_trainer(seed=11, n_envs=2, graphs=True, rollout_log="native") for _ in range(2))
    for tr in (eager, rec):           # first round launch by launch (kernel selection, allocator)
        tr.keep_rollout_log = True
        torch.manual_seed(12)
        tr.rollout("train")
        tr.update()
    _copy_training_state(eager, rec)
    rec.capture_graphs()
    rounds = []
    for r in range(2):
        row = {}
        for name, tr in (("eager", eager), ("recorded", rec)):
            torch.manual_seed(20 + r)
            stats = tr.rollout("train")
            assert stats["faults"] == 0
            scalars, actions, altitudes, bad = tr.read_rollout_log("train", 1)
            ret_max, ret_min, abs_max, abs_min = (float(x) for x in (tr.ret.max(), tr.ret.min(), tr.abs_ret.max(), tr.abs_ret.min()))
            tr.update()
            torch.cuda.synchronize()
            row[name] = dict(scalars=_hex(scalars.values()), keys=list(scalars), counts=[actions, sorted(altitudes.items()), bad],
                             finite=bool(np.isfinite(list(scalars.values())).all()), returns=_hex([abs_max, abs_min, ret_max, ret_min]),
                             critic=digest(tr.critic), actor=digest(tr.actor), last_rollout=tr.last_rollout is not None)
        rounds.append(row)
    return dict(rounds=rounds, T=eager.T, replays=[eager.step_replays, rec.step_replays], rows=eager.T * eager.E * eager.N)


class Recorder:
    """A writer that keeps every scalar it is given."""

    def __init__(self):
        self.records = []

    def add_scalar(self, tag, value, step):
        self.records.append((tag, float(value), int(step)))


def part_three(log_dir):
    import rollout_log_ref as R
    from ippmarl.missions.coma_mission import COMAMission
    from test_hip_adam_trainer import _params64
    missions, seen = {}, {}
    for mode in ("torch", "native"):
        torch.manual_seed(31)
        params = _params64(experiment__missions__n_episodes=1, experiment__missions__patience=1)
        m = COMAMission(params, Recorder(), n_envs=2, log_dir=os.path.join(log_dir, mode), eval_every=1, eval_episodes=4, first_episode=3,
                        graphs=True, rollout_log=mode)
        log = seen[mode] = dict(counts=[], refs=[])
        real = m.add_to_tensorboard

        def add(rollouts, diagnostics=None, m=m, log=log, real=real, mode=mode):
            if mode == "torch":
                ref, scale = stats_of(rollouts)
                log["refs"].append([ref.tolist(), R.bound(ref, scale).tolist()])
            out = real(rollouts, diagnostics)
            log["counts"].append([m.last_counts["actions"], sorted(m.last_counts["altitudes"].items())])
            return out

        m.add_to_tensorboard = add
        missions[mode] = m
    for mode, m in missions.items():       # the first round launch by launch (with its evaluation), then two more: native replays them
        torch.manual_seed(32)
        m.execute()
    missions["native"].trainer.capture_graphs()
    for mode, m in missions.items():
        m.num_episodes = 2
        torch.manual_seed(33)
        m.execute()
    tn, tt = missions["native"].trainer, missions["torch"].trainer
    return dict(records={mode: m.writer.records for mode, m in missions.items()}, counts={mode: seen[mode]["counts"] for mode in seen},
                refs=seen["torch"]["refs"], replays=[tt.step_replays, tn.step_replays], T=tn.T,
                returns={mode: m.episode_returns for mode, m in missions.items()},
                log_waves=tn.native_rollout_log().W)


def main():
    for v in SWITCHES:
        os.environ.pop(v, None)
    result = {"one": part_one(), "two": part_two(), "three": part_three(sys.argv[2])}
    with open(sys.argv[1], "w") as f:
        json.dump(result, f)


if __name__ == "__main__":
    main()
