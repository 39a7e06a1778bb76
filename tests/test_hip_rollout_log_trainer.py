"""GPU checks of ``rollout_log="native"`` above the kernels: the trainer's switch, the log of eager waves against the float64 restatement
on what the steps produced, and -- in a child process with deterministic convolutions (tests/rollout_log_recorded_rounds.py, run once for
the module) -- that the log changes nothing, that a trainer that keeps the log replays its recorded rollout with the eager log's bits, and
the mission's tags and counts.  The kernels themselves: tests/test_hip_rollout_log.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rollout_log_ref as R
from test_hip_adam_trainer import ALL_ENV, _count_lib, _params64, _trainer

pytestmark = pytest.mark.gpu

SWITCHES = ALL_ENV + ("IPPMARL_BUFFER", "IPPMARL_METRICS", "IPPMARL_ROLLOUT_LOG")
ENTRY_POINTS = ("ippm_rollout_log_bytes", "ippm_rollout_log_step", "ippm_rollout_log_finalize")


def test_switch_values(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    with pytest.raises(ValueError):
        _trainer(seed=6, n_envs=1, rollout_log="hip")
    monkeypatch.setenv("IPPMARL_ROLLOUT_LOG", "native")
    assert _trainer(seed=6, n_envs=1).rollout_log == "native"


def test_default_trainer_never_touches_the_native_log(monkeypatch):
    from ippmarl import _ffi
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    calls = {name: _count_lib(monkeypatch, name) for name in ENTRY_POINTS}
    tr = _trainer(seed=6, n_envs=1)
    tr.keep_rollout_log = True
    assert tr.rollout_log == "torch" and tr.rollout("train")["faults"] == 0
    assert tr.last_rollout is not None and tr.last_rollout["rewards"].shape == (1, tr.T)
    assert not any(calls.values()) and tr._rollout_log is None
    with pytest.raises(_ffi.IppmError):
        tr.read_rollout_log("train", 1)


def _watch(tr):
    """Wraps ``tr._rollout_step``: per step, the reward the log is defined on ([E,2]: the returned reward, or for DeepQ the last flying
    agent's row, which the native paths do not spend a gather on), env.action and env.pos[..., 2], copied to the host."""
    seen, real = [], tr._rollout_step

    def step(t, w, policy, store, eps):
        reward = real(t, w, policy, store, eps)
        if tr.deepq:
            reward = tr.last_agent_reward()
        seen.append((reward.cpu().numpy().copy(), tr.env.action.cpu().numpy().copy(), tr.env.pos[..., 2].cpu().numpy().copy()))
        return reward

    tr._rollout_step = step
    return seen


def _restate(tr, seen, waves):
    T = tr.T
    assert len(seen) == waves * T
    rew = np.stack([s[0] for s in seen]).reshape(waves, T, tr.E, 2)
    act = np.stack([s[1] for s in seen]).reshape(waves, T, tr.E, tr.N)
    alt = np.stack([s[2] for s in seen]).reshape(waves, T, tr.E, tr.N)
    d = tr.env.d
    rel, ab = rew[..., 0], rew[..., 1]
    cnt = R.counts(act, alt, tr.A, d.min_altitude, d.spacing, d.space_z, None if tr.env.n_active is None else tr.env.n_active.cpu().numpy())
    return R.scalars(rel, ab), R.scales(rel, ab), R.last_counts(cnt, tr.A, d.min_altitude, d.spacing, d.space_z), int(cnt[64])


def _check(tag, tr, seen, mode, waves):
    from ippmarl import rollout_native
    scalars, actions, altitudes, bad = tr.read_rollout_log(mode, waves)
    ref, scale, counts, ref_bad = _restate(tr, seen, waves)
    assert list(scalars) == [mode + k for k in rollout_native.KEYS]
    got, bound = np.array(list(scalars.values())), R.bound(ref, scale)
    for i, k in enumerate(scalars):
        print(f"{tag} {k:44s} got {got[i]!r} ref {ref[i]!r} |diff| {abs(got[i] - ref[i]):.3e} bound {bound[i]:.3e}")
    assert (np.abs(got - ref) <= bound).all(), (tag, got, ref, bound)
    assert actions == counts["actions"] and altitudes == counts["altitudes"] and bad == ref_bad == 0
    assert sum(actions) == sum(altitudes.values()) == waves * tr.T * (tr.E * tr.N if tr.env.n_active is None else int(tr.env.n_active.sum()))
    return got


@pytest.mark.parametrize("buffer", ["torch", "native"])
@pytest.mark.parametrize("form", ["coma", "deepq", "teams"])
def test_eager_log_is_the_restatement_of_what_the_steps_produced(monkeypatch, form, buffer):
    """Two eval waves (as a mission's evaluation: the buffer is empty), then one train wave: counts exact, scalars within ``R.bound``, and
    max / min of both return series exactly the trainer's own accumulators.  "teams" flies mixed team sizes: the agents that do not fly are
    counted nowhere."""
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    params = _params64(experiment__missions__type="DeepQ") if form == "deepq" else _params64()
    kw = dict(team_sizes=[1, 2, 2]) if form == "teams" else {}
    tr = _trainer(seed=7, n_envs=3, params=params, buffer=buffer, rollout_log="native", **kw)
    tr.keep_rollout_log = True
    tr.rollout_log_waves = 2
    steps = _count_lib(monkeypatch, "ippm_rollout_log_step")
    seen = _watch(tr)
    last = []
    for k in range(2):
        assert tr.eval_wave == k and tr.rollout("eval")["faults"] == 0
        last.append((tr.abs_ret.cpu().numpy().copy(), tr.ret.cpu().numpy().copy()))
    assert tr.eval_wave == 2 and tr.filled == 0 and len(steps) == 2 * tr.T and tr.last_rollout is None
    got = _check(f"{form}/{buffer}/eval", tr, seen, "eval", 2)
    ab, rel = np.concatenate([x[0] for x in last]).astype(np.float64), np.concatenate([x[1] for x in last]).astype(np.float64)
    assert (got[[2, 3, 10, 11]] == np.array([ab.max(), ab.min(), rel.max(), rel.min()])).all()
    assert tr.eval_wave == 0                                  # the read rewound the eval slots
    del seen[:]
    assert tr.rollout("train")["faults"] == 0
    assert len(steps) == 3 * tr.T and tr.last_rollout is None and tr.filled == 1 and tr.eval_wave == 0
    got = _check(f"{form}/{buffer}/train", tr, seen, "train", 1)
    exact = np.array([float(tr.abs_ret.max()), float(tr.abs_ret.min()), float(tr.ret.max()), float(tr.ret.min())])
    assert (got[[2, 3, 10, 11]] == exact).all(), (got, exact)


# ---- the child process: whole rounds with deterministic convolutions ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rounds(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rollout_log")
    out = tmp / "result.json"
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rollout_log_recorded_rounds.py")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    run = subprocess.run([sys.executable, script, str(out), str(tmp)], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]        # (nothing further is started after a failure)
    with open(out) as f:
        return json.load(f)


def test_the_log_changes_nothing(rounds):
    one = rounds["one"]
    assert one["buffers"][0] == one["buffers"][1] and one["params"][0] == one["params"][1]
    assert one["torch_has_rollout"] and not one["native_has_rollout"]
    native, ref, bound = (np.array(one[k]) for k in ("native", "ref", "bound"))
    assert len(native) == 12 and (np.abs(native - ref) <= bound).all(), (native, ref, bound)
    assert one["counts"] == one["ref_counts"]


def test_recorded_rollout_replays_with_the_eager_logs_bits(rounds):
    two = rounds["two"]
    assert two["replays"] == [0, 2 * two["T"]]             # the recorded trainer replayed every step of both waves; the eager one none
    assert len(two["rounds"]) == 2
    for row in two["rounds"]:
        e, r = row["eager"], row["recorded"]
        assert e["finite"] and r["finite"] and e["keys"] == r["keys"] and not e["last_rollout"] and not r["last_rollout"]
        assert e["scalars"] == r["scalars"], [(k, a, b) for k, a, b in zip(e["keys"], e["scalars"], r["scalars"]) if a != b]
        assert e["counts"] == r["counts"] and sum(e["counts"][0]) == two["rows"] and e["counts"][2] == 0
        assert e["critic"] == r["critic"] and e["actor"] == r["actor"]
        for x in (e, r):                                    # max / min of the return series are the trainer's accumulators, bit for bit
            assert [x["scalars"][i] for i in (2, 3, 10, 11)] == x["returns"]
    assert two["rounds"][0]["eager"]["scalars"] != two["rounds"][1]["eager"]["scalars"]


def test_mission_logs_the_same_tags_and_counts(rounds):
    three = rounds["three"]
    rt, rn = three["records"]["torch"], three["records"]["native"]
    assert [(tag, step) for tag, _, step in rt] == [(tag, step) for tag, _, step in rn] and len(rt) > 3 * 24
    assert three["counts"]["torch"] == three["counts"]["native"] and len(three["counts"]["native"]) == 6       # 3 rounds: train + eval
    assert three["returns"]["torch"] == three["returns"]["native"]
    # the native mission's train waves after the capture replayed their step graphs; its device log holds the evaluation's two waves
    assert three["replays"] == [0, 2 * three["T"]] and three["log_waves"] == 2
    returns = {tag: i for i, tag in enumerate(f"{k}/{s}" for k in ("Return/Episode", "Rewards/Episode", "Return/Relative(used)/Episode")
                                              for s in ("mean", "std", "max", "min"))}
    logs, seen = iter(three["refs"]), None
    for (tag, vt, step), (_, vn, _) in zip(rt, rn):
        for mode in ("train", "eval"):
            if tag.startswith(mode) and tag[len(mode):] in returns:
                i = returns[tag[len(mode):]]
                if i == 0:
                    seen = next(logs)                        # (each add_to_tensorboard call writes its twelve in order)
                ref, bound = seen[0][i], seen[1][i]
                assert abs(vn - ref) <= bound and abs(vt - ref) <= bound, (tag, step, vn, vt, ref, bound)
    assert next(logs, None) is None
