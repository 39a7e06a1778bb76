"""CPU checks around the native rollout log: the float64 restatement (tests/rollout_log_ref.py) IS the mission's log -- on random data it
equals ``metrics.return_scalars`` plus the count expressions of ``COMAMission.add_to_tensorboard`` -- and the switch, the constants and the
trainer's signature are what the header and the documents say."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import rollout_log_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _last_rollouts(rel, ab, action, z):
    """What COMATrainer.rollout keeps per wave on the torch path: returns by float32 adds, rewards [E,T], actions and altitudes [E,T,N]."""
    waves = []
    for w in range(rel.shape[0]):
        ret, abs_ret = torch.zeros(rel.shape[2]), torch.zeros(rel.shape[2])
        for t in range(rel.shape[1]):
            ret += torch.from_numpy(rel[w, t])
            abs_ret += torch.from_numpy(ab[w, t])
        waves.append(dict(episode_returns=ret, absolute_returns=abs_ret, rewards=torch.from_numpy(rel[w]).T.contiguous(),
                          actions=torch.from_numpy(action[w]).permute(1, 0, 2).contiguous(),
                          altitudes=torch.from_numpy(z[w]).permute(1, 0, 2).contiguous()))
    return waves


@pytest.mark.parametrize("W,T,E,N,A,levels", [(1, 1, 1, 1, 4, 1), (1, 2, 3, 2, 6, 3), (2, 3, 5, 4, 9, 5), (3, 15, 5, 4, 27, 3)])
def test_restatement_is_the_missions_log(W, T, E, N, A, levels):
    from ippmarl import metrics, rollout_native
    rng = np.random.RandomState(W + 10 * T + 100 * E)
    rel, ab = (rng.standard_normal((W, T, E)).astype(np.float32) for _ in range(2))
    action = rng.randint(0, A, size=(W, T, E, N)).astype(np.int32)
    z = (5 + 5 * rng.randint(0, levels, size=(W, T, E, N))).astype(np.int32)
    rollouts = _last_rollouts(rel, ab, action, z)
    # COMAMission.add_to_tensorboard's expressions
    cat = lambda key: torch.cat([r[key].flatten() for r in rollouts]).cpu()  # noqa: E731
    actions, altitudes = cat("actions"), cat("altitudes")
    last_counts = {"actions": [int((actions == a).sum()) for a in range(A)],
                   "altitudes": {int(v): int((altitudes == v).sum()) for v in torch.unique(altitudes)}}
    scalars = metrics.return_scalars("train", cat("absolute_returns"), cat("rewards"), cat("episode_returns"))
    assert list(scalars) == ["train" + k for k in rollout_native.KEYS]
    ref, scale = R.scalars(rel, ab), R.scales(rel, ab)
    got = np.array(list(scalars.values()))
    assert (np.abs(got - ref) <= R.bound(ref, scale)).all(), (got, ref)
    assert (got[[2, 3, 6, 7, 10, 11]] == ref[[2, 3, 6, 7, 10, 11]]).all()          # max / min: elements of the float32 series, exact
    cnt = R.counts(action, z, A, 5, 5, levels)
    assert R.last_counts(cnt, A, 5, 5, levels) == last_counts and cnt[64] == 0 and cnt.sum() == 2 * W * T * E * N


def test_count_rules():
    """Non-flying agents nowhere; an action outside the table and an altitude off the lattice or outside it into counts[64] only."""
    action = np.array([[[[0, 5], [-1, 2], [6, 1 << 30]]]], dtype=np.int32)          # [1,1,3,2]
    z = np.array([[[[5, 10], [7, 0], [20, -(1 << 31)]]]], dtype=np.int64)
    cnt = R.counts(action, z, 6, 5, 5, 3)
    assert cnt[:6].tolist() == [1, 0, 1, 0, 0, 1] and cnt[6:32].sum() == 0
    assert cnt[32:35].tolist() == [1, 1, 0] and cnt[35:64].sum() == 0 and cnt[64] == 3 + 4
    cnt = R.counts(action, z, 6, 5, 5, 3, n_active=[1, 2, 1])
    assert cnt[:6].tolist() == [1, 0, 1, 0, 0, 0] and cnt[32:35].tolist() == [1, 0, 0] and cnt[64] == 2 + 3
    assert R.last_counts(cnt, 6, 5, 5, 3) == {"actions": [1, 0, 1, 0, 0, 0], "altitudes": {5: 1}}


def test_returns_are_float32_adds_in_step_order():
    col = np.array([[[1e8], [1.0], [1.0], [-1e8]]], dtype=np.float32)              # [1,4,1]: 1e8 + 1 rounds back to 1e8 in float32
    assert R.returns(col).dtype == np.float32 and R.returns(col)[0, 0] == 0.0
    assert R.scalars(col, col)[0] == 0.0 and R.scalars(col, col)[4] == 0.5
    rows = R.last_flying_rows(np.arange(2 * 3 * 2, dtype=np.float32).reshape(1, 1, 2, 3, 2), n_active=[2, 3])
    assert rows.tolist() == [[[[2.0, 3.0], [10.0, 11.0]]]]


def test_resolve_mode(monkeypatch):
    from ippmarl import rollout_native
    monkeypatch.delenv(rollout_native.ENV_VAR, raising=False)
    assert rollout_native.ENV_VAR == "IPPMARL_ROLLOUT_LOG" and rollout_native.MODES == ("torch", "native")
    assert rollout_native.resolve_mode() == "torch" and rollout_native.resolve_mode("native") == "native"
    monkeypatch.setenv(rollout_native.ENV_VAR, "native")
    assert rollout_native.resolve_mode() == "native" and rollout_native.resolve_mode("torch") == "torch"
    monkeypatch.setenv(rollout_native.ENV_VAR, "")
    assert rollout_native.resolve_mode() == "torch"
    for bad in ("hip", "Native", ""):
        with pytest.raises(ValueError):
            rollout_native.resolve_mode(bad)
    monkeypatch.setenv(rollout_native.ENV_VAR, "device")
    with pytest.raises(ValueError):
        rollout_native.resolve_mode()


def test_constants_are_the_headers():
    from ippmarl import _ffi, rollout_native
    header = open(os.path.join(ROOT, "include", "ippmarl.h")).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", header).group(1))  # noqa: E731
    assert rollout_native.SCALARS == define("IPPM_ROLLOUT_SCALARS") == R.N_SCALARS == len(rollout_native.KEYS) == 12
    assert rollout_native.COUNTS == define("IPPM_ROLLOUT_COUNTS") == R.N_COUNTS == 65
    assert rollout_native.ROWS == define("IPPM_ROLLOUT_ROWS")
    for name in ("ippm_rollout_log_bytes", "ippm_rollout_log_step", "ippm_rollout_log_finalize"):
        assert name in _ffi.PROTOTYPES and re.search(rf"\bint {name}\(", header)
    assert len(_ffi.PROTOTYPES["ippm_rollout_log_step"]) == 17 and len(_ffi.PROTOTYPES["ippm_rollout_log_finalize"]) == 8


def test_trainer_has_the_switch():
    from ippmarl.trainer import COMATrainer
    sig = inspect.signature(COMATrainer.__init__)
    assert "rollout_log" in sig.parameters and sig.parameters["rollout_log"].default is None
    assert hasattr(COMATrainer, "read_rollout_log") and hasattr(COMATrainer, "native_rollout_log")


def test_native_log_is_gpu_only():
    from ippmarl import _ffi, rollout_native
    with pytest.raises(_ffi.IppmError):
        rollout_native.NativeRolloutLog(1, 15, 5, 4, 6, 5, 5, 3, "cpu")
