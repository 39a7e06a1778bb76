"""The rollout log of ``COMAMission.add_to_tensorboard`` restated in float64 NumPy straight from the definitions: the reference the native
rollout log (csrc/rollout_log.hip) is judged against.  Rewards are float32 arrays [W,T,E] (waves, steps, envs); an episode's return is the
float32 sum of its step rewards in step order, starting from the first one; every statistic is ``np.mean / np.std / np.max / np.min`` of the
float32 series converted to double.  Order of the 12 scalars: ``metrics.return_scalars`` (``ippmarl.rollout_native.KEYS``).  Counts follow
the rules of include/ippmarl.h: 65 integers, [0,32) actions, [32,64) altitude levels, [64] the entries that fall in no bin.

``bound(ref, scale) = 1e-9 (|ref| + mean |input|)`` is the project's bound of tests/metrics_native_ref.py: the inputs are exact in double,
reordering a sum of n <= 7e4 terms moves it by at most n 2^-53 ~ 8e-12 of sum |x|, and the Chan merges stay inside two orders of margin.
The largest series any test of the rollout log reduces has 2052 terms (the step rewards of tests/test_hip_rollout_log.py's shape
(W,T,E) = (2,2,513); the trainer and mission tests stay below 2 waves x 15 steps x 3 envs), far below the 7e4 of that derivation.
``scales`` gives, per scalar, the mean magnitude of the elements of its series."""
import numpy as np

N_SCALARS = 12
N_COUNTS = 65


def returns(col):
    """float32 [W,T,E] -> float32 [W,E]: cumulative float32 adds over the steps, starting from the first reward."""
    col = np.asarray(col, dtype=np.float32)
    ret = col[:, 0].copy()
    with np.errstate(all="ignore"):
        for t in range(1, col.shape[1]):
            ret = (ret + col[:, t]).astype(np.float32)
    return ret


def series(rel, ab):
    """The three series, as float64 vectors: absolute returns, per-step relative rewards, relative returns."""
    return [returns(ab).astype(np.float64).ravel(), np.asarray(rel, np.float32).astype(np.float64).ravel(),
            returns(rel).astype(np.float64).ravel()]


def scalars(rel, ab):
    """rel, ab float32 [W,T,E] -> float64 [12]."""
    out = []
    with np.errstate(all="ignore"):
        for x in series(rel, ab):
            out += [np.mean(x), np.std(x), np.max(x), np.min(x)]
    return np.array(out, dtype=np.float64)


def scales(rel, ab):
    """Per scalar, the mean magnitude of the (finite) elements of its series."""
    out = []
    for x in series(rel, ab):
        fin = np.abs(x[np.isfinite(x)])
        out += [float(fin.mean()) if fin.size else 0.0] * 4
    return np.array(out, dtype=np.float64)


def bound(ref, scale):
    return 1e-9 * (np.abs(ref) + scale)


def last_flying_rows(agent_reward, n_active=None):
    """DeepQ: agent_reward float32 [W,T,E,N,2] -> reward [W,T,E,2], the row of the last agent that flies in each env."""
    agent_reward = np.asarray(agent_reward, dtype=np.float32)
    W, T, E, N, _ = agent_reward.shape
    last = np.full(E, N - 1) if n_active is None else np.asarray(n_active).astype(np.int64) - 1
    return agent_reward[:, :, np.arange(E), last, :]


def counts(action, altitude, n_actions, min_altitude, spacing, n_levels, n_active=None):
    """action, altitude int [W,T,E,N] -> int64 [65].  An agent a >= n_active[e] is counted nowhere; an action outside [0, n_actions) and an
    altitude whose level (z - min_altitude) / spacing is no integer in [0, n_levels) add one to counts[64] each."""
    action = np.asarray(action).astype(np.int64)
    altitude = np.asarray(altitude).astype(np.int64)
    W, T, E, N = action.shape
    flying = np.ones((E, N), bool) if n_active is None else np.arange(N)[None, :] < np.asarray(n_active).reshape(E, 1)
    flying = np.broadcast_to(flying, action.shape)
    a, z = action[flying], altitude[flying]
    out = np.zeros(N_COUNTS, dtype=np.int64)
    a_ok = (a >= 0) & (a < n_actions)
    d = z - min_altitude
    z_ok = (d >= 0) & (d % spacing == 0) & (d // spacing < n_levels)
    out[:32] = np.bincount(a[a_ok], minlength=32)
    out[32:64] = np.bincount(d[z_ok] // spacing, minlength=32)
    out[64] = int((~a_ok).sum()) + int((~z_ok).sum())
    return out


def last_counts(cnt, n_actions, min_altitude, spacing, n_levels):
    """int64 [65] -> the mission's ``last_counts``: every action's count, and {metres: count} of the altitude levels that occur."""
    cnt = [int(c) for c in cnt]
    return {"actions": cnt[:n_actions], "altitudes": {min_altitude + k * spacing: c for k, c in enumerate(cnt[32:32 + n_levels]) if c}}
