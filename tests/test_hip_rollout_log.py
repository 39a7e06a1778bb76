"""The native rollout log's kernels (csrc/rollout_log.hip) alone, on constructed inputs, against the float64 NumPy restatement
(tests/rollout_log_ref.py).

Shapes (W,T,E,N): one row, the small odd ones, and both kernels' boundaries.  The step launch gives a workgroup IPPM_ROLLOUT_ROWS = 1024
(env, agent) rows, 256 per trip of its four wavefronts: row counts E*N of 1023, 1024, 1025, 2047, 2048, 2049.  The closing launch gives a
thread L = max(2, even ceil(W*E / 256)) consecutive episodes: W*E of 128 and 129 (wavefront boundary at L = 2), 511, 512 (L = 2, all
threads), 513 (L = 4), 683 and 1023 (a ragged last thread), 1026 (L = 6).  n_actions in {4, 6, 9, 27}, altitude levels in {1, 3, 5}.

Exactness.  Sums of small integers are exact in double, so on integer-valued rewards every mean, max and min equals the restatement bit for
bit whatever the values.  A Chan merge divides by counts that are no powers of two, so a std equals the two-pass np.std bit for bit only
where that arithmetic is exact: the ``paired`` rewards give episodes 2p and 2p + 1 (wave-major order) the step rewards m + d[p,t] and
m - d[p,t] (an odd last episode holds m), so that every thread's mean of every series is the series' mean, every M2 an exact integer and
every merge has delta 0; there all 12 scalars are compared bit for bit (but for the sign of a zero).  General merges (all partial means
different) are covered by the ``general`` integers -- means, max, min bit for bit, stds at ``R.bound`` -- and by the dense rewards at
``R.bound``."""
import ctypes as C

import numpy as np
import pytest
import torch

import rollout_log_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = 1024
GUARD = 4096
MIN_ALT, SPACING = 5, 5
#        W  T  E     N   A   levels
CASES = [(1, 1, 1, 1, 4, 1), (1, 2, 3, 2, 6, 3), (2, 3, 5, 4, 9, 5),
         (1, 2, ROWS - 1, 1, 27, 3), (2, 2, ROWS // 4, 4, 6, 3), (1, 2, 205, 5, 4, 5),           # rows 1023, 1024, 1025
         (1, 2, 89, 23, 9, 1), (2, 2, 64, 32, 27, 5), (1, 3, 683, 3, 6, 3),                      # rows 2047, 2048, 2049
         (1, 2, 129, 3, 9, 3), (1, 2, 511, 1, 4, 3), (2, 2, 513, 2, 6, 5)]                        # episodes 129, 511, 1026
SMALL = CASES[:3]
STD = (1, 5, 9)
NOT_STD = (0, 2, 3, 4, 6, 7, 8, 10, 11)


def _lib():
    from ippmarl import _ffi
    return _ffi, _ffi.load_library()


def test_constants_match_the_header():
    from ippmarl import rollout_native
    assert rollout_native.ROWS == ROWS and rollout_native.SCALARS == R.N_SCALARS and rollout_native.COUNTS == R.N_COUNTS


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def _paired(rng, W, T, E, m, kmax):
    """float32 [W,T,E]: episodes 2p, 2p + 1 (wave-major) hold m + d[p,t], m - d[p,t]; an odd last episode holds m."""
    n = W * E
    d = rng.randint(-kmax, kmax + 1, size=((n + 1) // 2, T))
    x = np.stack([m + d, m - d], 1).reshape(-1, T)[:n].astype(np.float32)       # [n, T]
    if n % 2:
        x[-1] = m
    return np.ascontiguousarray(x.reshape(W, E, T).transpose(0, 2, 1))


def make_inputs(kind, W, T, E, N, A, levels, seed=0):
    """kind: "dense" (seeded, unit scale), "general" (integers in +-8), "paired" (integers in pairs of episodes around one mean)."""
    rng = np.random.RandomState(100000 * W + 10000 * T + 10 * E + N + A + levels + seed)
    if kind == "dense":
        rel, ab = (rng.standard_normal((W, T, E)).astype(np.float32) for _ in range(2))
    elif kind == "general":
        rel, ab = (rng.randint(-8, 9, size=(W, T, E)).astype(np.float32) for _ in range(2))
    else:
        rel, ab = _paired(rng, W, T, E, 3, 6), _paired(rng, W, T, E, -2, 4)
    action = rng.randint(0, A, size=(W, T, E, N)).astype(np.int32)
    z = (MIN_ALT + SPACING * rng.randint(0, levels, size=(W, T, E, N))).astype(np.int32)
    return dict(rel=rel, ab=ab, action=action, z=z)


_CACHE = {}


def case(kind, W, T, E, N, A, levels):
    """(inputs, scalars, scales, counts) of a case, computed once and shared by the tests (never written to)."""
    key = (kind, W, T, E, N, A, levels)
    if key not in _CACHE:
        x = make_inputs(*key)
        _CACHE[key] = (x, R.scalars(x["rel"], x["ab"]), R.scales(x["rel"], x["ab"]),
                       R.counts(x["action"], x["z"], A, MIN_ALT, SPACING, levels))
    return _CACHE[key]


# ---- the device side -----------------------------------------------------------------------------------------------------------------------------
def _guarded(nbytes, fill):
    """A uint8 device buffer of GUARD + nbytes + GUARD bytes filled with ``fill``; -> (whole, payload view)."""
    whole = torch.full((2 * GUARD + nbytes,), fill, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD:GUARD + nbytes]


def _guards_intact(whole, nbytes, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + nbytes:] == fill).all())


def _put(arr, fill=0x3C):
    """A NumPy array into a guarded device buffer -> (whole, payload, nbytes)."""
    arr = np.ascontiguousarray(arr)
    whole, payload = _guarded(arr.nbytes, fill)
    payload.copy_(torch.from_numpy(arr.view(np.uint8).reshape(-1)))
    return whole, payload, arr.nbytes


def run(x, W, T, E, N, A, levels, prefill=0x5A, reverse=False, n_active=None, agent_reward=None, finalize_waves=None):
    """All step calls and the closing call on the raw entry points -> (out float64 [12], counts int64 [65], every guard band intact).
    ``x``: rel, ab [W,T,E], action, z [W,T,E,N]; agent_reward [W,T,E,N,2] selects the DeepQ form."""
    ffi, lib = _lib()
    nbytes = C.c_int64(0)
    ffi.check(lib.ippm_rollout_log_bytes(W, T, E, N, C.addressof(nbytes)), "ippm_rollout_log_bytes")
    assert nbytes.value % 16 == 0
    blob_all, blob = _guarded(nbytes.value, prefill)
    res_all, res = _guarded(8 * (R.N_SCALARS + R.N_COUNTS), 0xA5)
    out_ptr, cnt_ptr = res.data_ptr(), res.data_ptr() + 8 * R.N_SCALARS
    assert blob.data_ptr() % 16 == 0 and out_ptr % 8 == 0
    reward = np.stack([x["rel"], x["ab"]], -1).astype(np.float32)                       # [W,T,E,2]
    pos = np.stack([np.full_like(x["z"], -7), np.full_like(x["z"], 1 << 30), x["z"]], -1).astype(np.int32)
    act = _put(np.asarray(n_active, np.int32)) if n_active is not None else None
    bands = [(blob_all, nbytes.value, prefill), (res_all, 8 * (R.N_SCALARS + R.N_COUNTS), 0xA5)]      # (whole, payload bytes, fill)
    if act:
        bands.append((act[0], act[2], 0x3C))
    slots = [(w, t) for w in range(W) for t in range(T)]
    for w, t in (reversed(slots) if reverse else slots):
        r, a, p = _put(reward[w, t]), _put(x["action"][w, t]), _put(pos[w, t])
        g = _put(agent_reward[w, t]) if agent_reward is not None else None
        bands += [(b[0], b[2], 0x3C) for b in (r, a, p) + ((g,) if g else ())]
        ffi.check(lib.ippm_rollout_log_step(blob.data_ptr(), w, t, W, T, r[1].data_ptr(), g[1].data_ptr() if g else None,
                                            a[1].data_ptr(), p[1].data_ptr(), act[1].data_ptr() if act else None, E, N, A, MIN_ALT,
                                            SPACING, levels, None), "ippm_rollout_log_step")
    ffi.check(lib.ippm_rollout_log_finalize(blob.data_ptr(), finalize_waves or W, T, E, N, out_ptr, cnt_ptr, None),
              "ippm_rollout_log_finalize")
    torch.cuda.synchronize()
    intact = all(_guards_intact(*b) for b in bands)
    host = res.cpu().numpy().copy()
    return host[:8 * R.N_SCALARS].view(np.float64), host[8 * R.N_SCALARS:].view(np.int64), intact


def _bits(x):
    return (np.asarray(x, dtype=np.float64) + 0.0).view(np.uint64)      # (+ 0.0: -0 and +0 are the same result)


def _report(tag, got, ref, bound):
    for i, (g, r, b) in enumerate(zip(got, ref, bound)):
        print(f"{tag} [{i:2d}] got {g!r} ref {r!r} |diff| {abs(g - r):.3e} bound {b:.3e}")


def _assert_within(tag, got, ref, scale, idx=range(12)):
    bound = R.bound(ref, scale)
    _report(tag, got, ref, bound)
    for i in idx:
        assert abs(got[i] - ref[i]) <= bound[i], (tag, i, got[i], ref[i], bound[i])


# ---- tests ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,T,E,N,A,levels", CASES)
def test_paired_integer_rewards_bit_for_bit(W, T, E, N, A, levels):
    x, ref, scale, cref = case("paired", W, T, E, N, A, levels)
    out, cnt, intact = run(x, W, T, E, N, A, levels)
    assert intact
    _report("paired", out, ref, R.bound(ref, scale))
    assert (_bits(out) == _bits(ref)).all(), (out, ref)
    assert (cnt == cref).all() and cnt[64] == 0 and cnt[:32].sum() == cnt[32:64].sum() == W * T * E * N


@pytest.mark.parametrize("W,T,E,N,A,levels", CASES)
def test_general_integer_rewards(W, T, E, N, A, levels):
    x, ref, scale, cref = case("general", W, T, E, N, A, levels)
    out, cnt, intact = run(x, W, T, E, N, A, levels)
    assert intact and (cnt == cref).all()
    _report("general", out, ref, R.bound(ref, scale))
    assert (_bits(out[list(NOT_STD)]) == _bits(ref[list(NOT_STD)])).all(), (out, ref)
    _assert_within("general", out, ref, scale, STD)


@pytest.mark.parametrize("W,T,E,N,A,levels", CASES)
def test_dense_rewards_within_bound(W, T, E, N, A, levels):
    x, ref, scale, cref = case("dense", W, T, E, N, A, levels)
    out, cnt, intact = run(x, W, T, E, N, A, levels)
    assert intact and (cnt == cref).all()
    _assert_within("dense", out, ref, scale)
    # max and min of every series are elements of it: exact
    assert (_bits(out[[2, 3, 6, 7, 10, 11]]) == _bits(ref[[2, 3, 6, 7, 10, 11]])).all()


@pytest.mark.parametrize("W,T,E,N,A,levels", [CASES[0], CASES[2], CASES[8]])
def test_constant_series_has_std_zero(W, T, E, N, A, levels):
    x = dict(case("dense", W, T, E, N, A, levels)[0])
    x["rel"] = np.full((W, T, E), 0.1, np.float32)
    x["ab"] = np.full((W, T, E), -2.5, np.float32)
    out, _, _ = run(x, W, T, E, N, A, levels)
    ref = R.scalars(x["rel"], x["ab"])
    for i in STD:
        assert _bits(out[i]) == _bits(0.0), (i, out[i])
    assert (_bits(out[list(NOT_STD)]) == _bits(ref[list(NOT_STD)])).all(), (out, ref)


@pytest.mark.parametrize("W,T,E,N,A,levels", [CASES[2], CASES[5], CASES[11]])
def test_same_bits_whatever_the_blob_held_and_the_call_order(W, T, E, N, A, levels):
    x = case("dense", W, T, E, N, A, levels)[0]
    first = run(x, W, T, E, N, A, levels)
    for other in (run(x, W, T, E, N, A, levels, prefill=0xFF), run(x, W, T, E, N, A, levels, reverse=True), run(x, W, T, E, N, A, levels)):
        assert (first[0].view(np.uint64) == other[0].view(np.uint64)).all() and (first[1] == other[1]).all() and other[2]


def test_a_prefix_of_the_waves():
    """The blob is wave-major: a closing call that names fewer waves reduces those first waves."""
    W, T, E, N, A, levels = CASES[2]
    x = case("dense", W, T, E, N, A, levels)[0]
    out, cnt, _ = run(x, W, T, E, N, A, levels, finalize_waves=1)
    one = {k: v[:1] for k, v in x.items()}
    alone = run(one, 1, T, E, N, A, levels)
    assert (out.view(np.uint64) == alone[0].view(np.uint64)).all() and (cnt == alone[1]).all()


@pytest.mark.parametrize("W,T,E,N,A,levels", [CASES[2], CASES[6], CASES[8]])
def test_mixed_team_sizes_count_flying_agents_only(W, T, E, N, A, levels):
    x, ref, scale, _ = case("general", W, T, E, N, A, levels)
    n_active = np.random.RandomState(E).randint(1, N + 1, size=E).astype(np.int32)
    x = dict(x)
    flying = np.arange(N)[None, :] < n_active[:, None]
    # rows that do not fly hold what would be counted wrongly or read out of range if they were looked at
    x["action"] = np.where(flying, x["action"], 1 << 30).astype(np.int32)
    x["z"] = np.where(flying, x["z"], -(1 << 31)).astype(np.int32)
    out, cnt, intact = run(x, W, T, E, N, A, levels, n_active=n_active)
    cref = R.counts(x["action"], x["z"], A, MIN_ALT, SPACING, levels, n_active)
    assert intact and (cnt == cref).all() and cnt[64] == 0
    assert cnt[:32].sum() == cnt[32:64].sum() == W * T * int(n_active.sum())
    assert (_bits(out[list(NOT_STD)]) == _bits(ref[list(NOT_STD)])).all()


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("W,T,E,N,A,levels", [CASES[1], CASES[2], CASES[5]])
def test_deepq_form_takes_the_last_flying_agent(W, T, E, N, A, levels, mixed):
    x = dict(case("general", W, T, E, N, A, levels)[0])
    rng = np.random.RandomState(7 * E + N)
    agent_reward = rng.randint(-8, 9, size=(W, T, E, N, 2)).astype(np.float32)
    n_active = rng.randint(1, N + 1, size=E).astype(np.int32) if mixed else None
    rows = R.last_flying_rows(agent_reward, n_active)
    out, cnt, intact = run(x, W, T, E, N, A, levels, n_active=n_active, agent_reward=agent_reward)     # (x's own rewards must be ignored)
    ref = R.scalars(rows[..., 0], rows[..., 1])
    assert intact
    assert (_bits(out[list(NOT_STD)]) == _bits(ref[list(NOT_STD)])).all(), (out, ref)
    _assert_within("deepq", out, ref, R.scales(rows[..., 0], rows[..., 1]), STD)
    assert (cnt == R.counts(x["action"], x["z"], A, MIN_ALT, SPACING, levels, n_active)).all()


@pytest.mark.parametrize("W,T,E,N,A,levels", [CASES[1], CASES[2], CASES[5]])
def test_bad_rows_land_in_the_last_count_only(W, T, E, N, A, levels):
    x, ref, _, good = case("general", W, T, E, N, A, levels)
    x = dict(x, action=x["action"].copy(), z=x["z"].copy())
    flat_a, flat_z = x["action"].reshape(-1), x["z"].reshape(-1)
    n = flat_a.size
    bad_a = {0: -1, n - 1: A, n // 2: 1 << 30} if n > 2 else {0: -1}
    bad_z = {0: MIN_ALT + 1, n - 1: MIN_ALT + SPACING * levels, n // 3: MIN_ALT - SPACING, n // 2: -(1 << 31)} if n > 3 else {0: MIN_ALT + 1}
    for i, v in bad_a.items():
        flat_a[i] = v
    for i, v in bad_z.items():
        flat_z[i] = v
    out, cnt, intact = run(x, W, T, E, N, A, levels)
    cref = R.counts(x["action"], x["z"], A, MIN_ALT, SPACING, levels)
    assert intact and (cnt == cref).all()
    assert cnt[64] == len(bad_a) + len(bad_z)
    assert cnt[:32].sum() == n - len(bad_a) and cnt[32:64].sum() == n - len(bad_z)
    assert (cnt[:64] <= good[:64]).all() and (cnt[A:32] == 0).all() and (cnt[32 + levels:64] == 0).all()
    assert (_bits(out[list(NOT_STD)]) == _bits(ref[list(NOT_STD)])).all()          # the statistics do not see them


@pytest.mark.parametrize("column", ["ab", "rel"])
def test_non_finite_rewards_stay_in_their_series(column):
    """A NaN and an Inf in the absolute column reach the four scalars of the absolute returns and nothing else; in the relative column they
    reach the step rewards and the relative returns, the two series that column enters, and leave the absolute returns alone."""
    W, T, E, N, A, levels = CASES[2]
    x, ref, scale, cref = case("dense", W, T, E, N, A, levels)
    x = dict(x, **{column: x[column].copy()})
    x[column][0, 1, 2] = np.nan
    x[column][1, 0, 3] = np.inf
    out, cnt, intact = run(x, W, T, E, N, A, levels)
    hit = (0, 1, 2, 3) if column == "ab" else tuple(range(4, 12))
    clean = [i for i in range(12) if i not in hit]
    assert intact and (cnt == cref).all()
    assert not np.isfinite(out[list(hit)]).any(), out
    assert np.isnan(R.scalars(x["rel"], x["ab"])[list(hit)]).all() and np.isnan(out[list(hit)]).all()      # np.max / np.min keep the NaN
    assert np.isfinite(out[clean]).all()
    _assert_within("clean series", out, ref, scale, clean)


def test_an_inf_alone_is_numpys():
    W, T, E, N, A, levels = CASES[2]
    x = dict(case("dense", W, T, E, N, A, levels)[0])
    x["ab"] = x["ab"].copy()
    x["ab"][1, 2, 0] = -np.inf
    out, _, _ = run(x, W, T, E, N, A, levels)
    ref = R.scalars(x["rel"], x["ab"])
    assert out[0] == ref[0] == -np.inf and np.isnan(out[1]) and np.isnan(ref[1]) and out[2] == ref[2] and out[3] == ref[3] == -np.inf


def test_argument_errors_launch_nothing():
    ffi, lib = _lib()
    W, T, E, N, A, levels = 2, 3, 5, 4, 6, 3
    nbytes = C.c_int64(0)
    ffi.check(lib.ippm_rollout_log_bytes(W, T, E, N, C.addressof(nbytes)), "ippm_rollout_log_bytes")
    blob = torch.zeros(nbytes.value + 16, dtype=torch.uint8, device=DEV)
    res = torch.full((R.N_SCALARS + R.N_COUNTS,), 7, dtype=torch.int64, device=DEV)
    f = torch.ones(E * N * 2, device=DEV)
    i = torch.zeros(E * N * 3, dtype=torch.int32, device=DEV)
    bp, fp, ip, op, cp = blob.data_ptr(), f.data_ptr(), i.data_ptr(), res.data_ptr(), res.data_ptr() + 8 * R.N_SCALARS
    nb = C.addressof(nbytes)

    def step(log=bp, wave=0, step=0, waves=W, steps=T, reward=fp, agent=None, action=ip, pos=ip, active=None, envs=E, agents=N, actions=A,
             spacing=SPACING, lv=levels):
        return lib.ippm_rollout_log_step(log, wave, step, waves, steps, reward, agent, action, pos, active, envs, agents, actions, MIN_ALT,
                                         spacing, lv, None)

    def fin(log=bp, waves=W, steps=T, envs=E, agents=N, out=op, counts=cp):
        return lib.ippm_rollout_log_finalize(log, waves, steps, envs, agents, out, counts, None)

    bad = [
        lib.ippm_rollout_log_bytes(W, T, E, N, None), lib.ippm_rollout_log_bytes(0, T, E, N, nb), lib.ippm_rollout_log_bytes(4097, T, E, N, nb),
        lib.ippm_rollout_log_bytes(W, 0, E, N, nb), lib.ippm_rollout_log_bytes(W, 4097, E, N, nb), lib.ippm_rollout_log_bytes(W, T, 0, N, nb),
        lib.ippm_rollout_log_bytes(W, T, (1 << 20) + 1, N, nb), lib.ippm_rollout_log_bytes(W, T, E, 0, nb),
        lib.ippm_rollout_log_bytes(W, T, E, 33, nb),
        step(log=None), step(reward=None), step(action=None), step(pos=None), step(wave=-1), step(wave=W), step(step=-1), step(step=T),
        step(waves=0), step(waves=4097), step(steps=0), step(steps=4097), step(envs=0), step(envs=(1 << 20) + 1), step(agents=0),
        step(agents=33), step(actions=1), step(actions=33), step(lv=0), step(lv=33), step(spacing=0), step(spacing=-5),
        step(log=bp + 8), step(reward=fp + 2), step(agent=fp + 1), step(action=ip + 2), step(pos=ip + 1), step(active=ip + 3),
        fin(log=None), fin(out=None), fin(counts=None), fin(waves=0), fin(waves=4097), fin(steps=0), fin(envs=0), fin(agents=0), fin(agents=33),
        fin(log=bp + 8), fin(out=op + 4), fin(counts=cp + 4),
    ]
    assert bad == [-1] * len(bad), bad
    assert lib.ippm_last_error().decode().startswith("ippm_rollout_log_finalize")
    torch.cuda.synchronize()
    assert bool((res == 7).all()) and not bool(blob.any())          # nothing was launched: the outputs and the blob are untouched
