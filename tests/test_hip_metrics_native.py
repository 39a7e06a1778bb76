"""GPU checks of csrc/metrics.hip through the raw C entry points, against the float64 restatement (tests/metrics_native_ref.py).

Shapes: one row pair, the reference's minibatch (60 x 6) alone and as five slots, and the chunk boundary from below, on it, above it and
past two chunks, with n_actions 2, 4, 9, 27 and 32 (wavefronts of the column pass with one, two and eight columns each).

Exactness.  Sums of small integers are exact in double, so on integer inputs every mean, the minimum and the L1 norms equal the
restatement bit for bit whatever the inputs.  A second-moment merge (Chan) divides by counts that are no powers of two as soon as a chunk is
ragged, so it equals a two-pass evaluation bit for bit only where the arithmetic is exact: the ``paired`` inputs put every array in pairs
(m + k, m - k) (an odd tail holds m), so that every partial mean of every tree is m and every M2 an exact integer; there the stds and the
explained variance are compared bit for bit too.  General merges (all partial means different) are covered by the dense inputs at the
derived bound ``R.bound`` and by the ``general`` integer inputs at the same bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import metrics_native_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNK = 256
CASES = [(1, 2, 2), (1, 60, 6), (5, 60, 6), (3, CHUNK - 1, 4), (2, CHUNK, 9), (2, CHUNK + 1, 27), (2, 2 * CHUNK + 3, 32)]
GRAD_NUMEL = (7, 1, 4099, 5, 70001, 256, 1000, 3, 64 * 4 + 1, 2)       # one lane-strided tensor, sizes off every quad and part boundary
GUARD = 4096
TRANSCENDENTAL = (12, 22, 23, 24)                                        # log / exp enter: never bit for bit against NumPy
MEANS_MIN_L1 = (0, 1, 3, 4, 5, 8, 10, 13, 14, 15, 16, 17, 18, 19, 20, 25, 26, 27, 28, 29, 30, 31)
MOMENTS = (2, 6, 7, 9, 11, 21)


def _lib():
    from ippmarl import _ffi
    return _ffi, _ffi.load_library()


def test_constants_match_the_header():
    from ippmarl import metrics_native
    assert CHUNK == metrics_native.CHUNK and metrics_native.SCALARS == R.N_SCALARS == 32


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def _pairs(rng, n, m, kmax):
    """n integers in pairs (m + k, m - k), k in [0, kmax]; an odd tail holds m."""
    k = rng.randint(0, kmax + 1, size=(n + 1) // 2)
    x = np.stack([m + k, m - k], 1).reshape(-1)[:n].astype(np.float32)
    if n % 2:
        x[-1] = m
    return x


def make_inputs(kind, nb, B, A, seed=0):
    """kind: "dense" (seeded, unit scale), "general" (integers in +-8), "paired" (integers in +-8 in pairs around one mean per array)."""
    rng = np.random.RandomState(1000 * nb + 10 * B + A + seed)
    f32 = np.float32
    ints = lambda *shape: rng.randint(-8, 9, size=shape).astype(f32)  # noqa: E731
    soft = lambda: (lambda z: (np.exp(z) / np.exp(z).sum(1, keepdims=True)).astype(f32))(rng.standard_normal((B, A)))  # noqa: E731
    c = dict(loss=[], q_chosen=[], td=[], disc=[], q_new=[], action=[])
    a = dict(loss=[], adv=[], probs=[], action=[], hidden0=[], probs_after=[])
    for _ in range(nb):
        action = rng.randint(0, A, size=B).astype(np.int32)
        if kind == "dense":
            c["loss"].append(f32(rng.random_sample())); c["q_chosen"].append(rng.standard_normal(B).astype(f32))
            c["td"].append(rng.standard_normal(B).astype(f32)); c["disc"].append(rng.standard_normal(B).astype(f32))
            c["q_new"].append(rng.standard_normal((B, A)).astype(f32))
            a["loss"].append(f32(rng.standard_normal())); a["adv"].append(rng.standard_normal(B).astype(f32))
            a["hidden0"].append(rng.random_sample(256).astype(f32))
        elif kind == "general":
            c["loss"].append(f32(rng.randint(0, 9))); c["q_chosen"].append(ints(B)); c["td"].append(ints(B)); c["disc"].append(ints(B))
            c["q_new"].append(ints(B, A))
            a["loss"].append(f32(rng.randint(-8, 9))); a["adv"].append(ints(B)); a["hidden0"].append(ints(256))
        else:
            # td around 2, disc around 5 (>= 2), q_chosen around -4 (<= -1): disc - td = 3 +- (k - k'), |disc - q_chosen| = 9 +- (k - k')
            c["loss"].append(f32(rng.randint(0, 9))); c["td"].append(_pairs(rng, B, 2, 6)); c["disc"].append(_pairs(rng, B, 5, 3))
            c["q_chosen"].append(_pairs(rng, B, -4, 3))
            c["q_new"].append(np.stack([_pairs(rng, A, -1, 7) for _ in range(B)]))
            a["loss"].append(f32(rng.randint(-8, 9))); a["adv"].append(_pairs(rng, B, 1, 7)); a["hidden0"].append(ints(256))
        c["action"].append(action)
        a["action"].append(action)
        a["probs"].append(soft())
        a["probs_after"].append(soft())
    grads = [[(rng.standard_normal(n).astype(f32) if kind == "dense" else ints(n)) for n in GRAD_NUMEL] for _ in range(2)]
    return c, a, grads[0], grads[1]


_CACHE = {}


def case(kind, nb, B, A):
    """(inputs, restatement, scales) of a case, computed once and shared by the tests (never written to)."""
    key = (kind, nb, B, A)
    if key not in _CACHE:
        inputs = make_inputs(kind, nb, B, A)
        _CACHE[key] = (inputs, R.all_scalars(*inputs), R.scales(*inputs))
    return _CACHE[key]


# ---- the device side -----------------------------------------------------------------------------------------------------------------------------
def _guarded(nbytes, fill):
    """A uint8 device buffer of GUARD + nbytes + GUARD bytes filled with ``fill``; -> (whole, payload view)."""
    whole = torch.full((2 * GUARD + nbytes,), fill, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD:GUARD + nbytes]


def _guards_intact(whole, nbytes, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + nbytes:] == fill).all())


def run(inputs, nb, B, A, prefill=0x5A, slot_order=None, misalign_grads=False):
    """All calls of a round on the raw entry points -> (out float64 [32] as NumPy, guard bands intact)."""
    ffi, lib = _lib()
    c, a, cg, ag = inputs
    dev = lambda x, dt=torch.float32: torch.as_tensor(np.asarray(x), dtype=dt).to(DEV).contiguous()  # noqa: E731
    nbytes = C.c_int64(0)
    ffi.check(lib.ippm_metrics_bytes(nb, B, A, C.addressof(nbytes)), "ippm_metrics_bytes")
    blob_all, blob = _guarded(nbytes.value, prefill)
    out_all, out = _guarded(32 * 8, 0xA5)
    assert blob.data_ptr() % 16 == 0 and out.data_ptr() % 8 == 0
    keep = []
    for s in (slot_order if slot_order is not None else range(nb)):
        t = [dev(np.reshape(c["loss"][s], 1)), dev(c["q_chosen"][s]), dev(c["td"][s]), dev(c["disc"][s]), dev(c["q_new"][s]),
             dev(c["action"][s], torch.int32)]
        ffi.check(lib.ippm_metrics_critic(blob.data_ptr(), s, nb, *[x.data_ptr() for x in t], B, A, None), "ippm_metrics_critic")
        u = [dev(np.reshape(a["loss"][s], 1)), dev(a["adv"][s]), dev(a["probs"][s]), dev(a["action"][s], torch.int32), dev(a["hidden0"][s])]
        ffi.check(lib.ippm_metrics_actor(blob.data_ptr(), s, nb, *[x.data_ptr() for x in u], B, A, None), "ippm_metrics_actor")
        v = dev(a["probs_after"][s])
        ffi.check(lib.ippm_metrics_actor_after(blob.data_ptr(), s, nb, u[2].data_ptr(), v.data_ptr(), B, A, None), "ippm_metrics_actor_after")
        keep += t + u + [v]
    for net, grads in ((1, ag), (0, cg)) if slot_order is not None else ((0, cg), (1, ag)):
        if misalign_grads:      # the same values one float off a 16-byte boundary: the dword path must add in the same order
            gs = [torch.cat([torch.zeros(1, device=DEV), dev(g)])[1:] for g in grads]
            assert all(g.data_ptr() % 16 == 4 for g in gs)
        else:
            gs = [dev(g) for g in grads]
        ptrs = (C.c_void_p * 10)(*[g.data_ptr() for g in gs])
        numel = (C.c_int64 * 10)(*[g.numel() for g in gs])
        ffi.check(lib.ippm_metrics_grad_l1(blob.data_ptr(), net, ptrs, numel, 10, None), "ippm_metrics_grad_l1")
        keep += gs
    ffi.check(lib.ippm_metrics_finalize(blob.data_ptr(), nb, B, A, out.data_ptr(), None), "ippm_metrics_finalize")
    torch.cuda.synchronize()
    intact = _guards_intact(blob_all, nbytes.value, prefill) and _guards_intact(out_all, 32 * 8, 0xA5)
    return out.view(torch.float64).cpu().numpy().copy(), intact


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _report(tag, got, ref, bound):
    for i, (g, r, b) in enumerate(zip(got, ref, bound)):
        print(f"{tag} [{i:2d}] got {g!r} ref {r!r} |diff| {abs(g - r):.3e} bound {b:.3e}")


def _assert_within(tag, got, ref, scale, idx):
    bound = R.bound(ref, scale)
    _report(tag, got, ref, bound)
    for i in idx:
        assert (np.isnan(got[i]) and np.isnan(ref[i])) or abs(got[i] - ref[i]) <= bound[i], (tag, i, got[i], ref[i], bound[i])


# ---- tests ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,B,A", CASES)
def test_paired_integers_bit_for_bit(nb, B, A):
    inputs, ref, scale = case("paired", nb, B, A)
    got, intact = run(inputs, nb, B, A)
    assert intact
    _report("paired", got, ref, R.bound(ref, scale))
    for i in MEANS_MIN_L1 + MOMENTS:
        assert _bits(got[i]) == _bits(ref[i]), (i, got[i], ref[i])
    _assert_within("paired", got, ref, scale, TRANSCENDENTAL)
    assert got[17] == 0.0 and got[30] == 0.0                       # fc2


@pytest.mark.parametrize("nb,B,A", CASES)
def test_general_integers(nb, B, A):
    inputs, ref, scale = case("general", nb, B, A)
    got, intact = run(inputs, nb, B, A)
    assert intact
    for i in MEANS_MIN_L1:
        assert _bits(got[i]) == _bits(ref[i]), (i, got[i], ref[i])
    _assert_within("general", got, ref, scale, MOMENTS + TRANSCENDENTAL)


@pytest.mark.parametrize("nb,B,A", [(1, 2, 2), (5, 60, 6), (2, CHUNK + 1, 27)])
def test_constant_td_and_the_zero_rules(nb, B, A):
    c, a, cg, ag = case("paired", nb, B, A)[0]
    const = lambda v: [np.full(B, v, np.float32) for _ in range(nb)]  # noqa: E731
    # a constant td: std exactly 0
    got, _ = run((dict(c, td=const(3.0)), a, cg, ag), nb, B, A)
    assert _bits(got[2]) == _bits(0.0) and got[1] == 3.0
    # a constant disc: variance exactly 0 -> 1.0 when the residual's is 0 too (td = disc - 2), else 0.0
    got, _ = run((dict(c, disc=const(5.0), td=const(3.0)), a, cg, ag), nb, B, A)
    assert _bits(got[7]) == _bits(1.0) and _bits(got[9]) == _bits(0.0)
    got, _ = run((dict(c, disc=const(5.0)), a, cg, ag), nb, B, A)
    want = 1.0 if all(np.all(t == t[0]) for t in c["td"]) and len({float(t[0]) for t in c["td"]}) == 1 else 0.0
    assert _bits(got[7]) == _bits(want)
    assert want == 0.0 or B == 2                                        # (the paired td varies wherever it has room to)


@pytest.mark.parametrize("nb,B,A", CASES)
def test_dense_within_the_derived_bound(nb, B, A):
    inputs, ref, scale = case("dense", nb, B, A)
    got, intact = run(inputs, nb, B, A)
    assert intact
    _assert_within("dense", got, ref, scale, range(32))


@pytest.mark.parametrize("nb,B,A", [(1, 2, 2), (5, 60, 6), (2, 2 * CHUNK + 3, 32)])
def test_same_bits_across_runs_blob_contents_and_call_order(nb, B, A):
    inputs = case("dense", nb, B, A)[0]
    first, ok1 = run(inputs, nb, B, A)
    again, ok2 = run(inputs, nb, B, A)
    ones, ok3 = run(inputs, nb, B, A, prefill=0xFF)
    rev, ok4 = run(inputs, nb, B, A, slot_order=list(range(nb))[::-1], misalign_grads=True)
    assert ok1 and ok2 and ok3 and ok4                                 # the 4096-byte guard bands around the blob and out
    for other in (again, ones, rev):
        assert np.array_equal(_bits(first), _bits(other)), np.nonzero(_bits(first) != _bits(other))


def test_non_finite_inputs_reach_their_scalars_only():
    nb, B, A = 5, 60, 6
    c, a, cg, ag = case("dense", nb, B, A)[0]
    clean, _ = run((c, a, cg, ag), nb, B, A)
    assert np.isfinite(clean).all()
    td = [x.copy() for x in c["td"]]
    td[3][17] = np.nan
    got, _ = run((dict(c, td=td), a, cg, ag), nb, B, A)
    hit = np.isnan(got)
    assert sorted(np.nonzero(hit)[0]) == [1, 2, 7] and np.array_equal(_bits(got[~hit]), _bits(clean[~hit]))
    probs = [x.copy() for x in a["probs"]]
    probs[1][9, a["action"][1][9]] = np.nan                           # at the chosen action: log-chosen sees it too
    got, _ = run((c, dict(a, probs=probs), cg, ag), nb, B, A)
    hit = np.isnan(got)
    assert sorted(np.nonzero(hit)[0]) == [22, 23, 24] and np.array_equal(_bits(got[~hit]), _bits(clean[~hit]))


def test_argument_errors_launch_nothing():
    ffi, lib = _lib()
    nb, B, A = 2, 60, 6
    nbytes = C.c_int64(0)
    ffi.check(lib.ippm_metrics_bytes(nb, B, A, C.addressof(nbytes)), "ippm_metrics_bytes")
    blob = torch.zeros(nbytes.value + 16, dtype=torch.uint8, device=DEV)
    out = torch.full((32,), 7.0, dtype=torch.float64, device=DEV)
    f = torch.ones(B * A, device=DEV)
    act = torch.zeros(B, dtype=torch.int32, device=DEV)
    h = torch.ones(256, device=DEV)
    p, bp = f.data_ptr(), blob.data_ptr()
    ptrs = (C.c_void_p * 10)(*([p] * 10))
    numel = (C.c_int64 * 10)(*([4] * 10))
    critic = lambda acc=bp, slot=0, n=nb, loss=p, batch=B, actions=A: lib.ippm_metrics_critic(  # noqa: E731
        acc, slot, n, loss, p, p, p, p, act.data_ptr(), batch, actions, None)
    actor = lambda acc=bp, slot=0, probs=p, batch=B, actions=A: lib.ippm_metrics_actor(  # noqa: E731
        acc, slot, nb, p, p, probs, act.data_ptr(), h.data_ptr(), batch, actions, None)
    after = lambda acc=bp, slot=0, old=p, batch=B, actions=A: lib.ippm_metrics_actor_after(acc, slot, nb, old, p, batch, actions, None)  # noqa: E731
    bad = [
        lib.ippm_metrics_bytes(nb, B, A, None), lib.ippm_metrics_bytes(0, B, A, C.addressof(nbytes)),
        lib.ippm_metrics_bytes(nb, 1, A, C.addressof(nbytes)), lib.ippm_metrics_bytes(nb, B, 1, C.addressof(nbytes)),
        lib.ippm_metrics_bytes(nb, B, 33, C.addressof(nbytes)),
        critic(acc=None), critic(loss=None), critic(batch=1), critic(actions=1), critic(actions=33), critic(slot=-1), critic(slot=nb),
        critic(acc=bp + 8), critic(loss=p + 2),
        actor(acc=None), actor(probs=None), actor(batch=1), actor(actions=1), actor(actions=33), actor(slot=-1), actor(slot=nb), actor(acc=bp + 8),
        after(acc=None), after(old=None), after(batch=1), after(actions=1), after(actions=33), after(slot=-1), after(slot=nb), after(acc=bp + 8),
        lib.ippm_metrics_grad_l1(None, 0, ptrs, numel, 10, None), lib.ippm_metrics_grad_l1(bp, 0, None, numel, 10, None),
        lib.ippm_metrics_grad_l1(bp, 0, ptrs, None, 10, None), lib.ippm_metrics_grad_l1(bp, 0, ptrs, numel, 9, None),
        lib.ippm_metrics_grad_l1(bp, 0, ptrs, numel, 11, None), lib.ippm_metrics_grad_l1(bp, 2, ptrs, numel, 10, None),
        lib.ippm_metrics_grad_l1(bp + 8, 0, ptrs, numel, 10, None),
        lib.ippm_metrics_grad_l1(bp, 0, (C.c_void_p * 10)(*([p] * 9 + [None])), numel, 10, None),
        lib.ippm_metrics_grad_l1(bp, 0, ptrs, (C.c_int64 * 10)(*([4] * 9 + [0])), 10, None),
        lib.ippm_metrics_finalize(None, nb, B, A, out.data_ptr(), None), lib.ippm_metrics_finalize(bp, nb, B, A, None, None),
        lib.ippm_metrics_finalize(bp, 0, B, A, out.data_ptr(), None), lib.ippm_metrics_finalize(bp, nb, 1, A, out.data_ptr(), None),
        lib.ippm_metrics_finalize(bp, nb, B, 1, out.data_ptr(), None), lib.ippm_metrics_finalize(bp, nb, B, 33, out.data_ptr(), None),
        lib.ippm_metrics_finalize(bp + 8, nb, B, A, out.data_ptr(), None), lib.ippm_metrics_finalize(bp, nb, B, A, out.data_ptr() + 4, None),
    ]
    assert bad == [-1] * len(bad), bad
    assert lib.ippm_last_error().decode().startswith("ippm_metrics_finalize")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and not bool(blob.any())          # nothing was launched: out and the blob are untouched
