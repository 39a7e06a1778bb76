"""GPU checks of the native Adam step (csrc/optim.hip behind ippm_adam_state_bytes, ippm_adam_init and ippm_adam_step), through ctypes.  The
reference of every number is the restated contract (tests/adam_ref.py), never the code under test: the float32 restatement bit for bit, and
MARGIN spreads (float32 against float64 restatement of the same case) around the float64 one."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096                 # sentinel floats before and after every buffer
SENTINEL = -12345.678
ZERO_GRAD = 1
COUNTER_BYTES = 64
SETS = {"one": [1], "around-a-wavefront": [3, 255, 256, 257], "around-a-chunk": [4099, 1, 65537],
        "sixteen": [1, 2, 3, 5, 1023, 1024, 1025, 2047, 2048, 2049, 7, 300, 4096, 31, 64, 100]}


def _lib():
    from ippmarl import _ffi
    return _ffi, _ffi.load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def net_shapes(planes, A):
    return [(256, planes, 5, 5), (256,), (256, 256, 4, 4), (256,), (256, 256, 4, 4), (256,), (256, 256), (256,), (A, 256), (A,)]


class _Floats:
    """n floats between two bands of GUARD sentinels."""

    def __init__(self, values):
        values = np.asarray(values, dtype=np.float32).reshape(-1)
        self.n = values.size
        self.whole = torch.full((self.n + 2 * GUARD,), SENTINEL, device=DEV)
        self.t = self.whole[GUARD:GUARD + self.n]
        self.t.copy_(torch.from_numpy(values))

    def intact(self):
        return bool((self.whole[:GUARD] == SENTINEL).all()) and bool((self.whole[GUARD + self.n:] == SENTINEL).all())

    def bits(self):
        return self.t.cpu().numpy().view(np.uint32)


class _Bytes:
    """n bytes of ``fill`` between two bands of 4 * GUARD bytes of 0xA5."""

    def __init__(self, n, fill=0xFF):
        self.n = n
        self.whole = torch.full((n + 8 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.t = self.whole[4 * GUARD:4 * GUARD + n]
        self.t.fill_(fill)

    def intact(self):
        return bool((self.whole[:4 * GUARD] == 0xA5).all()) and bool((self.whole[4 * GUARD + self.n:] == 0xA5).all())

    def numpy(self):
        return self.t.cpu().numpy()


def _state_bytes(numel):
    _ffi, lib = _lib()
    arr = (C.c_int64 * len(numel))(*numel)
    nbytes = C.c_int64(0)
    _ffi.check(lib.ippm_adam_state_bytes(arr, len(numel), C.addressof(nbytes)), "ippm_adam_state_bytes")
    assert nbytes.value == COUNTER_BYTES + sum(2 * ((n + 3) // 4 * 16) for n in numel)      # the header's layout
    return nbytes.value


class _Run:
    """Parameters, gradients, the state blob (pre-filled with 0xFF, then initialised) and optionally a pack, all guarded."""

    def __init__(self, shapes, seed, pack=None, state_fill=0xFF):
        _ffi, lib = _lib()
        self.shapes = [tuple(s) if isinstance(s, (tuple, list)) else (s,) for s in shapes]
        self.numel = [int(np.prod(s)) for s in self.shapes]
        self.n = len(self.numel)
        self.p0 = R.parameters(seed, self.shapes)
        self.p = [_Floats(p) for p in self.p0]
        self.g = [_Floats(np.zeros(n)) for n in self.numel]
        self.c_numel = (C.c_int64 * self.n)(*self.numel)
        self.blob = _Bytes(_state_bytes(self.numel), state_fill)
        self.pack = self.planes = None
        self.A = 0
        if pack is not None:
            self.planes, self.A = pack
            nbytes = C.c_int64(0)
            fn = lib.ippm_actor_pack_bytes if self.planes == 7 else lib.ippm_critic_pack_bytes
            _ffi.check(fn(self.A, C.addressof(nbytes)), "pack_bytes")
            self.pack = _Bytes(nbytes.value, 0xFF)
        self.init()

    def init(self):
        _ffi, lib = _lib()
        _ffi.check(lib.ippm_adam_init(self.blob.t.data_ptr(), self.c_numel, self.n, _stream()), "ippm_adam_init")

    def pointers(self):
        return ((C.c_void_p * self.n)(*[x.t.data_ptr() for x in self.p]), (C.c_void_p * self.n)(*[x.t.data_ptr() for x in self.g]))

    def launch(self, lr, flags=ZERO_GRAD, with_pack=True, betas=R.BETAS, eps=R.EPS):
        _ffi, lib = _lib()
        ps, gs = self.pointers()
        packed = self.pack.t.data_ptr() if (self.pack is not None and with_pack) else None
        _ffi.check(lib.ippm_adam_step(self.blob.t.data_ptr(), ps, gs, self.c_numel, self.n, lr, betas[0], betas[1], eps, flags,
                                      self.planes if packed else 0, self.A if packed else 0, packed, _stream()), "ippm_adam_step")

    def step(self, grads, lr, **kw):
        for dst, g in zip(self.g, grads):
            dst.t.copy_(torch.from_numpy(np.asarray(g, dtype=np.float32).reshape(-1)))
        self.launch(lr, **kw)

    def read(self):
        torch.cuda.synchronize()
        raw = self.blob.numpy()
        out = {"t": int(raw[0:8].view(np.int64)[0]), "b1p": float(raw[8:16].view(np.float64)[0]), "b2p": float(raw[16:24].view(np.float64)[0]),
               "ticket": int(raw[24:28].view(np.uint32)[0]), "raw": raw.copy(), "p": [x.t.cpu().numpy() for x in self.p], "m": [], "v": []}
        off = COUNTER_BYTES
        for n in self.numel:
            span = (n + 3) // 4 * 16
            out["m"].append(raw[off:off + 4 * n].view(np.float32).copy())
            out["v"].append(raw[off + span:off + span + 4 * n].view(np.float32).copy())
            off += 2 * span
        return out

    def intact(self):
        torch.cuda.synchronize()
        return all(x.intact() for x in self.p + self.g + [self.blob] + ([self.pack] if self.pack is not None else []))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def _same_bits(got, ref32, what):
    """p, m, v and the counters of the device against the float32 restatement, as bits; the first of m, v, p that differs names the
    operation chain that disagrees."""
    assert got["t"] == ref32.t and got["ticket"] == 0, (what, got["t"], got["ticket"])
    assert np.float64(got["b1p"]).view(np.uint64) == np.float64(ref32.b1p).view(np.uint64), (what, got["b1p"], ref32.b1p)
    assert np.float64(got["b2p"]).view(np.uint64) == np.float64(ref32.b2p).view(np.uint64), (what, got["b2p"], ref32.b2p)
    for k in ("m", "v", "p"):
        for i, (a, b) in enumerate(zip(got[k], getattr(ref32, k))):
            differ = int((_bits(a) != _bits(b)).sum())
            assert differ == 0, f"{what}: {differ} of {a.size} elements of {k}[{i}] differ from the float32 restatement's bits"


# ---- 1. bit for bit against the float32 restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr", [1e-4, 1e-3])
@pytest.mark.parametrize("name", list(SETS))
def test_steps_equal_the_float32_restatement_bit_for_bit(name, lr):
    """After 1, 2 and 20 steps p, m, v and the counters are the float32 restatement's bits -- every operation of the contract is a correctly
    rounded IEEE operation on normal numbers -- and within MARGIN spreads of the float64 restatement."""
    shapes = SETS[name]
    run = _Run(shapes, seed=3)
    a32, a64 = R.Adam(run.p0, lr, np.float32), R.Adam(run.p0, lr, np.float64)
    for s in range(1, 21):
        grads = R.gradients(1000 + s, run.shapes)
        run.step(grads, lr)
        a32.step(grads)
        a64.step(grads)
        if s in (1, 2, 20):
            got = run.read()
            _same_bits(got, a32, f"{name} lr {lr} after {s} steps")
            spread, err = R.spreads(a32, a64), R.errors({k: got[k] for k in "pmv"}, a64)
            print(f"{name} lr {lr} step {s}: spreads {spread}, device errors {err}")
            for k in err:
                assert err[k] <= R.MARGIN * spread[k], (name, s, k, err[k], spread[k])
    assert run.intact()


# ---- 2. gradient zeroing ------------------------------------------------------------------------------------------------------------------
def test_zero_grad_flag():
    run = _Run(SETS["around-a-chunk"], seed=4)
    grads = R.gradients(7, run.shapes, zeros=0.0)
    run.step(grads, 1e-3, flags=0)
    torch.cuda.synchronize()
    for x, g in zip(run.g, grads):
        assert np.array_equal(x.bits(), _bits(g))                      # flag clear: the gradients keep their bits
    run.step(grads, 1e-3, flags=ZERO_GRAD)
    torch.cuda.synchronize()
    for x in run.g:
        assert not x.bits().any()                                       # every gradient is +0.0
    assert run.read()["t"] == 2 and run.intact()


# ---- 3. guard bands, determinism, init --------------------------------------------------------------------------------------------------------
def test_guard_bands_determinism_and_init():
    shapes = SETS["sixteen"]
    outs = []
    for fill in (0xFF, 0x00):
        run = _Run(shapes, seed=5, state_fill=fill)
        fresh = run.read()
        assert fresh["t"] == 0 and fresh["b1p"] == 1.0 and fresh["b2p"] == 1.0 and fresh["ticket"] == 0
        assert not fresh["raw"][28:].any()                                # padding and every moment: zero bytes, whatever the blob held
        for s in range(3):
            run.step(R.gradients(50 + s, run.shapes), 1e-3)
        outs.append(run.read())
        assert run.intact()
    assert np.array_equal(outs[0]["raw"], outs[1]["raw"])               # two runs from the same state: the same bits
    for a, b in zip(outs[0]["p"], outs[1]["p"]):
        assert np.array_equal(_bits(a), _bits(b))
    run.init()                                                           # ... and init on a used blob gives a fresh one
    again = run.read()
    assert again["t"] == 0 and again["b1p"] == 1.0 and again["b2p"] == 1.0 and not again["raw"][28:].any()
    assert np.array_equal(again["raw"][:28], fresh["raw"][:28])


def test_pack_run_guards():
    """The network-sized launch with a pack: guard bands around every parameter, gradient, the state blob and the pack stay untouched."""
    run = _Run(net_shapes(7, 6), seed=6, pack=(7, 6))
    run.step(R.gradients(8, run.shapes), 1e-3)
    assert run.intact() and run.read()["t"] == 1


# ---- 4. non-finite values ---------------------------------------------------------------------------------------------------------------------
def _class(x):
    return "nan" if np.isnan(x) else ("+inf" if x == np.inf else "-inf" if x == -np.inf else "finite")


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_gradient_reaches_its_own_element_only(bad):
    lr, tensor, at = 1e-3, 2, 40000
    clean, dirty = _Run(SETS["around-a-chunk"], seed=9), _Run(SETS["around-a-chunk"], seed=9)
    a32 = R.Adam(clean.p0, lr, np.float32)
    warm = R.gradients(60, clean.shapes)
    grads = R.gradients(61, clean.shapes)
    poisoned = [g.copy() for g in grads]
    poisoned[tensor].reshape(-1)[at] = bad
    for run in (clean, dirty):
        run.step(warm, lr)
    clean.step(grads, lr)
    dirty.step(poisoned, lr)
    a32.step(warm).step(poisoned)
    c, d = clean.read(), dirty.read()
    for k in "pmv":
        for i in range(len(clean.numel)):
            differ = np.nonzero(_bits(c[k][i]) != _bits(d[k][i]))[0]
            assert list(differ) == ([at] if i == tensor else []), (k, i, differ[:5])
        assert _class(d[k][tensor][at]) == _class(getattr(a32, k)[tensor].reshape(-1)[at]) != "finite", k
    assert d["t"] == c["t"] == 2 and d["b1p"] == c["b1p"] and clean.intact() and dirty.intact()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_gradient_reaches_its_own_pack_element_only(bad):
    lr, tensor, at = 1e-3, 2, 256 * 16 * 3 + 16 * 5 + 7               # conv2.w[3, 5, tap 7] -> pack row 3, k = 7 * 256 + 5
    shapes = net_shapes(12, 4)
    clean, dirty = _Run(shapes, seed=10, pack=(12, 4)), _Run(shapes, seed=10, pack=(12, 4))
    grads = R.gradients(62, clean.shapes)
    poisoned = [g.copy() for g in grads]
    poisoned[tensor].reshape(-1)[at] = bad
    clean.step(grads, lr)
    dirty.step(poisoned, lr)
    c, d = clean.read(), dirty.read()
    for k in "pmv":
        for i in range(len(clean.numel)):
            differ = np.nonzero(_bits(c[k][i]) != _bits(d[k][i]))[0]
            assert list(differ) == ([at] if i == tensor else []), (k, i, differ[:5])
    assert np.isnan(d["p"][tensor][at])
    pc, pd = clean.pack.numpy().view(np.uint16), dirty.pack.numpy().view(np.uint16)
    w2 = 256 * 320                                                       # conv2's rows follow conv1's 256 rows of padded K = 320
    assert list(np.nonzero(pc != pd)[0]) == [w2 + 3 * 4096 + 7 * 256 + 5]
    assert (pd[w2 + 3 * 4096 + 7 * 256 + 5] & 0x7FFF) > 0x7F80           # a bf16 NaN
    assert clean.intact() and dirty.intact()


# ---- 5. the pack ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [4, 6, 9, 27])
@pytest.mark.parametrize("planes", [7, 12])
def test_pack_equals_the_pack_entry_point_on_the_stepped_parameters(planes, A):
    """After a step with ``packed`` pre-filled with 0xFF the blob equals ippm_actor_pack / ippm_critic_pack of the stepped parameters byte
    for byte, and the parameters (and moments) equal those of a step without a pack."""
    _ffi, lib = _lib()
    shapes = net_shapes(planes, A)
    with_pack, without = _Run(shapes, seed=11, pack=(planes, A)), _Run(shapes, seed=11)
    grads = R.gradients(70 + A, with_pack.shapes)
    for s in range(2):
        with_pack.pack.t.fill_(0xFF if s == 0 else 0x5A)                 # no precondition on what the pack held
        with_pack.step(grads, 1e-3)
        without.step(grads, 1e-3)
    a, b = with_pack.read(), without.read()
    assert np.array_equal(a["raw"], b["raw"])
    for x, y in zip(a["p"], b["p"]):
        assert np.array_equal(_bits(x), _bits(y))
    want = _Bytes(with_pack.pack.n, 0x00)
    fn = lib.ippm_actor_pack if planes == 7 else lib.ippm_critic_pack
    _ffi.check(fn(*[x.t.data_ptr() for x in with_pack.p], A, want.t.data_ptr(), _stream()), "pack")
    torch.cuda.synchronize()
    got, ref = with_pack.pack.numpy(), want.numpy()
    differ = np.nonzero(got != ref)[0]
    assert differ.size == 0, f"{differ.size} of {got.size} pack bytes differ, the first at {differ[:4]}"
    assert with_pack.intact() and want.intact()
    for g in with_pack.g:
        assert not g.bits().any()


# ---- 6. argument errors -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    """Every error returns -1 with a message that names the entry point, and launches nothing: parameters, gradients, state and pack keep
    their bytes."""
    _ffi, lib = _lib()
    run = _Run(net_shapes(7, 6), seed=12, pack=(7, 6))
    for dst, g in zip(run.g, R.gradients(13, run.shapes)):
        dst.t.copy_(torch.from_numpy(g.reshape(-1)))
    small = _Run([5, 9], seed=14)
    before = run.read()
    before_g = [x.bits().copy() for x in run.g]
    nbytes = C.c_int64(0)
    stream = _stream()

    def fails(rc, name, word):
        msg = lib.ippm_last_error().decode()
        assert rc == -1 and name in msg and word in msg, (rc, name, word, msg)

    name = "ippm_adam_state_bytes"
    two = (C.c_int64 * 2)(5, 9)
    fails(lib.ippm_adam_state_bytes(None, 2, C.addressof(nbytes)), name, "null")
    fails(lib.ippm_adam_state_bytes(two, 2, None), name, "null")
    for bad in (0, -1, 17):
        fails(lib.ippm_adam_state_bytes(two, bad, C.addressof(nbytes)), name, "n_tensors")
    for bad in (0, -3):
        fails(lib.ippm_adam_state_bytes((C.c_int64 * 2)(5, bad), 2, C.addressof(nbytes)), name, "numel")
    name = "ippm_adam_init"
    fails(lib.ippm_adam_init(None, two, 2, stream), name, "null")
    fails(lib.ippm_adam_init(small.blob.t.data_ptr(), None, 2, stream), name, "null")
    fails(lib.ippm_adam_init(small.blob.t.data_ptr(), two, 0, stream), name, "n_tensors")
    fails(lib.ippm_adam_init(small.blob.t.data_ptr(), (C.c_int64 * 2)(0, 9), 2, stream), name, "numel")
    fails(lib.ippm_adam_init(small.blob.t.data_ptr() + 8, two, 2, stream), name, "16-byte aligned")

    name = "ippm_adam_step"
    ps, gs = run.pointers()
    ok = [run.blob.t.data_ptr(), ps, gs, run.c_numel, run.n, 1e-3, 0.9, 0.999, 1e-8, ZERO_GRAD, 7, 6, run.pack.t.data_ptr(), stream]

    def bad_call(word, **slots):
        call = list(ok)
        for slot, value in slots.items():
            call[int(slot[1:])] = value
        fails(lib.ippm_adam_step(*call), name, word)

    for slot in (0, 1, 2, 3):
        bad_call("null", **{f"s{slot}": None})
    holes = (C.c_void_p * run.n)(*[x.t.data_ptr() for x in run.p])
    holes[4] = None
    bad_call("null", s1=holes)
    bad_call("null", s2=holes)
    for bad in (0, -1, 17):
        bad_call("n_tensors", s4=bad)
    numel = (C.c_int64 * run.n)(*run.numel)
    numel[3] = 0
    bad_call("numel", s3=numel)
    bad_call("16-byte aligned", s0=ok[0] + 8)
    bad_call("16-byte aligned", s12=ok[12] + 4)
    for bad in (3, -7, 8, 1):
        bad_call("pack_planes", s10=bad)
    bad_call("pack_planes", s10=0)                                        # a pack without planes ...
    bad_call("pack_planes", s12=None)                                     # ... and planes without a pack
    bad_call("n_tensors = 10", s4=9)
    numel = (C.c_int64 * run.n)(*run.numel)
    numel[1] = 255
    bad_call("sizes", s3=numel)
    bad_call("sizes", s10=12)                                             # the actor's tensors are not the critic's
    bad_call("sizes", s11=7)                                              # fc3 has 6 rows
    for bad in (0, -1, 33):
        bad_call("n_actions", s11=bad)
    for bad in (float("nan"), float("inf"), -1e-3):
        bad_call("lr", s5=bad)
        bad_call("eps", s8=bad)
    for bad in (1.0, -0.1, 1.5, float("nan")):
        bad_call("beta", s6=bad)
        bad_call("beta", s7=bad)
    bad_call("flags", s9=2)

    after = run.read()                                                    # nothing was launched
    assert np.array_equal(before["raw"], after["raw"]) and after["t"] == 0
    for a, b in zip(before["p"], after["p"]):
        assert np.array_equal(_bits(a), _bits(b))
    for x, b in zip(run.g, before_g):
        assert np.array_equal(x.bits(), b)
    assert bool((run.pack.t == 0xFF).all()) and run.intact() and small.intact()
    assert lib.ippm_adam_step(*ok) == 0                                   # ... and the good call is one
    assert run.read()["t"] == 1 and run.intact()


# ---- 7. capture -----------------------------------------------------------------------------------------------------------------------------
def test_recorded_step_replayed_equals_eager_steps():
    """One step recorded with torch.cuda.graph and replayed three times equals three eager steps bit for bit, counters included: nothing the
    host passes changes from step to step."""
    shapes, lr = SETS["around-a-chunk"], 1e-3
    grads = R.gradients(90, [(n,) for n in shapes], zeros=0.0)
    eager, rec = _Run(shapes, seed=15), _Run(shapes, seed=15)
    for run in (eager, rec):
        for dst, g in zip(run.g, grads):
            dst.t.copy_(torch.from_numpy(g))
    for _ in range(3):
        eager.launch(lr, flags=0)                                          # (flag clear: every step reads the same gradients)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rec.launch(lr, flags=0)
    torch.cuda.synchronize()
    assert rec.read()["t"] == 0                                            # recording executes nothing
    for _ in range(3):
        graph.replay()
    e, r = eager.read(), rec.read()
    assert e["t"] == r["t"] == 3 and np.array_equal(e["raw"], r["raw"])
    for a, b in zip(e["p"], r["p"]):
        assert np.array_equal(_bits(a), _bits(b))
    a32 = R.Adam(eager.p0, lr, np.float32)
    for _ in range(3):
        a32.step(grads)
    _same_bits(r, a32, "replayed")
    assert eager.intact() and rec.intact()
