"""GPU checks of every bf16 matrix-core entry point -- ippm_actor_forward, ippm_critic_forward (ippm_bf16_net.h), ippm_conv4x4_bf16_*,
ippm_conv5x5_bf16_*, ippm_head_forward / _backward, ippm_critic_loss, ippm_actor_loss -- on operands that need rounding in an interesting
way and on operands that are not finite (round to nearest even, NaN stays NaN, overflow gives Inf; NaN and Inf
propagate as in the IEEE arithmetic of the definition; padding contributes nothing).  Inputs, dependence sets and expectations are
tests/bf16_operand_classes_ref.py's, whose every expected value is the float64 restatement of the entry point's own module; no comparison
here has a tolerance: finite values bit for bit, non-finite ones by class.

The harness is the one of the entry points' own test files: outputs pre-filled with NaN between two bands of GUARD sentinels, a scratch
of 0xFF bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import actor_native_ref as AR
import bf16_operand_classes_ref as R
import test_hip_conv2_train as T4
import test_hip_head_update as TH
import test_hip_trunk_update as T5

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, SENTINEL = TH.GUARD, TH.SENTINEL


def _network(kind, a):
    """ippm_actor_pack / _forward (eps = 0) or ippm_critic_pack / _forward on guarded, NaN-filled outputs and a 0xFF-filled pack and
    scratch -> {"logits", "probs"} or {"q"} on the CPU."""
    from ippmarl import _ffi
    lib = _ffi.load_library()
    A, x = a["A"], a["x"].to(DEV).contiguous()
    B = x.shape[0]
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = C.c_int64(0)
    _ffi.check(getattr(lib, f"ippm_{kind}_pack_bytes")(A, C.addressof(nbytes)), "pack_bytes")
    packed = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device=DEV)
    params = [t.to(DEV).contiguous() for name in AR.TRUNK + ("fc3",) for t in a["net"][name]]
    _ffi.check(getattr(lib, f"ippm_{kind}_pack")(*[t.data_ptr() for t in params], A, packed.data_ptr(), stream), "pack")
    _ffi.check(getattr(lib, f"ippm_{kind}_scratch_bytes")(B, C.addressof(nbytes)), "scratch_bytes")
    scratch = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device=DEV)
    if kind == "actor":
        g = TH._Guarded(probs=(B, A), logits=(B, A))
        _ffi.check(lib.ippm_actor_forward(packed.data_ptr(), x.data_ptr(), B, A, 0.0, None, scratch.data_ptr(), g.ptr("probs"), g.ptr("logits"),
                                          stream), "ippm_actor_forward")
    else:
        g = TH._Guarded(q=(B, A))
        _ffi.check(lib.ippm_critic_forward(packed.data_ptr(), x.data_ptr(), B, A, None, scratch.data_ptr(), g.ptr("q"), None, stream),
                   "ippm_critic_forward")
    return g.collect()


def _run(entry, a):
    """One entry point on the arguments of bf16_operand_classes_ref.restate -> {output: float32 tensor on the CPU}; every runner asserts
    rc == 0 and intact guard bands."""
    if entry.startswith("conv4x4"):
        op = entry.split(".")[1]
        first, second = {"y": ("x", "w"), "gx": ("gy", "w"), "gw": ("gy", "x")}[op]
        shape = R.restate_shapes(entry, a)[op].shape
        B, ih, iw = (a["x"].shape if "x" in a else (shape[0], shape[1], shape[2]))[:3]
        return {op: T4._run(op, a[first], a[second], B, ih, iw)}
    if entry == "conv5x5.y":
        return {"y": T5._forward(a["x"], a["w"], a.get("bias"))}
    if entry == "conv5x5.gw":
        return {"gw": T5._grad_weight(a["gy"], a["x"])}
    if entry == "head.forward":
        return TH._forward(a["h"], a["w1"], a["b1"], a["w3"], a["b3"])
    if entry == "head.backward":
        return TH._backward(a["dlogits"], None if a["scale"] == 1.0 else a["scale"], a["a1"], a["h"], a["w1"], a["w3"])
    if entry == "critic_loss":
        return TH._critic_loss(a["q"], a["action"], a["td"])
    if entry == "actor_loss":
        return TH._actor_loss(a["logits"], a["q_values"], a["mask"], a["action"], a["eps"])
    return _network(entry, a)


def _first_sample(entry, a):
    """batch 1 of a network case: its first sample"""
    return dict(a, x=a["x"][:1])


# ---- Part A: rounding classes through every rounded operand ------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(R.ROUNDING_CASES))
def test_rounding_classes(case_id):
    case = R.rounding_case(case_id)
    want = R.rounding_expected(case_id)
    runs = [(case.args, want)]
    if case.entry in R.PLANES:                               # the networks: batch 17 and batch 1
        runs.append((_first_sample(case.entry, case.args), {k: v[:1] for k, v in want.items()}))
    for args, ref in runs:
        got = _run(case.entry, args)
        assert set(got) == set(ref)
        bad = {k: R.disagreements(got[k], ref[k], exact=k not in R.BY_CLASS_ONLY) for k in ref}
        for k in ref:
            print(f"{case_id} {k}: {bad[k]} of {ref[k].numel()} elements differ in class or bits; "
                  f"{int((R.classes(ref[k].float()) != R.FINITE).sum())} expected non-finite")
        assert not any(bad.values()), (case_id, bad)


# ---- Part B: one poisoned element ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean_runs():
    cache = {}

    def run(base):
        if base not in cache:
            cache[base] = _run(*R.poison_base(base))
        return cache[base]

    return run


@pytest.mark.parametrize("site", list(R.POISON_SITES))
def test_one_poisoned_element(clean_runs, site):
    base = site.split("/")[0]
    clean = clean_runs(base)
    for k, v in clean.items():
        assert bool(torch.isfinite(v).all()), (site, k)
    failures = []
    for p in R.POISONS:
        entry, args, bad, operand, idx = R.poison_case(f"{site}/{p}")
        want, deps = R.poison_expected(f"{site}/{p}"), R.depends(entry, args, operand, idx)
        got = _run(entry, bad)                                # (asserts the guard bands)
        for k in want:
            wrong_class = int((R.classes(got[k]) != R.classes(want[k].float())).sum())
            moved = int((~R.same_bits(got[k], clean[k]))[~deps[k]].sum())
            print(f"{site}/{p} {k}: {wrong_class} elements of another class than the restatement's; {moved} of {int((~deps[k]).sum())} "
                  f"unconnected elements moved; {int((R.classes(want[k].float()) != R.FINITE).sum())} of {want[k].numel()} expected non-finite")
            if wrong_class or moved:
                failures.append((p, k, wrong_class, moved))
        if p == "nan" and entry in ("critic_loss", "actor_loss"):
            assert bool(torch.isnan(got["loss"])), (site, "the loss of a poisoned row is not NaN")
    assert not failures, (site, failures)
