"""CPU checks of tests/bf16_operand_classes_ref.py, the inputs and expectations of test_hip_bf16_operand_classes.py: the pattern lists are
what they claim to be, the selectors select, the float32 and the float64 restatement agree on every rounding case (so accumulation order
cannot excuse a device difference), and the dependence sets of the poison cases hold in the restatement itself."""
import math

import numpy as np
import pytest
import torch

import bf16_operand_classes_ref as R


def _rne_bf16(bits):
    """round to nearest even in integer arithmetic, independent of torch: float32 bits -> bf16 bits (no NaN among the patterns)"""
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) & 0xFFFF


# ---- the patterns -------------------------------------------------------------------------------------------------------------------------
def test_named_patterns_round_as_stated():
    for bits, want in R.NAMED.items():
        for sign in (0, 0x80000000):
            b = bits | sign
            assert _rne_bf16(b) == want | (sign >> 16), hex(b)
            x = torch.from_numpy(np.array([b], dtype=np.uint32).view(np.float32).copy())
            got = int(x.to(torch.bfloat16).view(torch.int16).item()) & 0xFFFF
            assert got == want | (sign >> 16), (hex(b), hex(got))                       # the restatements' .to(torch.bfloat16)
    # the classes the lists must hold
    assert {0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3FFF8000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0x00800000, 0} <= set(R.PATTERNS["nonneg-all"])
    assert 0x80000000 in R.PATTERNS["signed-all"]


@pytest.mark.parametrize("which", sorted(R.PATTERNS))
def test_pattern_lists(which):
    bits = R.PATTERNS[which]
    n = len(bits)
    assert n % 2 == 1 and math.gcd(n, 8) == 1 and len(set(bits)) == n
    for b in bits:
        exponent = (b >> 23) & 0xFF
        assert exponent != 0xFF and (exponent != 0 or b & 0x7FFFFFFF == 0), hex(b)      # finite, and no float32 subnormal
    rounds_to_inf = [b for b in bits if _rne_bf16(b) & 0x7FFF == 0x7F80]
    assert bool(rounds_to_inf) == which.endswith("all")
    if which.startswith("nonneg"):
        assert all(b < 0x80000000 for b in bits)
    else:
        assert {b ^ 0x80000000 for b in bits if b != 0x3E000000} == {b for b in bits if b != 0x3E000000}
    # cycled over a flat index every pattern meets every slot of the 2-wide and the 8-wide conversion groups
    t = R.cycled((8 * n,), which)
    idx = torch.arange(8 * n)
    assert len({(int(i) % 8, int(i) % n) for i in idx}) == 8 * n
    assert torch.equal(t.view(torch.int32)[:n], R.pattern_values(which).view(torch.int32))


def test_disagreements_counts_classes_and_bits():
    inf, nan = float("inf"), float("nan")
    want = torch.tensor([1.0, 0.0, inf, -inf, nan, 2.0], dtype=torch.float64)
    assert R.disagreements(torch.tensor([1.0, -0.0, inf, -inf, nan, 2.0]), want) == 0
    assert R.disagreements(torch.tensor([1.0, 0.0, -inf, -inf, nan, 2.0]), want) == 1
    assert R.disagreements(torch.tensor([1.0, 0.0, inf, -inf, 0.0, 2.0]), want) == 1
    assert R.disagreements(torch.tensor([1.0, 0.0, inf, nan, nan, 2.0]), want) == 1
    assert R.disagreements(torch.tensor([1.0000001, 0.0, inf, -inf, nan, 2.0]), want) == 1
    assert R.disagreements(torch.tensor([1.0000001, 0.0, inf, -inf, nan, 2.0]), want, exact=False) == 0
    assert R.disagreements(torch.tensor([3.0e38]), torch.tensor([1e39], dtype=torch.float64)) == 1     # (the cast to float32 overflows)


# ---- Part A -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(R.ROUNDING_CASES))
def test_rounding_case(case_id):
    case = R.rounding_case(case_id)
    finite_list = case_id.endswith("/finite")
    # 1. the other operands select: at most one product per output sum, and some
    counts = R.selected_counts(case)
    picked = 0
    for name, c in counts.items():
        if name in R.BY_CLASS_ONLY:
            continue
        assert bool(torch.isfinite(c).all()) and float(c.max()) <= 1.0 and float(c.min()) >= 0.0, (name, float(c.max()))
        picked += int((c == 1).sum())
    assert picked > 0
    # 2. the two restatements agree: classes everywhere, finite values bit for bit
    r64, r32 = R.rounding_expected(case_id), R.restate(case.entry, case.args, torch.float32)
    for name, want in r64.items():
        assert r32[name].dtype == torch.float32
        assert R.disagreements(r32[name], want, exact=name not in R.BY_CLASS_ONLY) == 0, name
    # 3. the finite list gives finite outputs that carry the patterns; the full one reaches NaN through the selector's zeros
    operand = R.get(case.args, case.operand)
    flat = torch.cat([v.reshape(-1) for k, v in r64.items() if k not in R.BY_CLASS_ONLY])
    if case.operand == "dlogits":
        operand = operand * case.args["scale"]
    if finite_list:
        assert bool(torch.isfinite(flat).all())
        values = operand.unique()
        values = values[values != 0]
        seen = set(flat.abs().unique().tolist())          # (rounded where the contract rounds the operand, as it is where it does not)
        carried = [float(v) for v in values if abs(float(v.to(torch.bfloat16))) in seen or abs(float(v)) in seen]
        assert len(carried) >= (len(values) + 1) // 2, (len(carried), len(values))
    elif case.support is None and not case.operand.endswith("bias"):      # (a bias meets no zero, and FLT_MAX stays what it is)
        assert not bool(torch.isfinite(flat).all())


# ---- Part B -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("site", list(R.POISON_SITES))
def test_poison_site_dependence_set(site):
    """In the restatement itself: nothing outside the dependence set moves, whatever the poison; NaN fills all of the set that a
    product or a sum carries it to; the loss of a poisoned row is NaN."""
    base = site.split("/")[0]
    clean = R.poison_clean_expected(base)
    for p in R.POISONS:
        entry, args, bad, operand, idx = R.poison_case(f"{site}/{p}")
        assert not torch.isfinite(R.get(bad, operand)[idx]) and bool(torch.isfinite(R.get(args, operand)).all())
        deps = R.depends(entry, args, operand, idx)
        want = R.poison_expected(f"{site}/{p}")
        assert set(deps) == set(want) == set(clean)
        hit = 0
        for name in want:
            assert deps[name].shape == want[name].shape, name
            outside = ~deps[name]
            assert bool(torch.isfinite(clean[name]).all()), name
            assert torch.equal(want[name][outside], clean[name][outside]), (p, name)
            inside = deps[name]
            hit += int((~torch.isfinite(want[name]))[inside].sum()) if p == "nan" else int((want[name][inside] != clean[name][inside]).sum())
        assert hit > 0, p                                    # the poison shows inside the set (-Inf may end as a finite 0 behind a ReLU)
        if p == "nan" and entry in ("critic_loss", "actor_loss"):
            assert bool(torch.isnan(want["loss"]))
    some_free = any(not bool(d.all()) for d in deps.values())
    everything = entry in ("actor", "critic") and operand != "x" and not (operand.startswith("fc3") and entry == "critic")
    assert some_free or everything, "the set leaves nothing to compare with the clean run"
