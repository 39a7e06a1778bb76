"""CPU half of tests/test_hip_learn_constructed.py: the constructed K7 / K8 inputs of tests/learn_cases.py do what they were built for, the
bounds the device is held to are met by restatements of the device arithmetic (so a miss on the GPU is the kernel's), and the one-line
changes the issue names are noticed -- or are shown to change no value at all."""
import numpy as np
import pytest

import ipp_oracle as O
import learn_cases as L


@pytest.mark.parametrize("A", L.ACTION_SETS)
def test_k7_constructed_rows_take_the_same_branch_in_both_precisions(A):
    """The float32 restatement of the kernel and the float64 oracle floor the same sums and the same pi~ on every constructed row -- with the
    one exception float32 forces: sum == 1e-5f itself, which is below the oracle's 1e-5 (floored there, not on the device) and where both
    branches give the same number to 2^-25."""
    worst = worst_pn = 0.0
    seen = set()
    for B in L.K7_BATCHES:
        probs, q, mask, action, kinds = L.k7_batch(A, B)
        seen |= set(kinds)
        adv, pn, s_raw, pn_raw = L.k7_float32(probs, q, mask, action)
        p64 = probs.astype(np.float64) * mask
        s64 = p64.sum(-1)
        at = s_raw == L.C32
        assert ((s_raw < L.C32) == (s64 < 1e-5))[~at].all()
        assert [k for k, a in zip(kinds, at) if a] == ["s_at"] * int(at.sum()) and abs(float(L.C32) - 1e-5) <= 2.0 ** -25 * 1e-5
        pn64 = p64 / np.where(s64 < 1e-5, 1e-5, s64)[:, None]
        assert ((pn_raw <= L.C32) == (pn64 <= 1e-5)).all()
        for r, kind in enumerate(kinds):
            if kind.startswith("s_"):       # one term: the sum is that term in float32 and in float64
                assert s_raw[r] == L._near(kind[2:]) and s64[r] == float(s_raw[r])
            if kind.startswith("pn_"):      # sum = 2^-16 and pi~(0) = the intended neighbour of 1e-5f, exactly, in both precisions
                assert s_raw[r] == np.float32(2.0 ** -16) and s64[r] == 2.0 ** -16
                assert pn_raw[r, 0] == L._near(kind[3:]) and pn64[r, 0] == float(pn_raw[r, 0])
                assert (pn[r, 0] == L.C32) == (kind != "pn_above")
            if kind == "all_masked":
                assert not mask[r].any() and (pn[r] == L.C32).all() and adv[r] == q[r, action[r]]
            if kind == "chosen_masked":
                assert mask[r, action[r]] == 0 and mask[r].any()
            if kind == "zero_on_valid":
                assert mask[r].any() and not (probs[r] * mask[r]).any()
        ratio, rel = L.k7_check(adv, pn, probs, q, mask, action)
        worst, worst_pn = max(worst, ratio), max(worst_pn, rel)
        # `<` for `<=` at the pi~ floor changes no value: at pn == 1e-5f both branches yield 1e-5f.  No test can notice that change.
        strict = L.k7_float32(probs, q, mask, action, strict_floor=True)
        assert np.array_equal(strict[0], adv) and np.array_equal(strict[1], pn)
    assert seen == set(L.K7_KINDS)
    print(f"\nK7 float32 restatement, {A} actions: largest |adv - ref| / bound {worst:.3f}, largest pi~ deviation {worst_pn:.2f} x 2^-24")


def test_k7_bound_notices_a_wrong_floor_and_a_wrong_tree():
    """What the bound is worth: a floor of 2e-5, or a row sum that leaves out one lane, is far outside it."""
    A = 6
    probs, q, mask, action, _ = L.k7_batch(A, 263)
    adv, pn, _, _ = L.k7_float32(probs, q, mask, action)
    wrong = pn.copy()
    wrong[pn == L.C32] = np.float32(2e-5)
    with pytest.raises(AssertionError):
        L.k7_check(adv, wrong, probs, q, mask, action)
    m = mask.astype(np.float32)
    short = (q[np.arange(263), action] - ((pn * q * m)[:, :A - 1]).sum(-1)).astype(np.float32)
    with pytest.raises(AssertionError):
        L.k7_check(short, pn, probs, q, mask, action)


def _k8_cases():
    for shape in L.K8_SHAPES:
        for pattern in L.K8_PATTERNS:
            if shape == (1, 256) and pattern not in ("all", "every_15th"):
                continue     # (the oracle takes 1.5 s per such chain: the device half runs them all)
            yield shape, pattern


@pytest.mark.parametrize("gamma,lam", L.K8_PARAMS)
def test_k8_restatement_meets_the_tolerance_and_the_guard_matters(gamma, lam):
    """ippm_td_lambda_at restated in Python floats and rounded once to float32 is within ulp32(ref) + 1e-12 sum|terms| of O.td_lambda_targets
    on the constructed chains; without the ``t + l == 0`` guard it is not."""
    worst, caught = 0.0, 0
    for (chains, length), pattern in _k8_cases():
        ref = L.k8_reference(chains, length, pattern, gamma, lam)
        reward, q_sel = L.k8_chains(chains, length)
        done = ref[4]
        got = [L.k8_kernel_f64(reward[c], done, q_sel[c], gamma, lam) for c in range(chains)]
        td = np.array([g[0] for g in got]).astype(np.float32)
        dr = np.array([g[1] for g in got]).astype(np.float32)
        worst = max(worst, L.k8_check(td, dr, ref, lam))
        bad = [L.k8_kernel_f64(reward[c], done, q_sel[c], gamma, lam, guard=False) for c in range(chains)]
        try:
            L.k8_check(np.array([g[0] for g in bad]).astype(np.float32), np.array([g[1] for g in bad]).astype(np.float32), ref, lam)
        except AssertionError:
            caught += 1
    print(f"\nK8 restatement, gamma {gamma} lambda {lam}: largest error {worst:.3f} of the tolerance; cases that notice the dropped guard: {caught}")
    assert caught >= 1


def test_k8_patterns_reach_the_leave_branch_everywhere():
    """The done patterns put the "leave" branch at element 1 (done at 0), at the chain's end, on consecutive elements and in the middle, for
    lengths 1 and 2 too; the buffer shapes are factorisations of the same (chains, len)."""
    for chains, length in L.K8_SHAPES:
        for W, T, E, N in L.K8_BUFFER_SHAPES[(chains, length)]:
            assert (E * N, W * T) == (chains, length)
    assert sorted(c * n for c, n in L.K8_SHAPES)[2:6] == [45, 255, 256, 257]
    assert L.k8_dones("first", 1).tolist() == [True] and L.k8_dones("last_two", 2).tolist() == [True, True]
    assert L.k8_dones("middle_two", 15).nonzero()[0].tolist() == [7, 8] and L.k8_dones("every_15th", 75).sum() == 5
    # a done in front of element t makes t's accumulation leave at once: its discounted return is 0 whatever the rewards are
    r, qs = L.k8_chains(3, 15)
    td, dr = O.td_lambda_targets(r[0].astype(np.float64), list(L.k8_dones("middle_two", 15)), qs[0].astype(np.float64), 0.99, 0.8)
    assert dr[8] == 0.0 and dr[9] == 0.0 and dr[7] != 0.0 and td[8] == 0.0
