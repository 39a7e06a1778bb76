"""Constructed inputs for K7 (k_coma_advantage; row code ippm_coma_baseline, csrc/ippm_internal.h) and K8 (ippm_td_lambda_at, run by
k_td_lambda and the replay buffer's k_td_lambda_buffer), with float64 / float32 restatements of the device arithmetic that the CPU half
(tests/test_learn_constructed_cpu.py) holds against the oracle.  Plain module; the device half is tests/test_hip_learn_constructed.py."""
import functools

import numpy as np

import ipp_oracle as O

ACTION_SETS = (4, 6, 9, 27)
K7_BATCHES = (1, 7, 8, 9, 263)      # 8 rows per workgroup: a single row, a ragged last workgroup, an empty half-wave
C32 = np.float32(1e-5)              # the device's floor, 1e-5f: the float32 NEXT BELOW the float64 1e-5 of the oracle
ULP = 2.0 ** -24
K7_KINDS = ("random", "all_masked", "one_valid", "chosen_masked", "zero_on_valid", "s_below", "s_at", "s_above", "pn_below", "pn_at", "pn_above",
            "big_q")


def _near(which):
    return {"below": np.nextafter(C32, np.float32(0)), "at": C32, "above": np.nextafter(C32, np.float32(1))}[which]


@functools.lru_cache(maxsize=None)
def k7_batch(A: int, B: int):
    """(probs, q, mask, action, kinds) of a constructed batch: float32 [B, A] x 2, uint8 [B, A], int32 [B], and each row's kind."""
    rng = np.random.RandomState(7000 + 31 * A + B)
    probs = rng.dirichlet(np.ones(A), size=B).astype(np.float32)
    q = rng.standard_normal((B, A)).astype(np.float32)
    mask = (rng.random_sample((B, A)) > 0.3).astype(np.uint8)
    action = rng.randint(0, A, size=B).astype(np.int32)
    mask[np.arange(B), action] = 1
    kinds = []
    for r in range(B):
        kind = K7_KINDS[(r + B) % len(K7_KINDS)]
        kinds.append(kind)
        k = int(rng.randint(0, A))
        if kind == "all_masked":
            mask[r] = 0
        elif kind == "one_valid":
            mask[r] = 0
            mask[r, k] = 1
        elif kind == "chosen_masked":
            mask[r, action[r]] = 0
            mask[r, (action[r] + 1) % A] = 1
        elif kind == "zero_on_valid":
            probs[r] = probs[r] * (1 - mask[r])
        elif kind.startswith("s_"):
            # sum(pi * m) = the float32 just below / at / just above 1e-5f: ONE valid action, so the sum is that number in any precision
            mask[r] = 0
            mask[r, k] = 1
            probs[r, k] = _near(kind[2:])
        elif kind.startswith("pn_"):
            # pi~(0) = the float32 just below / at / just above 1e-5f: sum(pi * m) = 2^-16 exactly (three terms whose float32 tree sum is exact
            # at every level), so the division is exact in any precision
            target = float(_near(kind[3:]))
            x = target * 2.0 ** -16
            rest = 2.0 ** -16 - x                                        # (40 significant bits: exact in float64)
            y1 = np.float32(rest)
            if float(y1) > rest:
                y1 = np.nextafter(y1, np.float32(0))
            y2 = rest - float(y1)
            assert float(np.float32(x)) == x and float(np.float32(y2)) == y2 and y2 >= 0 and float(y1) + y2 == rest
            probs[r] = 0
            probs[r, :3] = (x, float(y1), y2)
            mask[r] = 1
        elif kind == "big_q":
            # large Q of mixed sign: the baseline is what is left after the terms cancel
            q[r] = (rng.choice([-1.0, 1.0], size=A) * (1e6 + 1e3 * rng.random_sample(A))).astype(np.float32)
    return probs, q, mask, action, tuple(kinds)


def k7_reference(probs, q, mask, action):
    """(advantage, pi~, bound on |adv - ref|, floored) from O.coma_advantage in float64 on the float32 inputs.  The bound follows the kernel's
    operation count -- five tree levels, one division, two products, one subtraction, each at most 2^-24 relative:
    16 * 2^-24 * (|Q(chosen)| + sum |pi~ Q m|)."""
    p64, q64, m64 = probs.astype(np.float64), q.astype(np.float64), mask.astype(np.float64)
    adv, _, pn = O.coma_advantage(p64, q64, m64, action)
    q_chosen = q64[np.arange(len(action)), action]
    bound = 16 * ULP * (np.abs(q_chosen) + np.abs(pn * q64 * m64).sum(-1))
    raw = p64 * m64 / np.maximum((p64 * m64).sum(-1, keepdims=True), 1e-5)
    return adv, pn, bound, raw <= 1e-5


def k7_check(adv, pn, probs, q, mask, action):
    """Asserts the device's (or the float32 restatement's) outputs against the reference; returns the largest |adv - ref| / bound and the largest
    relative deviation of pi~ in units of 2^-24.  ``pn`` may be None (pi_tilde = NULL)."""
    adv_ref, pn_ref, bound, floored = k7_reference(probs, q, mask, action)
    err = np.abs(adv.astype(np.float64) - adv_ref)
    assert np.isfinite(adv).all()
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))))
    assert ratio <= 1.0, (ratio, int(np.argmax(err - bound)))
    rel = 0.0
    if pn is not None:
        assert (pn[floored] == C32).all(), "a floored pi~ must be exactly 1e-5f"
        dev = np.abs(pn.astype(np.float64) - pn_ref)[~floored] / pn_ref[~floored]
        rel = float(dev.max() / ULP) if dev.size else 0.0
        assert rel <= 4.0, rel
    return ratio, rel


def _tree32(v):
    """The 32-lane xor butterfly of ippm_coma_baseline in float32 (every lane ends with the same sum)."""
    w = np.zeros((len(v), 32), dtype=np.float32)
    w[:, :v.shape[1]] = v
    lanes = np.arange(32)
    for o in (16, 8, 4, 2, 1):
        w = (w + w[:, lanes ^ o]).astype(np.float32)
    assert (w == w[:, :1]).all()
    return w[:, 0]


def k7_float32(probs, q, mask, action, strict_floor=False):
    """ippm_coma_baseline + k_coma_advantage restated in NumPy float32, operation for operation.  ``strict_floor``: ``<`` for ``<=`` at the pi~
    floor (the one-line change the tests are asked to notice).  Returns (adv, pi~, s before its floor, pi~ before its floor)."""
    m = mask.astype(np.float32)
    p = (probs * m).astype(np.float32)
    s_raw = _tree32(p)
    s = np.where(s_raw < C32, C32, s_raw).astype(np.float32)
    pn_raw = (p / s[:, None]).astype(np.float32)
    pn = np.where((pn_raw < C32) if strict_floor else (pn_raw <= C32), C32, pn_raw).astype(np.float32)
    b = _tree32(((pn * q).astype(np.float32) * m).astype(np.float32))
    adv = (q[np.arange(len(action)), action] - b).astype(np.float32)
    return adv, pn, s_raw, pn_raw


# ---------------------------------------------------------------------------------------------------------------------------------
# K8
# ---------------------------------------------------------------------------------------------------------------------------------
K8_SHAPES = ((1, 1), (1, 2), (3, 15), (5, 51), (1, 256), (257, 1), (4, 75))     # chains x len: 255, 256 and 257 threads among them
K8_PATTERNS = ("none", "all", "first", "last", "last_two", "middle_two", "every_15th")
K8_PARAMS = ((0.99, 0.8), (1.0, 1.0), (0.99, 0.0), (0.5, 1.0), (0.0, 0.8))       # (gamma, lambda)
# the same chains in the replay buffer's order [W, T, E, N]: chains = E * N, len = W * T, a done at the end of every wave
K8_BUFFER_SHAPES = {(1, 1): ((1, 1, 1, 1),), (1, 2): ((2, 1, 1, 1), (1, 2, 1, 1)), (3, 15): ((1, 15, 3, 1),), (5, 51): ((3, 17, 1, 5),),
                    (1, 256): ((16, 16, 1, 1),), (257, 1): ((1, 1, 257, 1),), (4, 75): ((5, 15, 2, 2),)}


def k8_dones(pattern: str, L: int) -> np.ndarray:
    d = np.zeros(L, dtype=bool)
    if pattern == "all":
        d[:] = True
    elif pattern == "first":
        d[0] = True
    elif pattern == "last":
        d[-1] = True
    elif pattern == "last_two":
        d[-2:] = True
    elif pattern == "middle_two":
        d[L // 2:L // 2 + 2] = True
    elif pattern == "every_15th":
        d[14::15] = True
    else:
        assert pattern == "none"
    return d


@functools.lru_cache(maxsize=None)
def k8_chains(chains: int, L: int, shared: int = 1):
    """(reward, q_sel) float32 [chains, L]; ``shared``: that many consecutive chains share their rewards (the agents of an env)."""
    rng = np.random.RandomState(8000 + 1000 * chains + L)
    reward = np.repeat(rng.standard_normal((chains // shared, L)), shared, axis=0).astype(np.float32)
    q_sel = (3.0 * rng.standard_normal((chains, L))).astype(np.float32)
    return reward, q_sel


def k8_kernel_f64(r, done, qs, gamma, lam, guard=True):
    """ippm_td_lambda_at for one chain in Python floats, statement for statement: (td, discounted return, sum |terms| of td, of the return) per
    element, before the device's one rounding to float32.  ``guard=False`` drops the ``t + l == 0`` test: ``done(-1)`` is then whatever lies
    in front of the chain -- the previous chain's last flag, which is what Python's index -1 stands in for here."""
    L = len(r)
    td, dr, td_abs, dr_abs = np.zeros(L), np.zeros(L), np.zeros(L), np.zeros(L)
    for t in range(L):
        total = g = disc = 0.0
        total_abs = g_abs = 0.0
        gpow = lpow = 1.0
        for n in range(1, L - t + 1):
            l = n - 1  # noqa: E741
            ok = (guard and t + l == 0) or not done[t + l - 1]
            if not ok:
                total += lpow * lam * g
                total_abs += lpow * lam * g_abs
                disc = g
                break
            g += gpow * float(r[t + l])
            g_abs += gpow * abs(float(r[t + l]))
            disc = g
            gn, gn_abs = g, g_abs
            if t + n < L and not (done[t + n] or t + n + 1 >= L):
                gn += gpow * gamma * float(qs[t + n])
                gn_abs += gpow * gamma * abs(float(qs[t + n]))
            total += lpow * gn
            total_abs += lpow * gn_abs
            gpow *= gamma
            lpow *= lam
        td[t], dr[t] = (1.0 - lam) * total, disc
        td_abs[t], dr_abs[t] = abs(1.0 - lam) * total_abs, g_abs
    return td, dr, td_abs, dr_abs


@functools.lru_cache(maxsize=None)
def k8_reference(chains: int, L: int, dones_key, gamma: float, lam: float, shared: int = 1):
    """O.td_lambda_targets on every chain (float64 on the float32 inputs), and the sums of |terms| for the tolerance.  ``dones_key``: a pattern
    name, or ("waves", T) for the replay buffer's done at the end of every wave of T steps."""
    reward, q_sel = k8_chains(chains, L, shared)
    done = k8_dones(dones_key, L) if isinstance(dones_key, str) else (np.arange(L) % dones_key[1] == dones_key[1] - 1)
    td, dr, td_abs, dr_abs = (np.zeros((chains, L)) for _ in range(4))
    for c in range(chains):
        td[c], dr[c] = O.td_lambda_targets(reward[c].astype(np.float64), list(done), q_sel[c].astype(np.float64), gamma, lam)
        _, _, td_abs[c], dr_abs[c] = k8_kernel_f64(reward[c], done, q_sel[c], gamma, lam)
    return td, dr, td_abs, dr_abs, done


def ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def k8_check(got_td, got_dr, ref, lam):
    """The kernel works in double and rounds once: |got - ref| <= ulp32(ref) + 1e-12 * sum |terms|; lambda = 1: td == 0 exactly.  Returns the
    largest error in units of that tolerance."""
    td, dr, td_abs, dr_abs, _ = ref
    worst = 0.0
    for got, want, terms in ((got_td, td, td_abs), (got_dr, dr, dr_abs)):
        tol = ulp32(want) + 1e-12 * terms
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= tol).all(), (float(err.max()), int(np.argmax(err - tol)))
        worst = max(worst, float((err / tol).max()))
    if lam == 1.0:
        assert (got_td == 0).all()
    return worst
