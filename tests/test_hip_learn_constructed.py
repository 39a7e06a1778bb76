"""K7 (ippm_coma_advantage) and K8 (ippm_td_lambda, ippm_td_lambda_buffer) on the constructed inputs of tests/learn_cases.py against the
oracle in float64, with bounds derived from the kernels' operation counts (tests/learn_cases.py: k7_reference, k8_check), not from what the
kernels give; the CPU half (tests/test_learn_constructed_cpu.py) shows the inputs reach what they were built for.  Also the two host-side
rules of csrc/learn.hip: an empty call returns 0 and launches nothing, chains * len beyond 2^31 - 1 is refused."""
import numpy as np
import pytest

import learn_cases as L
from configs import make_params

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _context(**over):
    from ippmarl import _ffi
    from ippmarl.derived import DerivedConstants
    return _ffi.Context(DerivedConstants(make_params("small", **over)))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.mark.parametrize("A", L.ACTION_SETS)
def test_k7_constructed_rows_against_the_oracle(A):
    from ippmarl import _ffi
    ctx = _context(experiment__constraints__num_actions=A)
    worst = worst_pn = 0.0
    for B in L.K7_BATCHES:
        probs, q, mask, action, _ = L.k7_batch(A, B)
        tp, tq, tm, ta = _dev(probs), _dev(q), _dev(mask), _dev(action)
        results = []
        for with_pn in (True, False):
            adv = torch.full((B + 8,), 7.0, dtype=torch.float32, device=DEV)          # (eight more rows: nothing may be written past the batch)
            pn = torch.full((B + 8, A), 7.0, dtype=torch.float32, device=DEV)
            ctx.call("ippm_coma_advantage", _ffi.ptr(tp), _ffi.ptr(tq), _ffi.ptr(tm), _ffi.ptr(ta), _ffi.ptr(adv), _ffi.ptr(pn) if with_pn else None,
                     B, _stream())
            torch.cuda.synchronize()
            adv, pn = adv.cpu().numpy(), pn.cpu().numpy()
            assert (adv[B:] == 7.0).all() and (pn[B:] == 7.0).all() and (with_pn or (pn == 7.0).all())
            ratio, rel = L.k7_check(adv[:B], pn[:B] if with_pn else None, probs, q, mask, action)
            worst, worst_pn = max(worst, ratio), max(worst_pn, rel)
            results.append(adv[:B])
        assert np.array_equal(results[0], results[1])      # the advantage does not depend on whether pi~ is asked for
    print(f"\nK7, {A} actions: largest |adv - ref| / bound {worst:.3f}, largest pi~ deviation {worst_pn:.2f} x 2^-24 (bound 4)")
    ctx.close()


@pytest.mark.parametrize("pattern", L.K8_PATTERNS)
@pytest.mark.parametrize("gamma,lam", L.K8_PARAMS)
def test_k8_chain_kernel_against_the_oracle(gamma, lam, pattern):
    from ippmarl import _ffi
    ctx = _context(networks__gamma=gamma, networks__lambda=lam)
    worst = 0.0
    for chains, length in L.K8_SHAPES:
        ref = L.k8_reference(chains, length, pattern, gamma, lam)
        reward, q_sel = L.k8_chains(chains, length)
        done = np.repeat(ref[4][None, :], chains, axis=0).astype(np.uint8)
        n = chains * length
        td = torch.full((n + 256,), 7.0, dtype=torch.float32, device=DEV)           # (room for one more workgroup: nothing may land there)
        dr = torch.full((n + 256,), 7.0, dtype=torch.float32, device=DEV)
        t_r, t_d, t_q = _dev(reward), _dev(done), _dev(q_sel)
        ctx.call("ippm_td_lambda", _ffi.ptr(t_r), _ffi.ptr(t_d), _ffi.ptr(t_q), _ffi.ptr(td), _ffi.ptr(dr), chains, length, _stream())
        torch.cuda.synchronize()
        td, dr = td.cpu().numpy(), dr.cpu().numpy()
        assert (td[n:] == 7.0).all() and (dr[n:] == 7.0).all()
        worst = max(worst, L.k8_check(td[:n].reshape(chains, length), dr[:n].reshape(chains, length), ref, lam))
    print(f"\nK8 chains, gamma {gamma} lambda {lam} dones {pattern}: largest error {worst:.3f} of ulp32(ref) + 1e-12 sum|terms|")
    ctx.close()


@pytest.mark.parametrize("gamma,lam", L.K8_PARAMS)
def test_k8_buffer_kernel_against_the_oracle(gamma, lam):
    """The same chains in the replay buffer's order [W, T, E, N] (a done at the end of every wave), rewards stored per agent [W, T, E, N] and
    per env [W, T, E]: the agents of an env share its rewards in both."""
    from ippmarl import _ffi
    ctx = _context(networks__gamma=gamma, networks__lambda=lam)
    worst = 0.0
    for (chains, length), forms in L.K8_BUFFER_SHAPES.items():
        for W, T, E, N in forms:
            ref = L.k8_reference(chains, length, ("waves", T), gamma, lam, shared=N)
            reward, q_sel = L.k8_chains(chains, length, shared=N)                   # [E * N, W * T], chain (e, n) = row e * N + n
            to_buf = lambda x: np.ascontiguousarray(x.reshape(E, N, W, T).transpose(2, 3, 0, 1))   # noqa: E731  -> [W, T, E, N]
            r_agent, q_buf = to_buf(reward), to_buf(q_sel)
            r_env = np.ascontiguousarray(r_agent[..., 0])
            assert (r_agent == r_env[..., None]).all()
            n = chains * length
            for per_agent, r_buf in ((1, r_agent), (0, r_env)):
                td = torch.full((n + 256,), 7.0, dtype=torch.float32, device=DEV)
                dr = torch.full((n + 256,), 7.0, dtype=torch.float32, device=DEV)
                t_r, t_q = _dev(r_buf), _dev(q_buf)
                ctx.call("ippm_td_lambda_buffer", _ffi.ptr(t_r), per_agent, _ffi.ptr(t_q), _ffi.ptr(td), _ffi.ptr(dr), W, T, E, N, _stream())
                torch.cuda.synchronize()
                td, dr = td.cpu().numpy(), dr.cpu().numpy()
                assert (td[n:] == 7.0).all() and (dr[n:] == 7.0).all()
                to_chain = lambda x: x[:n].reshape(W, T, E, N).transpose(2, 3, 0, 1).reshape(chains, length)   # noqa: E731
                worst = max(worst, L.k8_check(to_chain(td), to_chain(dr), ref, lam))
    print(f"\nK8 buffer order, gamma {gamma} lambda {lam}: largest error {worst:.3f} of ulp32(ref) + 1e-12 sum|terms|")
    ctx.close()


def test_empty_calls_return_zero_and_touch_nothing():
    """ippm_coma_advantage(batch <= 0) and ippm_td_lambda(chains <= 0 or len <= 0): rc 0, no launch (a grid of zero workgroups is a launch
    error), outputs untouched; chains * len > 2^31 - 1 is refused with a message."""
    from ippmarl import _ffi
    ctx = _context()
    lib = ctx.lib
    A = ctx.cfg.n_actions
    x = torch.ones(4 * A, dtype=torch.float32, device=DEV)
    m = torch.ones(4 * A, dtype=torch.uint8, device=DEV)
    a = torch.zeros(4, dtype=torch.int32, device=DEV)
    out = torch.full((4 * A,), 3.0, dtype=torch.float32, device=DEV)
    out2 = torch.full((4 * A,), 3.0, dtype=torch.float32, device=DEV)
    p = _ffi.ptr
    for batch in (0, -1, -(2 ** 31)):
        assert lib.ippm_coma_advantage(ctx.handle, p(x), p(x), p(m), p(a), p(out), p(out2), batch, _stream()) == 0, batch
    for chains, length in ((0, 5), (5, 0), (0, 0), (-3, 4), (4, -3), (-2, -2)):
        assert lib.ippm_td_lambda(ctx.handle, p(x), p(m), p(x), p(out), p(out2), chains, length, _stream()) == 0, (chains, length)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((out2 == 3.0).all())
    for chains, length in ((1 << 16, 1 << 15), (2 ** 31 - 1, 2), (3, 2 ** 30)):
        assert lib.ippm_td_lambda(ctx.handle, p(x), p(m), p(x), p(out), p(out2), chains, length, _stream()) == -1, (chains, length)
        assert "ippm_td_lambda" in lib.ippm_last_error().decode() and "2^31" in lib.ippm_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((out2 == 3.0).all())
    # null arguments are still refused before anything else
    assert lib.ippm_coma_advantage(ctx.handle, None, p(x), p(m), p(a), p(out), None, 0, _stream()) == -1
    assert lib.ippm_td_lambda(ctx.handle, p(x), p(m), p(x), None, p(out2), 0, 0, _stream()) == -1
    # ... and the calls still work
    assert lib.ippm_coma_advantage(ctx.handle, p(x), p(x), p(m), p(a), p(out), None, 4, _stream()) == 0
    assert lib.ippm_td_lambda(ctx.handle, p(x), p(m), p(x), p(out2), p(out), 2, 2, _stream()) == 0
    torch.cuda.synchronize()
    ctx.close()
