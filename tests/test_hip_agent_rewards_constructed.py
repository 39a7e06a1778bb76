"""k_agent_rewards on the device (csrc/agent_rewards.hip, ippm_agent_rewards) against the constructed scenes of
tests/agent_reward_scenes.py: the scene sets of test_hip_constructed_rects.py with one more check per step (A1), and value and
geometry sets through direct calls of the entry point (A2, A3).  The references, the bounds and what the sets reach are in
agent_reward_scenes.py and tests/test_agent_reward_scenes_cpu.py; measured figures in profiles/r22/README.md.

Bounds: (S1_i, S2_i) against float64 at rtol 1e-5 beside sums_atol (check_deepq_batch's and _check_env_step's bound for these sums;
the float32 restatement keeps half of it on every scene, CPU test); agent_reward against float32(rewards_of) of the device's own sums
to one float32 rounding, and against the reference at check_deepq_batch's reward tolerances where |S2| passes reward_cutoff."""
import functools

import numpy as np
import pytest

import agent_reward_scenes as A
from test_hip_constructed_rects import N, Runner, sums_atol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 16                 # elements before and behind each output
MARK_S, MARK_R = -7.25e77, -3.5e33


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def run_direct(ds, layout, T, code=None, teams=None, with_sums=True):
    """One call of ippm_agent_rewards on a bare context.  -> (agent_sums [E, N, 2] or None, agent_reward [E, N, 2], kernel name);
    asserts that the inputs are unchanged bit for bit and the guard bands around both outputs intact."""
    from ippmarl import _ffi
    from ippmarl.vec_env import tiles_view
    g, E, n = ds.g, ds.E, ds.N
    ctx = _ffi.Context(g.d)
    try:
        tiled = layout == "tiles"
        ctx.call("ippm_set_map_layout", 1 if tiled else 0)
        stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
        glob = tiles_view(torch.from_numpy(ds.K), tiled).contiguous().to(DEV)
        code_t, rec = _dev(ds.code if code is None else code), _dev(ds.records)
        sums_h = np.full((E, 8), 12345.678)                      # (only [e][2] is read)
        sums_h[:, 2] = T
        sums = _dev(sums_h)
        keep = [t.clone() for t in (glob, code_t, rec, sums)]
        out_s = torch.full((2 * GUARD + E * n * 2,), MARK_S, dtype=torch.float64, device=DEV)
        out_r = torch.full((2 * GUARD + E * n * 2,), MARK_R, dtype=torch.float32, device=DEV)
        view_s, view_r = out_s[GUARD:GUARD + E * n * 2], out_r[GUARD:GUARD + E * n * 2]
        n_active = None
        if teams is not None:
            n_active = _dev(np.asarray(teams, dtype=np.int32))
            ctx.call("ippm_set_team_sizes", _ffi.ptr(n_active))
        ctx.kernel_timing(True)
        ctx.call("ippm_agent_rewards", _ffi.ptr(glob), _ffi.ptr(code_t), _ffi.ptr(rec), _ffi.ptr(sums), _ffi.ptr(view_s) if with_sums else None,
                 _ffi.ptr(view_r), E, stream)
        torch.cuda.synchronize()
        kernel = ctx.kernel_times(stream)["agent_rewards"]["kernel"]
        for a, b in zip((glob, code_t, rec, sums), keep):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), ds.name
        for out, mark in ((out_s, MARK_S), (out_r, MARK_R)):
            assert bool((out[:GUARD] == mark).all()) and bool((out[-GUARD:] == mark).all()), ds.name
        if not with_sums:
            assert bool((view_s == MARK_S).all())
        return (view_s.cpu().numpy().reshape(E, n, 2) if with_sums else None), view_r.cpu().numpy().reshape(E, n, 2), kernel
    finally:
        ctx.close()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def check_against_reference(ds, got_s, got_r, T, tag, flying=None):
    """The comparisons of one call.  T [E]: what the caller put into sums[e][2].  -> the largest error / bound of S1 and of S2 - T."""
    g, ref = ds.g, ds.ref
    fly = np.ones((ds.E, ds.N), dtype=bool) if flying is None else flying
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), (ds.E,))
    bound = ds.bound(ref["S"])                                   # from the reference's own sums, whatever T the caller passes
    want = np.stack([ref["S"][..., 0], T[:, None] + ref["D"]], axis=-1)
    err = np.abs(got_s - want)
    slack = np.stack([np.zeros_like(T), np.abs(T) * 2.0 ** -51], axis=-1)[:, None, :]     # (the float64 rounding of T + d)
    assert np.isfinite(got_s).all(), (tag, np.argwhere(~np.isfinite(got_s))[:4].tolist())
    ratio = np.where(fly[..., None], err / (bound + slack), 0.0)
    print(tag, "largest error / bound: S1 %.4f, S2 - T %.4f" % (ratio[..., 0].max(), ratio[..., 1].max()))
    bad = np.argwhere(~(ratio <= 1.0))      # (a NaN among the sums is a miss too)
    assert bad.size == 0, (tag, bad[:4].tolist(), [(ds.tags[e][i], got_s[e, i].tolist(), want[e, i].tolist()) for e, i, _ in bad[:4]])
    # the final expression, on the device's own sums: one float32 rounding
    rel, ab = A.rewards_of(g, got_s[..., 0], got_s[..., 1])
    for k, w in enumerate((rel, ab)):
        w32 = w.astype(np.float32)
        with np.errstate(invalid="ignore"):
            ok = (got_r[..., k] == w32) | (np.isnan(got_r[..., k]) & np.isnan(w32)) | (np.abs(got_r[..., k] - w32) <= np.spacing(np.abs(w32)))
        assert ok[fly].all(), (tag, "reward of the device's sums", k, np.argwhere(~ok & fly)[:4].tolist())
    # ... and against the reference, where the sums' bound carries through 22 S1 / S2
    far = A.reward_cutoff(want) & fly
    rel, ab = A.rewards_of(g, want[..., 0], want[..., 1])
    tol_rel, tol_ab = A.reward_tol(rel, ab)
    with np.errstate(invalid="ignore"):
        near = (np.abs(got_r[..., 0] - rel) <= tol_rel) & (np.abs(got_r[..., 1] - ab) <= tol_ab)
    assert near[far].all(), (tag, "reward")
    # exact values: agents without a footprint (prior 0.5)
    if not g.shift:
        for e in range(ds.E):
            for i in range(ds.N):
                if fly[e, i] and not A.R._some(ds.rects[e, i]):
                    assert got_s[e, i, 0] == 0.0 and got_s[e, i, 1] == T[e], (tag, e, i, got_s[e, i].tolist())
                    if T[e] != 0:
                        assert got_r[e, i].tolist() == [np.float32(-0.5), np.float32(-0.17)], (tag, e, i, got_r[e, i].tolist())
    return ratio[..., 0].max(), ratio[..., 1].max()


@pytest.mark.parametrize("name,layout", A.DIRECT_SETS)
def test_direct_sets_match_the_reference(name, layout):
    """Every agent of every scene of a value or geometry set: the sums within the project's bound, the reward of the device's own
    sums to one rounding and the reference's reward beyond the cut-off; the kernel the set names ran.  Geometry sets run with
    sums[e][2] at the reference's own T, at 0 and at 1e6: S2_i - T follows the reference in all three."""
    ds = A.direct_set(name)
    modes = [("T own", ds.ref["T"])]
    if name.startswith("geometry_"):
        modes += [("T 0", np.zeros(ds.E)), ("T 1e6", np.full(ds.E, 1e6))]
    for mode, T in modes:
        got_s, got_r, kernel = run_direct(ds, layout, T)
        assert kernel == A.instantiation(ds.g, layout == "tiles"), kernel
        check_against_reference(ds, got_s, got_r, T, f"{name} {layout} {mode}")


PROPERTY_SETS = [("geometry_48", "rows"), ("geometry_48", "tiles"), ("geometry_46", "rows"), ("geometry_34", "rows"), ("geometry_48p", "rows"),
                 ("geometry_34p", "rows"), ("values128", "tiles"), ("values_nf", "rows")]


@pytest.mark.parametrize("name,layout", PROPERTY_SETS)
def test_direct_call_properties(name, layout):
    """Two runs are bit-identical; agent_sums = NULL gives the same reward bits; code tiles whose bytes and bits outside the footprint's
    cells are 0xFF or random give the same bits as zero-filled ones; the same scene first, in the middle and last in the batch gives
    the same bits; agents switched off by ippm_set_team_sizes get exact zeros and change nobody else's result.  (Inputs unchanged and
    guard bands intact: asserted by every run.)"""
    ds = A.direct_set(name)
    T = ds.ref["T"]
    s0, r0, _ = run_direct(ds, layout, T)
    s1, r1, _ = run_direct(ds, layout, T)
    assert np.array_equal(_bits(s0), _bits(s1)) and np.array_equal(_bits(r0), _bits(r1)), "two runs differ"
    _, r2, _ = run_direct(ds, layout, T, with_sums=False)
    assert np.array_equal(_bits(r0), _bits(r2)), "agent_sums = NULL changes the reward"
    for fill in (0xFF, 20261):
        stale = ds.stale_code(fill)
        assert not np.array_equal(stale, ds.code)
        s3, r3, _ = run_direct(ds, layout, T, code=stale)
        assert np.array_equal(_bits(s0), _bits(s3)) and np.array_equal(_bits(r0), _bits(r3)), ("stale code tile", fill)
    if hasattr(ds, "copies"):
        for k in ds.copies[1:]:
            assert np.array_equal(_bits(s0[0]), _bits(s0[k])) and np.array_equal(_bits(r0[0]), _bits(r0[k])), ("placement in the batch", k)
    teams = A.team_sizes(ds)
    fly = np.arange(ds.N)[None, :] < teams[:, None]
    assert (~fly).any() and fly.all(axis=1).any()
    s4, r4, _ = run_direct(ds, layout, T, teams=teams)
    assert not s4[~fly].any() and not r4[~fly].any() and not np.signbit(s4[~fly]).any() and not np.signbit(r4[~fly]).any()
    assert np.array_equal(_bits(s4[fly]), _bits(s0[fly])) and np.array_equal(_bits(r4[fly]), _bits(r0[fly])), "team sizes change a flying agent's result"


def test_all_free_map_with_T_zero_gives_the_oracles_zero_over_zero():
    """Every class weight 0 before and after, T = 0: S1 = S2 = 0 exactly and, as utils/reward.py's NumPy division has it, a relative
    reward of 0 / 0 = nan beside the absolute reward -0.17: the device gives what the oracle's arithmetic gives."""
    ds = A.free_set()
    assert ds.ref["T"][0] == 0.0 and not ds.ref["S"].any()
    rel, ab = A.rewards_of(ds.g, ds.ref["S"][..., 0], ds.ref["S"][..., 1])
    assert np.isnan(rel).all() and (ab == -0.17).all()
    for layout in ("rows", "tiles"):
        got_s, got_r, _ = run_direct(ds, layout, np.zeros(1))
        assert not got_s.any(), got_s
        assert np.isnan(got_r[..., 0]).all() and (got_r[..., 1] == np.float32(-0.17)).all(), got_r


# ---- A1 -------------------------------------------------------------------------------------------------------------------------
class RewardRunner(Runner):
    """test_hip_constructed_rects.Runner whose VecEnv is built with agent_rewards=True.  Runner takes no such argument, so the class it
    builds is exchanged for the time of its constructor.  Two things this depends on: Runner.__init__ imports VecEnv from
    ippmarl.vec_env INSIDE the method (a module-level import there would bind the plain class before the exchange; the assertion below
    would then fail), and A.geom(grid) runs before Runner asks test_hip_constructed_rects.geom for a grid of A.AR_GRIDS (see A.geom)."""

    def __init__(self, grid, layout):
        import ippmarl.vec_env as V
        A.geom(grid)
        plain = V.VecEnv
        V.VecEnv = functools.partial(plain, agent_rewards=True)
        try:
            super().__init__(grid, layout, False)
        finally:
            V.VecEnv = plain
        assert self.env.agent_rewards and self.env.agent_reward is not None


@pytest.mark.parametrize("grid,layout", A.A1_FORMS)
def test_scene_sets_agent_rewards_match_the_reference(grid, layout):
    """The scene sets of test_hip_constructed_rects.py, every step: after the step's K3, ippm_agent_rewards over the sense records of
    the new footprints; agent_sums and agent_reward of all 8 agents of every scene against the reference computed from Sim's global map
    after the fusion of the step and the bits Sim.sense returns -- and the instantiation the grid names ran."""
    g = A.geom(grid)
    run = RewardRunner(grid, layout)
    env = run.env
    ref = A.a1_reference(grid)
    worst = np.zeros(2)
    for t in range(g.steps):
        run.fuse(t)
        run.sense(t)
        env.profile = True
        env._agent_rewards(env.rect_next)
        kernel = env.event_times_us()["agent_rewards"]["kernel"]
        env.profile = False
        assert kernel == A.instantiation(g, layout == "tiles"), kernel
        S, _ = ref[t]
        got_s, got_r = env.agent_sums.cpu().numpy(), env.agent_reward.cpu().numpy()
        atol = np.vectorize(lambda s2: sums_atol(g, s2))(S[..., 1])
        bound = A.RTOL * np.abs(S) + atol[..., None]
        ratio = np.abs(got_s - S) / bound
        worst = np.maximum(worst, ratio.max(axis=(0, 1)))
        bad = np.argwhere(~(ratio <= 1.0))      # (a NaN among the sums is a miss too)
        assert bad.size == 0, (grid, layout, t, [(run.scenes[e]["name"], i, got_s[e, i].tolist(), S[e, i].tolist()) for e, i, _ in bad[:4]])
        rel, ab = A.rewards_of(g, got_s[..., 0], got_s[..., 1])
        for k, w in enumerate((rel, ab)):
            w32 = w.astype(np.float32)
            assert (np.abs(got_r[..., k] - w32) <= np.spacing(np.abs(w32))).all(), (grid, layout, t, "reward of the device's sums", k)
        far = A.reward_cutoff(S)
        rel, ab = A.rewards_of(g, S[..., 0], S[..., 1])
        tol_rel, tol_ab = A.reward_tol(rel, ab)
        assert (np.abs(got_r[..., 0] - rel) <= tol_rel)[far].all() and (np.abs(got_r[..., 1] - ab) <= tol_ab)[far].all(), (grid, layout, t)
        assert got_s.shape == (run.E, N, 2)
    print(grid, layout, "largest error / bound: S1 %.4f, S2 %.4f" % tuple(worst))
    assert env.counters()["work_list_rejects"] == 0 and int(env.fault.abs().sum()) == 0
