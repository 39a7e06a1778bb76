"""The comm matrix on the device (comm_pair in csrc/step_small.hip) against the constructed cases of tests/comm_scenes.py, bit for bit on
the [E, N, N] bytes, in every form the code runs in:

  matrix    ippm_comm_matrix (k_comm: a lane per row) on a bare context -- every case, cfg.comm_range (NULL range array) included;
  inline    ippm_comm_fuse_local (k_plan_step with IPPM_STEP_COMM: lanes = ordered pairs, a sweep per 64 pairs) on a bare context --
            every case;
  batched   VecEnv.build_observations(t, features=False) in row and in tile storage, and the env-only step that also moves
            (VecEnv.steps(..., features=False): comm reads the pre-move positions) -- every case but the 19 whose cfg.comm_range
            is a double that no float32 equals (the float64 neighbours of a distance, sqrt(d2) of a non-square): VecEnv always hands the
            kernel its per-env float32 range array, which cannot say such a range.  32 cases (BATCHED); the moving step runs the 30
            of them without team sizes (a team of 0 has nothing to move or sense).
Beyond the matrix: what a plan receives follows the row -- the sources of the type-1 ops of local map i in `ws` are the set bits of
row i other than i, ascending, without agents whose published rectangle is empty."""
import numpy as np
import pytest

import comm_scenes as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FAMILIES = ["range", "draws", "philox", "team"]
BATCHED = {"range": 10, "draws": 2, "philox": 10, "team": 10}      # cases per family in the batched forms ...
MOVING = {"range": 10, "draws": 2, "philox": 10, "team": 8}        # ... and in the step that also moves


def _dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def _context(c):
    from ippmarl import _ffi
    from ippmarl.derived import DerivedConstants
    return _ffi.Context(DerivedConstants(c.params, philox_seed=C.SEED))


def _sources(ws, E, n):
    """[E][n] lists: the sources of the type-1 ops of every local map's plan (ws words: 8 = number of ops, 16 + 8 k = type, 17 + 8 k = source)."""
    ws = ws.cpu().numpy()
    return [[[int(ws[e, i, 17 + 8 * k]) for k in range(int(ws[e, i, 8])) if ws[e, i, 16 + 8 * k] == 1] for i in range(n)] for e in range(E)]


def run_matrix(c, teams=False):
    from ippmarl import _ffi
    ctx = _context(c)
    try:
        stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
        episode, pos, rng, draws = _dev(c.episode), _dev(c.pos), _dev(c.range32), _dev(c.draws)
        comm = torch.full((c.E, c.n, c.n), 0xA5, dtype=torch.uint8, device=DEV)
        n_active = _dev(c.n_active) if teams else None
        if teams:
            ctx.call("ippm_set_team_sizes", _ffi.ptr(n_active))
        ctx.call("ippm_comm_matrix", _ffi.ptr(episode), _ffi.ptr(pos), _ffi.ptr(rng), _ffi.ptr(draws), _ffi.ptr(comm), c.t, c.E, stream)
        torch.cuda.synchronize()
        assert np.array_equal(pos.cpu().numpy(), c.pos)
        return comm.cpu().numpy()
    finally:
        ctx.close()


def run_inline(c):
    from ippmarl import _ffi
    ctx = _context(c)
    try:
        d = ctx.derived
        stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
        episode, pos, rng, draws = _dev(c.episode), _dev(c.pos), _dev(c.range32), _dev(c.draws)
        rect = C.published(c)
        comm = torch.full((c.E, c.n, c.n), 0xA5, dtype=torch.uint8, device=DEV)
        local = torch.zeros(c.E, c.n, d.grid_x, d.grid_y, dtype=torch.float32, device=DEV)
        code = torch.zeros(c.E, c.n, d.tile_bytes, dtype=torch.uint8, device=DEV)
        ws = torch.zeros(c.E, c.n + 1, _ffi.WS_WORDS, dtype=torch.int32, device=DEV)
        rect_t = _dev(rect)
        ctx.call("ippm_comm_fuse_local", _ffi.ptr(episode), _ffi.ptr(pos), _ffi.ptr(rng), _ffi.ptr(draws), _ffi.ptr(comm), _ffi.ptr(local),
                 _ffi.ptr(code), _ffi.ptr(rect_t), _ffi.ptr(ws), c.t, c.E, stream)
        torch.cuda.synchronize()
        return comm.cpu().numpy(), _sources(ws, c.E, c.n), rect
    finally:
        ctx.close()


def run_batched(c, layout, move):
    from ippmarl.vec_env import POLICY_UNIFORM, VecEnv
    teams = None if c.n_active is None else np.maximum(c.n_active, 1)      # (the constructor wants flying teams; the array is read at every launch)
    env = VecEnv(c.params, c.E, philox_seed=C.SEED, track_area=False, map_layout=layout, team_sizes=teams)
    assert env.tiled == (layout == "tiles")
    env.reset(np.arange(1, c.E + 1), start_positions=torch.from_numpy(c.pos))
    env.episode.copy_(torch.from_numpy(c.episode))        # (ids beyond what the start-state generator admits: comm only keys Philox with them)
    if c.range32 is not None:
        env.comm_range.copy_(torch.from_numpy(c.range32))
    else:
        assert (env.comm_range.cpu().numpy() == np.float32(c.comm_range)).all()
    if c.n_active is not None:
        env.n_active.copy_(torch.from_numpy(c.n_active))
    rect = C.published(c)
    draws = _dev(c.draws)
    if move:
        env.steps(c.t, policy=POLICY_UNIFORM, features=False, comm_draws=draws)
        torch.cuda.synchronize()
        return env.comm.cpu().numpy(), None, None
    env.rect.copy_(torch.from_numpy(rect))
    env.build_observations(c.t, comm_draws=draws, features=False)
    torch.cuda.synchronize()
    assert env.counters()["work_list_rejects"] == 0
    assert np.array_equal(env.pos.cpu().numpy(), c.pos)
    return env.comm.cpu().numpy(), _sources(env.ws, c.E, c.n), rect


def _family(fam):
    return [c for c in C.cases() if c.name.startswith(fam + "/")]


def _same(got, want, tag):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (tag, len(bad), bad[:6].tolist())


@pytest.mark.parametrize("fam", FAMILIES)
def test_comm_matrix_matches_the_oracle(fam):
    """ippm_comm_matrix on every case; it ignores team sizes by contract: with ippm_set_team_sizes set it still gives the whole team's matrix."""
    for c in _family(fam):
        _same(run_matrix(c), c.expected_whole_team, (c.name, "matrix"))
        if c.n_active is not None:
            _same(run_matrix(c, teams=True), c.expected_whole_team, (c.name, "matrix with team sizes set"))


@pytest.mark.parametrize("fam", FAMILIES)
def test_inline_comm_matches_the_oracle_and_the_plans_follow_the_rows(fam):
    for c in _family(fam):
        comm, sources, rect = run_inline(c)
        _same(comm, c.expected_whole_team, (c.name, "inline"))
        whole = C.Case(c.name, c.n, c.comm_range, c.failure_rate, c.pos, c.t, c.episode, c.range32, c.draws)
        assert sources == C.plan_sources(whole, comm, rect), (c.name, "plan sources")


@pytest.mark.parametrize("layout", ["rows", "tiles"])
@pytest.mark.parametrize("fam", FAMILIES)
def test_batched_comm_matches_the_oracle_and_the_plans_follow_the_rows(fam, layout):
    """VecEnv.build_observations: rows and columns of agents that do not fly are zero, even of one co-located with a flying agent."""
    ran = 0
    for c in _family(fam):
        if not c.batched:
            continue
        comm, sources, rect = run_batched(c, layout, move=False)
        _same(comm, c.expected, (c.name, layout, "build_observations"))
        assert sources == C.plan_sources(c, comm, rect), (c.name, layout, "plan sources")
        ran += 1
    assert ran == BATCHED[fam]


@pytest.mark.parametrize("fam", FAMILIES)
def test_env_only_step_comm_reads_the_positions_before_the_move(fam):
    ran = 0
    for c in _family(fam):
        if not c.batched or c.n_active is not None:
            continue
        comm, _, _ = run_batched(c, "rows", move=True)
        _same(comm, c.expected, (c.name, "steps"))
        ran += 1
    assert ran == MOVING[fam]
