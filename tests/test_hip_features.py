"""GPU tests of the network-input kernels (csrc/features.hip, K6: ippm_actor_features, ippm_critic_features, ippm_area_sums,
ippm_area_resize, ippm_entropy_maps) on inputs BUILT to reach every path, against the oracle's literal restatement of the reference
(O.actor_observation / O.critic_state) and float64 NumPy.

Nothing under test feeds the expected side: the measurements and footprint images come from O.update_grid_map under the oracle's own
Philox mirror (the device senses the same positions under the same (seed, episode, agent, stage 0) streams at reset), the belief maps
are constructed float32 log-odds whose float64 sigmoid the oracle sees, comm rows, pre-move positions and actions are written by the
test on both sides.  No class-weight tie is excused: test_feature_cases_are_decidable (no GPU) holds every deciding average of
planes 3, 4 and 8 at least MARGIN away from 0.499 / 0.501, and asserts that each case has the geometry its row claims."""
import functools
import types

import numpy as np
import pytest

import ipp_oracle as O
from configs import make_params

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

from test_hip_ig_planner import build_maps, sigmoid64   # noqa: E402  (the planner tests' map writer: observed, saturated, beyond the clip, +-inf, prior)

RTOL = 1e-5                  # README: float outputs within 1e-5 relative
MARGIN = 1e-6                # distance every deciding average keeps from a class-weight threshold
SEED = 0x1234567ABC          # Philox seed of the device context and of the oracle's mirror
FEAT = 11
EXACT_ACTOR, EXACT_CRITIC = (0, 1, 2), (0, 1, 2, 7, 11)     # budget, id, position / + critic position, other actions


def feature_atol(prior):
    """check_philox_episodes' absolute tolerance of the feature planes."""
    return 2e-6 if prior == 0.5 else 6e-6


def square(angle, number):
    return dict(sensor__field_of_view__angle_x=angle, sensor__field_of_view__angle_y=angle, sensor__pixel__number_x=number,
                sensor__pixel__number_y=number)


def agents(n):
    return dict(experiment__missions__n_agents=n)


# ---- geometries: one env each -> (positions [N, 3] in metres, comm [N, N], pre-move positions or None) -------------------------------
# (small: lattice step 5 m, centre cells [0, 12, 25, 38, 51, 64, 76, 89, 102, 115, 128], half widths 7 / 15 / 22 at 5 / 10 / 15 m)

def geo_nested(d, rng):
    """Three agents on ONE lattice cell at the three altitudes (footprints nested around one centre), a fourth with the same x-edges as
    the top one (same row, same altitude, one step along y), everybody hears everybody: the own rectangle inside received ones
    (agent 1: covered entirely), received ones inside the own (agent 0), shared x-edges, a shared lattice cell in the critic planes."""
    pos = [(25, 25, 15), (25, 25, 5), (25, 30, 15), (25, 25, 10), (30, 25, 10), (20, 20, 5)]
    return np.array(pos), np.ones((6, 6), dtype=np.uint8), None


def geo_one_way(d, rng):
    """Asymmetric comm rows, others at lattice offsets of exactly +-5 (the border of the egocentric plane) and +-6 (just outside);
    the critic's pre-move positions are NOT the sensed ones."""
    pos = np.array([(0, 0, 15), (25, 25, 10), (30, 0, 5), (25, 30, 15), (50, 50, 15), (20, 25, 10)])
    comm = (rng.random_sample((6, 6)) < 0.5).astype(np.uint8)
    for i, j, v in [(0, 1, 1), (1, 0, 0), (0, 2, 1), (2, 0, 0), (0, 3, 1), (1, 2, 1), (4, 1, 1), (1, 4, 1), (4, 5, 1), (5, 4, 0)]:
        comm[i, j] = v
    np.fill_diagonal(comm, 1)
    return pos, comm, pos[[1, 2, 3, 4, 5, 0]]


def geo_corners(d, rng):
    """An agent in each corner at the top altitude (footprints clipped on every side, pasted at both offsets), heard by one in the middle."""
    pos = [(0, 0, 15), (0, 50, 15), (50, 0, 15), (50, 50, 15), (25, 25, 15), (25, 0, 5)]
    return np.array(pos), np.ones((6, 6), dtype=np.uint8), None


def geo_random(d, rng, all_heard=False):
    """Distinct random lattice points at random altitudes, a random asymmetric comm matrix."""
    n, taken = d.n_agents, []
    while len(taken) < n:
        p = (int(rng.randint(d.space_x)) * d.spacing, int(rng.randint(d.space_y)) * d.spacing, d.min_altitude + int(rng.randint(d.space_z)) * d.spacing)
        if p[:2] not in [q[:2] for q in taken]:
            taken.append(p)
    comm = np.ones((n, n), dtype=np.uint8) if all_heard else (rng.random_sample((n, n)) < 0.6).astype(np.uint8)
    np.fill_diagonal(comm, 1)
    return np.array(taken), comm, None


def geo_all_heard(d, rng):
    return geo_random(d, rng, all_heard=True)


def geo_packed16(d, rng):
    """Sixteen agents one lattice step apart in a 4 x 4 block, altitudes mixed: rows of four share both x-edges when they share an altitude."""
    x0, y0 = 5 * int(rng.randint(0, 8)), 5 * int(rng.randint(0, 8))
    pos = [(x0 + 5 * (k // 4), y0 + 5 * (k % 4), (15, 15, 10, 5)[(k + k // 4) % 4]) for k in range(16)]
    order = rng.permutation(16)
    return np.array(pos)[order], np.ones((16, 16), dtype=np.uint8), None


def geo_extremes(d, rng):
    """The near corner, the far corner and the middle at the top altitude, one more agent low down; all heard."""
    n = d.n_agents
    far = (d.space_x - 1) * d.spacing
    pos = [(0, 0, 15), (far, far, 15), (25, 25, 15), (far, 0, 5), (0, far, 10), (25, 0, 10)][:n]
    return np.array(pos), np.ones((n, n), dtype=np.uint8), None


def geo_edges(d, rng):
    """Edge midpoints and a corner at mixed altitudes, random comm."""
    n = d.n_agents
    far = (d.space_x - 1) * d.spacing
    pos = [(far, 25, 15), (25, far, 10), (0, 25, 15), (far, far, 5), (5, 5, 15), (45, 45, 10)][:n]
    comm = (rng.random_sample((n, n)) < 0.6).astype(np.uint8)
    np.fill_diagonal(comm, 1)
    return np.array(pos), comm, None


CASES = {
    # id: config, overrides, one geometry per env, steps t the features are built for, extras               what only it reaches
    "small_geometry": dict(config="small", over=agents(6), envs=[geo_nested, geo_one_way, geo_corners, geo_random], ts="ends"),
    "small_team16": dict(config="small", over=dict(experiment__uav__communication_range=100, experiment__constraints__num_actions=27, **agents(16)),
                         envs=[geo_all_heard, geo_packed16], ts=(3,)),                                  # 32 edges of MAX_EDGES 34
    "small_mixed": dict(config="small", over=agents(6), envs=[geo_random, geo_nested, geo_one_way], ts=(5,), teams=[1, 3, 6]),
    "narrow42": dict(config="default", over=square(110.0, 12), envs=[geo_extremes, geo_edges, geo_random], ts=(2,)),   # vec == 1
    "edge45": dict(config="default", over=square(110.0, 13), envs=[geo_extremes, geo_edges, geo_random], ts=(2,)),     # gy % 4 == 1, S = 44
    "default493": dict(config="default", over=agents(3), envs=[geo_extremes, geo_random], ts=(7,)),     # bins 44.8 cells wide
    "wide1110": dict(config="small", over=dict(sensor__pixel__number_x=130, sensor__pixel__number_y=130, **agents(3)), envs=[geo_extremes],
                     ts=(1,)),                                                                          # bins of 101 / 102 cells: mask word 3
    "small_tiles": dict(config="small", over={}, envs=[geo_extremes, geo_random, geo_edges], ts=(4,), layout="tiles"),
    "small_prior03": dict(config="small", over=dict(mapping__prior=0.3), envs=[geo_extremes, geo_random, geo_edges], ts=(4,)),
}
GRIDS = {"small_geometry": 128, "small_team16": 128, "small_mixed": 128, "narrow42": 42, "edge45": 45, "default493": 493, "wide1110": 1110,
         "small_tiles": 128, "small_prior03": 128}
# seed of a case's maps, random positions, comm rows and actions: the first from 100 + (position in CASES) on whose deciding averages all
# keep 5e-6 from the thresholds (saturated and half-observed bins hover around 0.5: about one seed in three comes within 1e-6)
MAP_SEED = {"small_geometry": 104, "small_team16": 114, "small_mixed": 103, "narrow42": 103, "edge45": 105, "default493": 105, "wide1110": 112,
            "small_tiles": 108, "small_prior03": 108}


def bin_cells(b, g):
    """Cells that bin b of an axis of g cells touches."""
    return min(g, -(-(b + 1) * g // FEAT)) - (b * g) // FEAT


def case_params(case, n_agents=None):
    c = CASES[case]
    over = dict(c["over"]) if n_agents is None else dict(c["over"], **agents(n_agents))
    return make_params(c["config"], **over)


@functools.lru_cache(maxsize=None)
def build_case(case):
    """Inputs of a case and the oracle's answer to them (computed once, never modified)."""
    from ippmarl.derived import DerivedConstants
    c = CASES[case]
    params = case_params(case)
    d = O.Derived(params)
    d.exact = True
    dc = DerivedConstants(params, philox_seed=SEED)
    E, N, gx, gy = len(c["envs"]), d.n_agents, int(d.gx), int(d.gy)
    teams = list(c.get("teams", [N] * E))
    rng = np.random.RandomState(MAP_SEED[case])
    ts = (0, d.budget) if c["ts"] == "ends" else tuple(c["ts"])
    episodes = [11 + 7 * e for e in range(E)]
    pos, comm, pos_pre = np.zeros((E, N, 3), dtype=np.int32), np.zeros((E, N, N), dtype=np.uint8), np.zeros((E, N, 3), dtype=np.int32)
    for e, geo in enumerate(c["envs"]):
        p, cm, pre = geo(d, rng)
        pos[e], comm[e], pos_pre[e] = p, cm, p if pre is None else pre
    for e in range(E):      # agents that do not fly: whatever their comm entries hold, nobody hears them
        comm[e, :, teams[e]:] = 1
    actions = rng.randint(0, d.num_actions, size=(E, N)).astype(np.int32)
    local = build_maps(d, dc.logit_clip, E, rng)                                                     # [E, N, gx, gy] float32 log-odds
    glob = build_maps(d, dc.logit_clip, E + 1, rng, n_agents=1)[1:, 0]   # (map (0, 0) is the all-saturated one)
    p_local, p_glob = sigmoid64(local), sigmoid64(glob)
    dsize = (d.space_y, d.space_x)
    want_obs = {t: np.zeros((E, N, FEAT, FEAT, 7)) for t in ts}
    want_state = {t: np.zeros((E, N, FEAT, FEAT, 12), dtype=np.float32) for t in ts}
    rects = np.zeros((E, N, 4), dtype=np.int32)
    fulls = np.zeros((E, N, 4), dtype=np.int32)
    decide = []                                  # (what, env, agent, float64 [11, 11])
    for e in range(E):
        na = teams[e]
        d_e = O.Derived(case_params(case, na))   # the reference's team size is a per-run parameter: env e is a run with n_agents = na
        d_e.exact = True
        truth = O.make_truth(d, episodes[e])
        info = {}
        for j in range(na):
            full, fc = O.project_field_of_view(d, pos[e, j])
            corr = O.philox_correctness(SEED, episodes[e], j, 0, fc, d.gy, O.noise_of_altitude(pos[e, j, 2]))
            _, _, fc, m2c, fimg = O.update_grid_map(d, truth, pos[e, j], O.init_prior_map(d), corr)
            info[j] = dict(position=pos[e, j], map2communicate=m2c, footprint_img=fimg)
            rects[e, j], fulls[e, j] = fc, full
            decide.append(("fp", e, j, O.area_resize(np.asarray(fimg, dtype=np.float64), dsize)))
            decide.append(("local", e, j, O.area_resize(p_local[e, j], dsize)))
        decide.append(("global", e, -1, O.area_resize(p_glob[e], dsize)))
        published = {j: dict(position=pos_pre[e, j], map2communicate=info[j]["map2communicate"]) for j in range(na)}
        for t in ts:
            for i in range(na):
                heard = {j: info[j] for j in range(na) if j == i or comm[e, i, j]}      # ascending j, like the reference's dict
                obs = O.actor_observation(d_e, heard, p_local[e, i], truth, i, t)
                want_obs[t][e, i] = obs
                want_state[t][e, i] = O.critic_state(d_e, published, p_glob[e], obs, actions[e, :na], i, truth)
    return types.SimpleNamespace(case=case, params=params, d=d, dc=dc, E=E, N=N, teams=teams, ts=ts, episodes=episodes, pos=pos, comm=comm,
                                 pos_pre=pos_pre, actions=actions, local=local, glob=glob, rects=rects, fulls=fulls, decide=decide,
                                 want_obs=want_obs, want_state=want_state, layout=c.get("layout", "rows"))


def lattice(b, p):
    return np.asarray(p)[..., :2] // b.d.spacing


def heard_pairs(b, e):
    """(i, j): flying agent i hears flying agent j != i in env e."""
    na = b.teams[e]
    return [(i, j) for i in range(na) for j in range(na) if i != j and b.comm[e, i, j]]


def case_properties(b):
    """What the constructed inputs of a case actually hold (asserted per case in test_feature_cases_are_decidable)."""
    d, gy = b.d, int(b.d.gy)
    props = dict(grid=(int(d.gx), int(d.gy)), vec=b.dc.vec, widest_bin=max(bin_cells(k, gy) for k in range(FEAT)))
    shared_edge = nested_own_in_other = nested_other_in_own = covered_own = one_way = False
    off5, off6, edges, corners, shared_cell, mask_bit = set(), set(), 0, set(), False, 0
    clip_xy = far_clip = False
    for e in range(b.E):
        na = b.teams[e]
        r = b.rects[e]
        for i in range(na):
            part = [i] + [j for j in range(na) if j != i and b.comm[e, i, j]]
            edges = max(edges, 2 * len(part))
            for j in part[1:]:
                shared_edge |= bool(len({r[i][2], r[i][3]} & {r[j][2], r[j][3]}))
                inside = lambda a, c: r[c][0] <= r[a][0] and r[a][1] <= r[c][1] and r[c][2] <= r[a][2] and r[a][3] <= r[c][3]   # noqa: E731
                nested_own_in_other |= bool(inside(i, j))
                nested_other_in_own |= bool(inside(j, i))
                off = lattice(b, b.pos[e, j]) - lattice(b, b.pos[e, i])
                if max(abs(off)) == 5:
                    off5 |= {int(v) for v in off if abs(v) == 5}
                if max(abs(off)) == 6:
                    off6 |= {int(v) for v in off if abs(v) == 6}
            cover = np.zeros((r[i][3] - r[i][2], r[i][1] - r[i][0]), dtype=bool)
            for j in part[1:]:
                x0, x1, y0, y1 = max(r[j][2], r[i][2]), min(r[j][3], r[i][3]), max(r[j][0], r[i][0]), min(r[j][1], r[i][1])
                if x1 > x0 and y1 > y0:
                    cover[x0 - r[i][2]:x1 - r[i][2], y0 - r[i][0]:y1 - r[i][0]] = True
            covered_own |= bool(cover.size and cover.all())
            # the highest mask bit a participating rectangle sets in any column bin (bit k = cell c0 + k of the bin)
            for j in part:
                for k in range(FEAT):
                    c0, c1 = (k * gy) // FEAT, min(gy, -(-(k + 1) * gy // FEAT))
                    hi = min(r[j][1], c1) - c0
                    if hi > max(r[j][0], c0) - c0:
                        mask_bit = max(mask_bit, hi - 1)
            clipped_lo_x, clipped_lo_y = r[i][2] > b.fulls[e, i][2], r[i][0] > b.fulls[e, i][0]
            clip_xy |= bool(clipped_lo_x and clipped_lo_y)                           # xoff and yoff both nonzero
            far_clip |= bool(r[i][3] < b.fulls[e, i][3] and r[i][1] < b.fulls[e, i][1])
            if b.pos[e, i, 2] == d.max_altitude:
                corners.add(tuple(int(v) for v in lattice(b, b.pos[e, i])))
        one_way |= any(not b.comm[e, j, i] for i, j in heard_pairs(b, e))
        cells = [tuple(v) for v in lattice(b, b.pos_pre[e, :na])]
        shared_cell |= len(set(cells)) < len(cells)
    last = d.space_x - 1
    props.update(shared_edge=shared_edge, nested_own_in_other=nested_own_in_other, nested_other_in_own=nested_other_in_own,
                 covered_own=covered_own, one_way=one_way, off5=off5, off6=off6, edges=edges, shared_cell=shared_cell, mask_bit=mask_bit,
                 four_corners={(0, 0), (0, last), (last, 0), (last, last)} <= corners, clip_xy=clip_xy, far_clip=far_clip)
    return props


def threshold_distance(b):
    """Smallest distance of any deciding average of planes 3, 4 and 8 from a class-weight threshold, and where it is."""
    best = (np.inf, None)
    for what, e, i, v in b.decide:
        dist = np.minimum(np.abs(v - 0.499), np.abs(v - 0.501))
        k = np.unravel_index(int(np.argmin(dist)), dist.shape)
        if dist[k] < best[0]:
            best = (float(dist[k]), (what, e, i, k, float(v[k])))
    return best


@pytest.mark.parametrize("case", list(CASES))
def test_feature_cases_are_decidable(case):
    """No GPU: every deciding average (the oracle's decide_local / decide_fp / decide_global: the 11 x 11 area averages whose class
    weight planes 3, 4 and 8 carry) is at least MARGIN away from 0.499 and 0.501, the grid is the one the case is named for, and the
    constructed inputs hold the geometry the case is there for."""
    b = build_case(case)
    p = case_properties(b)
    print(case, {k: v for k, v in p.items()})
    assert p["grid"] == (GRIDS[case], GRIDS[case])
    dist, where = threshold_distance(b)
    print(f"{case}: closest deciding average {where}, {dist:.3e} from a threshold")
    assert dist >= MARGIN, (dist, where)
    assert all(0 <= t <= b.d.budget for t in b.ts)
    if case == "small_geometry":
        assert p["shared_edge"] and p["nested_own_in_other"] and p["nested_other_in_own"] and p["covered_own"] and p["one_way"]
        assert p["off5"] == {-5, 5} and p["off6"] == {-6, 6} and p["shared_cell"] and p["four_corners"] and p["clip_xy"] and p["far_clip"]
        assert b.ts == (0, b.d.budget) and not np.array_equal(b.pos_pre[1], b.pos[1])
        assert len({int(b.actions[0, j]) for j in (0, 1, 3)}) == 3      # the agents sharing a lattice cell in env 0 chose different actions
    if case == "small_team16":
        assert p["edges"] == 32 and b.d.num_actions == 27 and p["shared_edge"]
    if case == "small_mixed":
        assert b.teams == [1, 3, 6] and b.N == 6 and all(b.comm[e, :, n:].all() for e, n in enumerate(b.teams))
        for e, n in enumerate(b.teams):      # an absent agent within +-5 lattice steps of a flying one: hearing it would show in the position plane
            assert n == b.N or any(np.abs(lattice(b, b.pos[e, j]) - lattice(b, b.pos[e, i])).max() <= 5 for i in range(n) for j in range(n, b.N)), e
    if case == "narrow42":
        assert p["vec"] == 1 and b.dc.tile_stride == 40 and b.dc.radius_x == [6, 12, 18] and p["clip_xy"] and p["far_clip"]
    if case == "edge45":
        assert p["vec"] == 4 and b.dc.tile_stride == 44 and GRIDS[case] % 4 == 1 and p["clip_xy"] and p["far_clip"]
    if case == "default493":
        assert 493 % FEAT != 0 and p["widest_bin"] == 46 and b.N == 3
    if case == "wide1110":
        assert p["widest_bin"] > 96 and p["mask_bit"] >= 96 and b.E == 1 and b.N == 3 and GRIDS[case] % 4 == 2
    if case == "small_tiles":
        assert b.layout == "tiles"
    if case == "small_prior03":
        assert b.d.prior == 0.3 and np.any(b.local == np.float32(np.log(0.3 / 0.7)))      # an untouched prior region


# ---- the device side -------------------------------------------------------------------------------------------------------------------

def device_features(b):
    """{t: (obs [E, N, 11, 11, 7], state [E, N, 11, 11, 12])} from ippm_actor_features / ippm_critic_features on the case's inputs."""
    from ippmarl import _ffi
    from ippmarl.vec_env import VecEnv
    teams = None if b.teams == [b.N] * b.E else b.teams
    env = VecEnv(b.params, b.E, philox_seed=SEED, track_area=False, map_layout=b.layout, team_sizes=teams)
    assert env.tiled == (b.layout == "tiles") and env.d.vec == b.dc.vec
    env.reset(b.episodes, start_positions=torch.from_numpy(b.pos))
    # the start sensing wrote `rect` (and `code`) for the chosen positions: the oracle's clipped footprints, bit for bit
    got_rect = env.rect.cpu().numpy()
    for e, na in enumerate(b.teams):
        assert np.array_equal(got_rect[e, :na], b.rects[e, :na]), (e, got_rect[e].tolist(), b.rects[e].tolist())
    dev = env.device
    env.local.copy_(env.tiles_view(torch.from_numpy(b.local).to(dev)))
    env.glob.copy_(env.tiles_view(torch.from_numpy(b.glob).to(dev)))
    env.rebuild_area()
    env.comm.copy_(torch.from_numpy(b.comm).to(dev))
    env.pos_pre.copy_(torch.from_numpy(b.pos_pre).to(dev))
    env.action.copy_(torch.from_numpy(b.actions).to(dev))
    out = {}
    for t in b.ts:
        obs = torch.full((b.E, b.N, FEAT, FEAT, _ffi.ACTOR_PLANES), float("nan"), dtype=torch.float32, device=dev)     # every element must be written
        state = torch.full((b.E, b.N, FEAT, FEAT, _ffi.CRITIC_PLANES), float("nan"), dtype=torch.float32, device=dev)
        env.ctx.call("ippm_actor_features", _ffi.ptr(env.area), _ffi.ptr(env.code), _ffi.ptr(env.rect), _ffi.ptr(env.pos), _ffi.ptr(env.comm),
                     int(t), _ffi.ptr(obs), b.E, env.stream)
        env.ctx.call("ippm_critic_features", _ffi.ptr(env.area), _ffi.ptr(env.rect), _ffi.ptr(env.pos_pre), _ffi.ptr(env.action), _ffi.ptr(obs),
                     _ffi.ptr(state), b.E, env.stream)
        out[t] = (obs.cpu().numpy(), state.cpu().numpy())
    return out


def hold_planes(got, want, exact, atol, tag):
    """The planes in ``exact`` equal the oracle's value after float32 rounding; every other plane at rtol 1e-5 and ``atol``."""
    assert np.all(np.isfinite(got)), f"{tag}: elements left unwritten or not finite at {np.argwhere(~np.isfinite(got))[:5].tolist()}"
    want = np.asarray(want, dtype=np.float64)
    for p in range(got.shape[-1]):
        g, w = got[..., p], want[..., p]
        if p in exact:
            bad = np.argwhere(g != w.astype(np.float32))
            assert not len(bad), f"{tag} plane {p}: {len(bad)} elements differ, first at (env, agent, a, b) {bad[0].tolist()}: " \
                                 f"{g[tuple(bad[0])]!r} vs {w[tuple(bad[0])]!r}"
        else:
            err = np.abs(g - w) / (atol + RTOL * np.abs(w))
            k = np.unravel_index(int(np.argmax(err)), err.shape)
            print(f"{tag} plane {p}: worst |got - want| / (atol + rtol |want|) = {err[k]:.3f} at {tuple(int(v) for v in k)}: {g[k]!r} vs {w[k]!r}")
            np.testing.assert_allclose(g, w, rtol=RTOL, atol=atol, err_msg=f"{tag} plane {p}")


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_features_on_constructed_inputs_match_oracle(case):
    """ippm_actor_features and ippm_critic_features on constructed positions, comm rows, maps, pre-move positions and actions against
    O.actor_observation / O.critic_state: budget, id, position and action planes equal after float32 rounding, every other plane at
    rtol 1e-5 and check_philox_episodes' atol; rows of agents that do not fly are zero; no class-weight tie is excused (the inputs
    keep every deciding average MARGIN away from the thresholds: test_feature_cases_are_decidable)."""
    b = build_case(case)
    dist, where = threshold_distance(b)
    assert dist >= MARGIN, (dist, where)
    atol = feature_atol(b.d.prior)
    got = device_features(b)
    for t in b.ts:
        obs, state = got[t]
        hold_planes(obs, b.want_obs[t], EXACT_ACTOR, atol, f"{case} t={t} obs")
        hold_planes(state, b.want_state[t], EXACT_CRITIC, atol, f"{case} t={t} state")
        for e, na in enumerate(b.teams):
            assert not obs[e, na:].any() and not state[e, na:].any(), (case, e)


# ---- the bin-width limit of the footprint planes --------------------------------------------------------------------------------------

def widest_bin(g):
    return max(bin_cells(k, g) for k in range(FEAT))


def feature_entry_points(params, grid=None):
    """(name, call) of the two feature entry points on a bare context with a few small dummy buffers and n_envs = 0: the checks run,
    nothing is launched.  ``grid``: the context's grid is set to grid x grid cells, whatever ``params`` derive (only the checks see it)."""
    from ippmarl import _ffi
    from ippmarl.derived import DerivedConstants
    dc = DerivedConstants(params)
    if grid is not None:
        dc.grid_x = dc.grid_y = int(grid)
    ctx = _ffi.Context(dc)
    assert (ctx.cfg.grid_x, ctx.cfg.grid_y) == ((dc.grid_x, dc.grid_y))
    dummy = torch.zeros(64, dtype=torch.float64, device="cuda:0")
    p = _ffi.ptr(dummy)
    return ctx, [("ippm_actor_features", lambda: ctx.call("ippm_actor_features", p, p, p, p, p, 0, p, 0, None)),
                 ("ippm_critic_features", lambda: ctx.call("ippm_critic_features", p, p, p, p, p, p, 0, None))]


def test_bin_width_bound():
    """No GPU: the grids whose widest column bin fits the 128-bit masks are exactly those up to 1398 cells and 1408 (= 11 x 128)."""
    assert [g for g in range(FEAT, 4000) if widest_bin(g) <= 128] == list(range(FEAT, 1399)) + [1408]
    assert widest_bin(1400) == 129 and bin_cells(3, 1400) == 129      # cells 381 .. 509


@gpu
def test_too_wide_grid_is_rejected():
    """too_wide: the footprint planes (6 and 10) hold the cells of a column bin in 128-bit masks; default with angle 30.0 and
    number 100 is 1866 x 1866 with bins of 171 cells, whose planes would silently lose the cells beyond bit 127.  Both entry points
    refuse it with -2 and a message naming the limit, as they refuse 1399, 1400 and 1409 (bins of 129 cells); 1398 and 1408 x 1408
    (bins of at most / exactly 128 cells) pass the check."""
    from ippmarl import _ffi
    wide = make_params("default", **square(30.0, 100))
    d = O.Derived(wide)
    assert (int(d.gx), int(d.gy)) == (1866, 1866) and widest_bin(1866) == 171
    fits = make_params("small", sensor__pixel__number_x=165, sensor__pixel__number_y=165)
    d = O.Derived(fits)
    assert (int(d.gx), int(d.gy)) == (1408, 1408) and widest_bin(1408) == 128
    for params, grid, cells in [(wide, None, 171), (fits, 1399, 129), (fits, 1400, 129), (fits, 1409, 129)]:
        assert widest_bin(grid or 1866) == cells
        ctx, calls = feature_entry_points(params, grid)
        for name, call in calls:
            with pytest.raises(_ffi.IppmError) as err:
                call()
            msg = str(err.value)
            assert f"{name} failed (-2)" in msg and f"grid_y = {grid or 1866} has a feature bin of {cells} cells" in msg, msg
            assert "at most 128 cells per bin" in msg and "up to 1398 fits, and 1408" in msg, msg
    for grid in (None, 1398, 1397):
        assert widest_bin(grid or 1408) <= 128
        ctx, calls = feature_entry_points(fits, grid)
        for name, call in calls:
            call()


# ---- the area machinery, directly -------------------------------------------------------------------------------------------------------

def bare_context(params, tiled=False):
    from ippmarl import _ffi
    from ippmarl.derived import DerivedConstants
    ctx = _ffi.Context(DerivedConstants(params))
    ctx.call("ippm_set_map_layout", 1 if tiled else 0)
    return ctx


@gpu
@pytest.mark.parametrize("rows,cols", [(11, 11), (12, 43), (33, 44), (65, 45), (31, 47), (100, 36), (493, 1110)])
def test_area_resize_matches_numpy(rows, cols):
    """ippm_area_resize (cv2.resize INTER_AREA to 11 x 11) against O.area_resize in float64: the identity, one cell per lane (width
    < 44), 16-byte groups with a 0 / 1 / 3-cell tail, row counts that are no multiple of the 32-row chunk, a wide rectangle; three
    arrays per call, of scale 1, 1000 and 1e-3.  Bound: 1e-6 of the array's scale (the kernel accumulates in float64; what is rounded
    is the float32 partial sum of a lane's four cells and the final store)."""
    from ippmarl import _ffi
    rng = np.random.RandomState(rows * 2000 + cols)
    scales = (1.0, 1000.0, 1e-3)
    src = rng.random_sample((len(scales), rows, cols)).astype(np.float32)
    src[rng.random_sample(src.shape) < 0.1] = 0.0
    src[rng.random_sample(src.shape) < 0.1] = 1.0
    src[:, 0, 0], src[:, -1, -1], src[:, 0, -1], src[:, -1, 0] = 1.0, 0.0, 1.0, 0.0
    src *= np.array(scales, dtype=np.float32)[:, None, None]
    ctx = bare_context(make_params("small"))
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    t = torch.from_numpy(src).to(dev)
    dst = torch.full((len(scales), FEAT, FEAT), float("nan"), dtype=torch.float32, device=dev)
    scratch = torch.full((len(scales), FEAT * FEAT), -3.0, dtype=torch.float64, device=dev)      # (the call clears it itself)
    ctx.call("ippm_area_resize", _ffi.ptr(t), rows, cols, _ffi.ptr(dst), _ffi.ptr(scratch), len(scales), stream)
    got = dst.cpu().numpy()
    for k, s in enumerate(scales):
        want = O.area_resize(src[k].astype(np.float64), (FEAT, FEAT))
        err = np.abs(got[k] - want).max() / float(np.abs(src[k]).max())
        print(f"{rows} x {cols}, scale {s}: worst error {err:.3e} of the array's scale")
        np.testing.assert_allclose(got[k], want, rtol=0, atol=1e-6 * float(np.abs(src[k]).max()))


AREA_SENTINEL = -7.0
# |area / (gx gy) - exact| <= 5e-7: a cell's float32 sigmoid (exp, add, reciprocal at 1 - 2 ulp each) is within 4 ulp of 1 = 2.4e-7 of
# the float64 one, a lane's four-cell partial sums and their weighted product add three float32 roundings (1.8e-7 relative of a value
# <= 1); every later sum is float64.  (The project holds the same averages from exported probabilities at 3e-7.)
AREA_ATOL = 5e-7


@gpu
@pytest.mark.parametrize("case,tiled", [("narrow42", False), ("default493", False), ("small_geometry", False), ("small_geometry", True)])
def test_area_sums_slots_match_numpy(case, tiled):
    """ippm_area_sums with (maps_per_env, slot0) = (N, 0), (1, N) and (N + 1, 0) -- the local maps, the global map, all of an env's
    maps -- on the constructed maps of a one-cell-per-lane grid, of 493 x 493 and of `small` in both storage layouts: the addressed
    slots hold sum nr nc sigmoid(L) with the oracle's area weights in float64, every other slot keeps its sentinel."""
    from ippmarl import _ffi
    from ippmarl.vec_env import tiles_view
    b = build_case(case)
    E, N, gx, gy = b.E, b.N, int(b.d.gx), int(b.d.gy)
    if not tiled and (gx % 4 or gy % 8):     # tile storage needs whole tiles: these grids have one layout only
        with pytest.raises(_ffi.IppmError):
            bare_context(b.params, True)
    ctx = bare_context(b.params, tiled)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    every = np.concatenate([b.local, b.glob[:, None]], axis=1)                       # [E, N + 1, gx, gy]
    W = O.area_weights(gx, FEAT), O.area_weights(gy, FEAT)
    want = np.einsum("ax,enxy,by->enab", W[0], sigmoid64(every), W[1]).reshape(E, N + 1, FEAT * FEAT)    # area averages
    for maps, per, slot0 in [(b.local, N, 0), (b.glob[:, None], 1, N), (every, N + 1, 0)]:
        stored = tiles_view(torch.from_numpy(np.ascontiguousarray(maps)).to(dev), tiled).contiguous()
        area = torch.full((E, N + 1, FEAT * FEAT), AREA_SENTINEL, dtype=torch.float64, device=dev)
        ctx.call("ippm_area_sums", _ffi.ptr(stored), _ffi.ptr(area), E * per, per, slot0, stream)
        got = area.cpu().numpy()
        addressed = np.zeros(N + 1, dtype=bool)
        addressed[slot0:slot0 + per] = True
        assert np.all(got[:, ~addressed] == AREA_SENTINEL), (per, slot0)
        err = np.abs(got[:, addressed] / (gx * gy) - want[:, addressed])
        print(f"{case} tiled={tiled} (maps_per_env, slot0) = ({per}, {slot0}): worst error of an area average {err.max():.3e}")
        np.testing.assert_allclose(got[:, addressed] / (gx * gy), want[:, addressed], rtol=0, atol=AREA_ATOL)


def entropy_inputs():
    f = np.float32
    edge = [f(0), f(1), f(1e-4), f(0.9999), f(0.5)]
    for thr in (f(0.499), f(0.501)):
        edge += [np.nextafter(thr, f(0)), thr, np.nextafter(thr, f(1))]
    edge += [np.nextafter(f(1e-4), f(0)), np.nextafter(f(0.9999), f(1)), f(0.25), f(0.75), f(0.4985), f(0.5015), f(1e-7), f(1 - 1e-6)]
    rng = np.random.RandomState(17)
    p = np.concatenate([np.array(edge, dtype=np.float32), rng.random_sample(1000).astype(np.float32)])
    target = np.concatenate([p[:len(edge)][::-1], (rng.random_sample(1000) < 0.5).astype(np.float32)]).astype(np.float32)   # edge values in another order, then a ground truth
    return p, target


@gpu
@pytest.mark.parametrize("with_target", [False, True])
def test_entropy_maps_match_numpy(with_target):
    """ippm_entropy_maps (calculate_w_entropy per element) on 0, 1, the clip values, 0.5 and the float32 neighbours of 0.499 / 0.501:
    the weights equal O.class_weights of the same float32 array (of ``target`` when given), the clipped copy equals the float32 clip,
    entropy and weighted entropy are held at rtol 1e-5, atol 2e-6; with all four outputs, and with every combination of null outputs
    ippmarl/utils/state.py uses (no w_entropy) plus each output alone."""
    from ippmarl import _ffi
    p, target = entropy_inputs()
    src = target if with_target else p
    want_w = O.class_weights(src.copy())
    assert want_w.dtype == np.float32 and set(np.unique(want_w)) == {0.0, 0.5, 1.0}
    want_h = O.shannon_entropy(p.astype(np.float64))
    want_grid = np.clip(p, np.float32(1e-4), np.float32(0.9999))
    ctx = bare_context(make_params("small"))
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    dp, dt = torch.from_numpy(p).to(dev), torch.from_numpy(target).to(dev) if with_target else None
    for outputs in [(1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]:
        bufs = [torch.full_like(dp, float("nan")) if on else None for on in outputs]
        ctx.call("ippm_entropy_maps", _ffi.ptr(dp), _ffi.ptr(dt), *[_ffi.ptr(x) for x in bufs], p.size, stream)
        we, w, se, grid = [None if x is None else x.cpu().numpy() for x in bufs]
        if w is not None:
            assert np.array_equal(w, want_w), np.argwhere(w != want_w)[:5].tolist()
        if grid is not None:
            assert np.array_equal(grid, want_grid)
        if se is not None:
            np.testing.assert_allclose(se, want_h, rtol=RTOL, atol=2e-6)
        if we is not None:
            np.testing.assert_allclose(we, want_w.astype(np.float64) * want_h, rtol=RTOL, atol=2e-6)
    assert torch.equal(dp.cpu(), torch.from_numpy(p))       # the inputs are read-only
