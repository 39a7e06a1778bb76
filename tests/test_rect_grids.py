"""Rectangular worlds (environment.x_dim != y_dim, hence grid_x != grid_y and space_x != space_y) against the oracle on the GPU.

Every other parity test flies a square world, where a kernel that took the wrong axis -- or the wrong extent in a tile index, a slab,
a footprint rect -- computes the same thing as one that took the right one.  The shapes below are picked for the branches the library
decides by one axis (csrc/api.hip: the 4-wide instantiations by grid_y >= 44, 128-byte line rounding of row segments by grid_y >= 512,
the tile form of the fusion by grid_y <= 1024; tile storage by grid_x % 4 and grid_y % 8; ippmarl/terrain.py: the native transform when
each side is 128 .. 1024 cells).  The lattice is not 11 x 11 there, so there are no network inputs: env-only episodes."""
import numpy as np
import pytest

import ipp_oracle as O
from configs import make_params
import test_hip_env_parity as P
from test_hip_env_parity import check_philox_episodes

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _world(x, y, **over):
    return dict(environment__x_dim=x, environment__y_dim=y, **over)


# name, overrides, envs, (grid_x, grid_y), tile storage admitted, native terrain
SHAPES = {
    "128x256": ("small", _world(50, 100), 3, (128, 256), True, True),       # whole tiles; native terrain with unequal passes
    "256x128": ("small", _world(100, 50), 3, (256, 128), True, True),
    "128x512": ("small", _world(50, 200), 2, (128, 512), True, True),       # line rounding on (grid_y >= 512) with a narrow x
    "512x128": ("small", _world(200, 50), 2, (512, 128), True, True),       # ... and its transpose (line rounding off)
    "128x1024": ("c2", _world(25, 200), 2, (128, 1024), True, True),        # grid_y at the tile-form limit; 6 x 41 lattice
    "1024x128": ("c2", _world(200, 25), 2, (1024, 128), True, True),        # 41 x 6 lattice
    "256x1280": ("c2", _world(50, 250), 2, (256, 1280), False, False),      # grid_y > 1024: no tile form, the row walker
    "256x512": ("c4", _world(25, 50), 2, (256, 512), True, True),           # 8 UAVs; footprints up to 181 cells on a 256-cell x extent
    "192x128": ("small", _world(75, 50), 3, (192, 128), True, False),       # whole tiles, not a power of two: FFT terrain
    "115x128": ("small", _world(45, 50), 3, (115, 128), False, False),      # not whole tiles: x not a multiple of 4
    "128x115": ("small", _world(50, 45), 3, (128, 115), False, False),      # y not a multiple of 8 (nor of 4)
    "179x256": ("c2", _world(35, 50), 2, (179, 256), False, False),         # x not a multiple of 4
}


def _params(shape):
    name, over = SHAPES[shape][:2]
    return make_params(name, **over)


def _env(params, n_envs, **kw):
    from ippmarl.vec_env import VecEnv
    return VecEnv(params, n_envs, **kw)


def test_shapes_reach_their_branches():
    """The table's shapes are what it says they are: grid sizes, lattice, the tile form and tile storage where admitted (and refused
    where not), the native terrain path -- so a case cannot drift off its branch unnoticed."""
    from ippmarl import _ffi
    for shape, (name, over, _, grid, tiles, native) in SHAPES.items():
        params = _params(shape)
        d = O.Derived(params)
        assert (d.gx, d.gy) == grid and (d.space_x, d.space_y) != (11, 11), shape
        env = _env(params, 1, track_area=False, map_layout="rows", terrain="random_field")
        assert env.d.vec == 4 and (env.d.grid_x, env.d.grid_y) == grid, shape
        assert env._tile_form == (grid[1] <= 1024), shape
        assert env._terrain().native == native, shape
        assert not env.tiled
        if tiles:
            assert _env(params, 1, track_area=False, map_layout="tiles").tiled, shape
        else:
            with pytest.raises(_ffi.IppmError):
                _env(params, 1, track_area=False, map_layout="tiles")
            assert not _env(params, 1, track_area=False, map_layout="auto", layout_envs=1 << 14).tiled, shape


CASES = [(shape, layout, fused) for shape in SHAPES for layout in (("rows", "tiles") if SHAPES[shape][4] else ("rows",))
         for fused in (False, True)]


@pytest.mark.parametrize("shape,layout,fused_step", CASES)
def test_rect_env_step_matches_oracle(shape, layout, fused_step):
    """Every step of 2-3 env-only episodes against the oracle: comm, masks, actions, positions, footprint rects bit for bit, every
    cell of the local and global maps at 1e-5, rewards and S1 / S2 within check_philox_episodes' bounds."""
    name, over, n_envs = SHAPES[shape][:3]
    check_philox_episodes(name, over, n_envs, seed=0x7EC7A9, first_episode=31, track_area=False, fused_step=fused_step, map_layout=layout)


@pytest.mark.parametrize("shape,layout", [("128x256", "rows"), ("1024x128", "rows"), ("256x1280", "rows")])
def test_rect_prior_shift_matches_oracle(shape, layout):
    """prior != 0.5 (the explicit slow path: every fusion shifts the whole grid) on rectangular grids."""
    name, over, n_envs = SHAPES[shape][:3]
    check_philox_episodes(name, dict(over, mapping__prior=0.3), 2, seed=0x7EC7AA, first_episode=5, track_area=False, fused_step=True,
                          map_layout=layout)


@pytest.mark.parametrize("layout", ["rows", "tiles"])
def test_rect_mixed_team_sizes_match_oracle(layout):
    """Env e flies teams[e] UAVs on a 512 x 128 grid; each against an oracle run of that team size."""
    name, over = SHAPES["512x128"][:2]
    check_philox_episodes(name, dict(over, experiment__missions__n_agents=6), 4, team_sizes=[1, 6, 3, 4], track_area=False,
                          fused_step=True, map_layout=layout)


@pytest.mark.parametrize("shape,layout", [("128x1024", "tiles"), ("256x128", "rows"), ("192x128", "tiles")])
def test_rect_random_field_episode_matches_oracle(shape, layout):
    """The device-synthesised field (native transform, or rocFFT at 192 x 128) handed to the oracle; bench.py's step sequence."""
    name, over, n_envs = SHAPES[shape][:3]
    check_philox_episodes(name, over, n_envs, seed=3, first_episode=1, track_area=False, fused_step=True, terrain="random_field",
                          map_layout=layout)


@pytest.mark.parametrize("shape", ["128x1024", "1024x128", "179x256"])
def test_rect_tracked_step_matches_oracle(shape):
    """track_area=True, fused_step=True: the tracked K3 and the tracked fusion (area sums in LDS) on a rectangular grid."""
    name, over, n_envs = SHAPES[shape][:3]
    check_philox_episodes(name, over, n_envs, seed=0x7EC7AB, first_episode=2, track_area=True, fused_step=True, map_layout="rows")


@pytest.mark.parametrize("shape", ["128x1024", "1024x128", "256x512", "179x256", "128x115"])
def test_rect_split_truth_and_start_states(shape):
    """k_fill_truth's half-plane truth and the start states on rectangular grids against the oracle, bit for bit (the check of
    test_reset_matches_numpy_legacy_streams)."""
    params = _params(shape)
    d = O.Derived(params)
    eps = np.arange(1, 17) * 37 + 5
    env = _env(params, len(eps), track_area=False)
    env.reset(eps)
    pos = env.pos.cpu().numpy()
    for e, ep in enumerate(eps):
        for a in range(d.n_agents):
            assert list(pos[e, a]) == list(O.start_state(d, a, int(ep))), (ep, a)
        assert np.array_equal(env.truth_map[e].numpy(), O.make_truth(d, int(ep)).astype(np.uint8)), ep
    assert [tuple(v) for v in env.split_pct.cpu().numpy()] == [O.truth_split_params(int(ep)) for ep in eps]


@pytest.mark.parametrize("shape,n_envs,slabs", [("128x1024", 12, True), ("1024x128", 6, False)])
def test_rect_reset_leaves_nothing_of_the_last_episode(shape, n_envs, slabs, monkeypatch):
    """test_reset_leaves_nothing_of_the_last_episode on rectangular grids: the dirty slabs run 16 rows along x (a 128-cell x extent
    with 1024-cell rows), the reset's fill boxes (1024 rows of 128 cells)."""
    name, over = SHAPES[shape][:2]
    P.test_reset_leaves_nothing_of_the_last_episode(name, over, n_envs, slabs, monkeypatch)


@pytest.mark.parametrize("shape", ["128x256", "256x128", "128x1024", "1024x128", "512x1024"])
def test_rect_native_terrain(shape):
    """The native terrain path's checks (spectrum bins, Hermitian columns, inverse transform against NumPy, packed truth) on
    rectangular power-of-two grids, where the two passes run transforms of different lengths."""
    if shape == "512x1024":
        params = make_params("c4", **_world(50, 100), experiment__missions__n_agents=2)
    else:
        params = _params(shape)
    d = O.Derived(params)
    assert f"{d.gx}x{d.gy}" == shape
    P.check_native_terrain(params)


def test_rect_fft_terrain():
    """The FFT path's checks on 192 x 128: whole tiles, not a power of two."""
    P.check_fft_terrain(_params("192x128"), np.array([3, 1000003, 17, 4]))


@pytest.mark.parametrize("layout", ["rows", "tiles"])
def test_rect_batch_independence(layout):
    """An episode's trajectory does not depend on the batch it runs in, on a 128 x 1024 grid: 512 envs (in ``layout``) against an
    8-env row-major batch of the same episodes -- maps, positions, measurement codes bit for bit, returns to the summation order of
    the float64 reward atomics (as test_full_size_properties)."""
    from ippmarl.vec_env import POLICY_UNIFORM
    params = _params("128x1024")
    E = 512
    env = _env(params, E, track_area=False, map_layout=layout)
    small = _env(params, 8, track_area=False, map_layout="rows")
    assert env.tiled == (layout == "tiles") and not small.tiled
    pick = np.array([1, 2, 3, E // 2 - 12, E // 2 - 11, (3 * E) // 4 + 9, E - 24, E])

    def episode(e):
        returns = torch.zeros(e.E, device=e.device)
        for t in range(e.d.budget + 1):
            r, _, _ = e.steps(t, policy=POLICY_UNIFORM, features=False)
            returns += r[:, 0]
        return returns

    env.reset(np.arange(1, E + 1))
    small.reset(pick)
    returns, small_returns = episode(env), episode(small)
    assert int(env.fault.abs().sum()) == 0 and int(small.fault.abs().sum()) == 0
    assert env.counters()["work_list_rejects"] == 0 and small.counters()["work_list_rejects"] == 0
    assert torch.equal(env.rows_view(env.local[pick - 1]), small.rows_view(small.local))
    assert torch.equal(env.rows_view(env.glob[pick - 1]), small.rows_view(small.glob))
    assert torch.equal(env.pos[pick - 1], small.pos)
    assert torch.equal(env.code[pick - 1], small.code)
    torch.testing.assert_close(returns[pick - 1], small_returns, rtol=1e-6, atol=1e-6)
    p = env.pos.cpu().numpy()
    assert p[..., 0].max() <= env.d.x_dim_m and p[..., 1].max() <= env.d.y_dim_m
