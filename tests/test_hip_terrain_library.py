"""GPU checks of the terrain library (csrc/terrain_library.hip) against its NumPy restatement (tests/terrain_library_ref.py), byte for
byte: the pack, the draw on every class of grid (spare byte, rows that are no multiple of 32 cells, rectangles, 256 x 256) under every
augmentation, the error returns; then the env on top of it -- oracle parity of whole episodes over library truths, SplitVecEnv, and
COMATrainer's rollout / returns_on / curves_on."""
import numpy as np
import pytest

import terrain_library_ref as R
from configs import make_params
from test_hip_features import square

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = 0x1234567ABC


def _maps(M, lgx, lgy, seed):
    """Random maps, cells 0 / 1, about half of them set: no two windows of a library look alike."""
    rng = np.random.RandomState(seed)
    return (rng.rand(M, lgx, lgy) < 0.5).astype(np.uint8)


def _context(params):
    from ippmarl import _ffi
    from ippmarl.derived import DerivedConstants
    d = DerivedConstants(params, philox_seed=SEED)
    return d, _ffi.Context(d)


def _pack(ctx, cells_np, prefill=0xFF):
    from ippmarl import _ffi
    M, lgx, lgy = cells_np.shape
    n = np.zeros(1, dtype=np.int64)
    _ffi.check(ctx.lib.ippm_terrain_library_bytes(M, lgx, lgy, n.ctypes.data), "bytes")
    lib = torch.full((int(n[0]),), prefill, dtype=torch.uint8, device="cuda")
    cells = torch.from_numpy(cells_np).cuda()
    _ffi.check(ctx.lib.ippm_terrain_library_pack(_ffi.ptr(cells), M, lgx, lgy, _ffi.ptr(lib), torch.cuda.current_stream().cuda_stream), "pack")
    torch.cuda.synchronize()
    return lib


@pytest.mark.parametrize("shape", [(3, 70, 67), (2, 5, 64), (1, 3, 129), (2, 300, 517)])
def test_pack_equals_the_reference(shape):
    _, ctx = _context(make_params("small"))
    rng = np.random.RandomState(7)
    cells = rng.choice(np.array([0, 1, 255], dtype=np.uint8), size=shape)
    lib = _pack(ctx, cells)
    want = R.pack_library(cells)
    assert lib.numel() == want.size
    assert np.array_equal(lib.cpu().numpy(), want)


# id: (config, overrides, (gx, gy), library shape with room for every symmetry)
GRIDS = {
    "45x45": ("default", square(110.0, 13), (45, 45), (3, 70, 67)),                                          # gy % 4 != 0: the spare byte
    "64x48": ("small", dict(environment__x_dim=25, environment__y_dim=19), (64, 48), (3, 70, 67)),           # gy % 4 == 0, gy % 32 != 0
    "64x128": ("small", dict(environment__x_dim=25, environment__y_dim=50), (64, 128), (3, 130, 141)),       # gy % 32 == 0, gx != gy
    "256x256": ("c2", {}, (256, 256), (2, 300, 517)),
}
E = 37
# some ids repeated, one beyond 2^32 (the C-ABI takes any int64; VecEnv's own limit is NumPy's legacy seeding)
EPISODES = np.array([11 + 7 * k for k in range(30)] + [11, 18, 2 ** 31 - 1, (1 << 33) + 5, 0, 1, 11], dtype=np.int64)


def _draw(ctx, d, lib, shape, flags, episodes=EPISODES, draws=True):
    """-> (rc, truth bytes [E, truth_bytes], draws [E,4]) of two calls into 0xFF-filled planes, which must agree."""
    from ippmarl import _ffi
    M, lgx, lgy = shape
    ep = torch.from_numpy(episodes).cuda()
    n = ep.numel()
    outs = []
    for _ in range(2):
        truth = torch.full((n, d.truth_bytes), 0xFF, dtype=torch.uint8, device="cuda")
        dr = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")
        rc = ctx.lib.ippm_terrain_library_draw(ctx.handle, _ffi.ptr(ep), _ffi.ptr(lib), M, lgx, lgy, flags, _ffi.ptr(dr) if draws else None,
                                               _ffi.ptr(truth), n, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append((rc, truth.cpu().numpy(), dr.cpu().numpy()))
    assert outs[0][0] == outs[1][0] and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    return outs[0]


def _check_planes(d, maps, flags, truth, draws, episodes=EPISODES):
    from ippmarl import _ffi
    M, lgx, lgy = maps.shape
    gx, gy = d.grid_x, d.grid_y
    assert truth.shape == (len(episodes), R.truth_bytes(gx, gy)) and d.truth_bytes == R.truth_bytes(gx, gy)
    seen = set()
    for e, ep in enumerate(int(v) for v in episodes):
        want = R.draw(SEED, ep, M, lgx, lgy, gx, gy, flags)
        assert tuple(draws[e]) == want == _ffi.host_library_draw(SEED, ep, M, lgx, lgy, gx, gy, flags), (e, ep)
        assert np.array_equal(truth[e], R.truth_plane(maps, want, gx, gy)), (e, ep, want)
        seen.add(want[3])
    for a in range(len(episodes)):          # repeated ids: the same plane bit for bit
        for b in range(a):
            if episodes[a] == episodes[b]:
                assert np.array_equal(truth[a], truth[b])
    return seen


@pytest.mark.parametrize("augment", ["none", "flips", "d4"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_draw_equals_the_reference(grid, augment):
    config, over, dims, shape = GRIDS[grid]
    d, ctx = _context(make_params(config, **over))
    assert (d.grid_x, d.grid_y) == dims
    maps = _maps(*shape, seed=len(grid))
    lib = _pack(ctx, maps)
    flags = R.AUGMENT[augment]
    rc, truth, draws = _draw(ctx, d, lib, shape, flags)
    assert rc == 0, ctx.lib.ippm_last_error()
    seen = _check_planes(d, maps, flags, truth, draws)
    # (a condition on EPISODES, so that "d4" means all eight: each symmetry is met on every grid)
    assert seen == {"none": {0}, "flips": {0, 1, 2, 3}, "d4": set(range(8))}[augment]


@pytest.mark.parametrize("grid", list(GRIDS))
def test_library_of_exactly_the_grids_size(grid):
    """Every offset is 0, the last word of the last row of the last map is read.  Where the grid is not square the transpose does not fit:
    the call returns the error and leaves truth (and draws) untouched."""
    config, over, (gx, gy), _ = GRIDS[grid]
    d, ctx = _context(make_params(config, **over))
    shape = (2, gx, gy)
    maps = _maps(*shape, seed=3)
    lib = _pack(ctx, maps)
    for augment in ("none", "flips", "d4"):
        flags = R.AUGMENT[augment]
        rc, truth, draws = _draw(ctx, d, lib, shape, flags)
        if augment == "d4" and gx != gy:
            assert rc == -1 and "TRANSPOSE" in ctx.lib.ippm_last_error().decode()
            assert (truth == 0xFF).all() and (draws == -1).all()
            continue
        assert rc == 0
        _check_planes(d, maps, flags, truth, draws)
        assert not draws[:, 1:3].any()


def test_turned_library_and_optional_draws():
    """A library that holds the grid only one way round per axis pair: 64 x 48 in 48 x 64 maps fits turned but not straight (error), in
    70 x 64 maps both ways; draws may be NULL; one env alone gives the plane it has in a batch."""
    config, over, _, _ = GRIDS["64x48"]
    d, ctx = _context(make_params(config, **over))
    maps = _maps(2, 48, 64, seed=5)
    rc, truth, _ = _draw(ctx, d, _pack(ctx, maps), maps.shape, R.AUGMENT["d4"])
    assert rc == -1 and (truth == 0xFF).all()
    maps = _maps(2, 70, 64, seed=5)
    lib = _pack(ctx, maps)
    rc, truth, draws = _draw(ctx, d, lib, maps.shape, R.AUGMENT["d4"])
    assert rc == 0
    _check_planes(d, maps, R.AUGMENT["d4"], truth, draws)
    rc, truth2, draws2 = _draw(ctx, d, lib, maps.shape, R.AUGMENT["d4"], draws=False)
    assert rc == 0 and np.array_equal(truth, truth2) and (draws2 == -1).all()
    rc, solo, _ = _draw(ctx, d, lib, maps.shape, R.AUGMENT["d4"], episodes=EPISODES[5:6])
    assert rc == 0 and np.array_equal(solo[0], truth[5])
    rc, _, _ = _draw(ctx, d, lib, (0,) + maps.shape[1:], 0)
    assert rc == -1


# ---- the env over a library -------------------------------------------------------------------------------------------------------------

ENV_MAPS = _maps(3, 150, 170, seed=11)
ENV_EPISODES = [11, 18, 25]
_oracles = {}


def _small3():
    return make_params("small", experiment__missions__n_agents=3)


def _library_oracles(params, truths):
    """The oracle's episodes over the library truths, once for both forms of the step."""
    from oracle_pool import philox_episodes
    if "small3" not in _oracles:
        _oracles["small3"] = philox_episodes(params, ENV_EPISODES, SEED, [t.astype(np.float64) for t in truths], build_features=True)
    return _oracles["small3"]


@pytest.mark.parametrize("fused_step", [False, True])
def test_episodes_over_library_truths_match_the_oracle(fused_step):
    """check_philox_episodes' comparison (tests/test_hip_env_parity.py) with terrain="library": after the reset truth_map is the reference's
    crop, then every step against the oracle flying over those truths -- tracked with the network inputs, and env-only."""
    from ippmarl.vec_env import VecEnv, POLICY_UNIFORM
    from test_hip_env_parity import _check_env_step
    from conftest import assert_posteriors
    params = _small3()
    n = 3
    env = VecEnv(params, n, philox_seed=SEED, track_area=not fused_step, terrain="library", terrain_library=ENV_MAPS, library_augment="d4")
    env.reset(ENV_EPISODES)
    gx, gy = env.d.grid_x, env.d.grid_y
    draws = env.library_draws.cpu().numpy()
    want = [R.draw(SEED, ep, 3, 150, 170, gx, gy, R.AUGMENT["d4"]) for ep in ENV_EPISODES]
    assert [tuple(v) for v in draws] == want
    truths = [R.crop(ENV_MAPS, w, gx, gy) for w in want]
    assert np.array_equal(env.truth_map.numpy(), np.stack(truths))
    oracles = _library_oracles(params, truths)
    feats = not fused_step
    for t in range(env.d.budget + 1):
        if fused_step:
            obs = local = None
        else:
            obs = env.build_observations(t, features=True)
            local = env.posterior_local().cpu().numpy()
        reward, done, state = env.steps(t, policy=POLICY_UNIFORM, features=feats)
        comm = env.comm.cpu().numpy()
        glob = env.posterior_global().cpu().numpy()
        sensed = env.posterior_local().cpu().numpy() if fused_step else None
        for e, (log, _, _) in enumerate(oracles):
            _check_env_step(env, e, n, t, log[t], comm, glob, local, sensed, reward, obs, state, feats)
    final = env.posterior_local().cpu().numpy()
    for e, (_, final_local, _) in enumerate(oracles):
        assert_posteriors(final[e], final_local, strict=True, msg=f"final local e={e}")
    assert env.counters()["work_list_rejects"] == 0
    # an explicit truth still wins over the env's terrain; the other terrains stay available per reset
    env.reset(ENV_EPISODES, truth=np.stack(truths)[::-1].copy())
    assert np.array_equal(env.truth_map.numpy(), np.stack(truths)[::-1])
    env.reset(ENV_EPISODES, terrain="split")
    import ipp_oracle as O
    assert np.array_equal(env.truth_map[0].numpy(), O.make_truth(O.Derived(params), ENV_EPISODES[0]).astype(np.uint8))
    env.reset(ENV_EPISODES)
    assert np.array_equal(env.truth_map.numpy(), np.stack(truths))


def test_constructor_and_reset_errors():
    from ippmarl import _ffi
    from ippmarl.vec_env import VecEnv
    params = _small3()
    with pytest.raises(ValueError, match="unknown terrain"):
        VecEnv(params, 2, terrain="mountains")
    with pytest.raises(ValueError, match="terrain_library"):
        VecEnv(params, 2, terrain="library")
    with pytest.raises(_ffi.IppmError, match="smaller than the grid"):
        VecEnv(params, 2, terrain="library", terrain_library=_maps(2, 100, 200, seed=1))
    with pytest.raises(_ffi.IppmError, match="TRANSPOSE"):      # holds the turned grid only with "flips"
        VecEnv(make_params("small", environment__x_dim=25, environment__y_dim=50), 2, terrain="library", terrain_library=_maps(2, 64, 128, seed=1))
    with pytest.raises(ValueError, match="library_augment"):
        VecEnv(params, 2, terrain="library", terrain_library=ENV_MAPS, library_augment="rot90")
    env = VecEnv(params, 2, terrain="split")
    assert env.library_draws is None
    with pytest.raises(ValueError, match="terrain_library"):
        env.reset([1, 2], terrain="library")
    with pytest.raises(ValueError, match="unknown terrain"):
        env.reset([1, 2], terrain="mountains")
    # a list of maps and a bool tensor are the same library as the array; prefetch_terrain is a no-op here
    a = VecEnv(params, 2, philox_seed=SEED, terrain="library", terrain_library=[m for m in ENV_MAPS], library_augment="flips", track_area=False)
    b = VecEnv(params, 2, philox_seed=SEED, terrain="library", terrain_library=torch.from_numpy(ENV_MAPS).bool(), library_augment="flips",
               track_area=False)
    a.prefetch_terrain([5, 6])
    assert a._side is None
    a.reset([5, 6])
    b.reset([5, 6])
    assert torch.equal(a.truth, b.truth) and torch.equal(a.library_draws, b.library_draws) and a.truth.any()


def test_terrain_class_times_the_draw():
    from ippmarl.vec_env import VecEnv
    env = VecEnv(_small3(), 4, philox_seed=SEED, terrain="library", terrain_library=ENV_MAPS, track_area=False)
    env.profile = True
    env.reset([1, 2, 3, 4])
    times = env.event_times_us()
    assert times["terrain"]["launches"] == 1 and "k_library_draw" in times["terrain"]["kernel"]


@pytest.mark.parametrize("parts", [2, 3])
def test_split_batch_draws_the_same_planes(parts):
    from ippmarl.vec_env import SplitVecEnv, VecEnv
    params = _small3()
    eps = [40 + 3 * k for k in range(7)]
    one = VecEnv(params, 7, philox_seed=SEED, track_area=False, terrain="library", terrain_library=ENV_MAPS)
    one.reset(eps)
    split = SplitVecEnv(params, 7, parts=parts, philox_seed=SEED, terrain="library", terrain_library=ENV_MAPS)
    split.reset(eps)
    split.join()
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([p.truth for p in split.parts]), one.truth)
    assert torch.equal(torch.cat([p.library_draws for p in split.parts]), one.library_draws)
    gx, gy = one.d.grid_x, one.d.grid_y
    want = np.stack([R.truth_plane(ENV_MAPS, R.draw(SEED, ep, 3, 150, 170, gx, gy, 3), gx, gy) for ep in eps])
    assert np.array_equal(one.truth.cpu().numpy(), want)


# ---- COMATrainer ------------------------------------------------------------------------------------------------------------------------

def _trainer(**kw):
    from ippmarl.trainer import COMATrainer
    torch.manual_seed(0)
    return COMATrainer(_small3(), n_envs=3, philox_seed=77, first_episode=21, terrain="library", terrain_library=ENV_MAPS, **kw)


def test_two_trainers_fill_identical_buffers():
    a, b = _trainer(), _trainer()
    a.rollout("train")
    b.rollout("train")
    torch.cuda.synchronize()
    gx, gy = a.env.d.grid_x, a.env.d.grid_y
    want = np.stack([R.crop(ENV_MAPS, R.draw(77, ep, 3, 150, 170, gx, gy, 3), gx, gy) for ep in (21, 22, 23)])
    assert np.array_equal(a.env.truth_map.numpy(), want)
    for name in ("buf_obs", "buf_state", "buf_action", "buf_mask", "buf_reward"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.env.truth, b.env.truth)
    assert a.fingerprint() == b.fingerprint() and "terrain_library" not in a.fingerprint()


def test_fixed_episodes_mean_the_same_truth_for_every_policy():
    tr = _trainer()
    episodes = [40, 41, 42]
    tr.returns_on(episodes, "random")
    first = tr.env.truth.clone()
    tr.returns_on(episodes, "ig")
    assert torch.equal(tr.env.truth, first) and first.any()
    gx, gy = tr.env.d.grid_x, tr.env.d.grid_y
    want = np.stack([R.crop(ENV_MAPS, R.draw(77, ep, 3, 150, 170, gx, gy, 3), gx, gy) for ep in episodes])
    assert np.array_equal(tr.env.truth_map.numpy(), want)


def test_curves_over_library_truths():
    """tests/test_hip_scoring.py's oracle_curves builds its own split truth and takes none from outside, so the curves are held to what
    must be true of them: the prior map's target entropy is 1 bit, the final one is not above it, and a second call -- and a second
    trainer -- gives the same curves bit for bit."""
    tr = _trainer()
    episodes = [21, 22, 23]
    out = tr.curves_on(episodes, "random")
    again = tr.curves_on(episodes, "random")
    other = _trainer().curves_on(episodes, "random")
    ent = out["target_entropy"].cpu().numpy()
    assert ent.shape == (3, tr.T + 1) and not out["faults"].any()
    np.testing.assert_allclose(ent[:, 0], 1.0, rtol=1e-6)
    assert (ent[:, -1] <= ent[:, 0]).all() and (ent[:, -1] < 1.0).any()
    for k in ("target_entropy", "f1", "f1_counts", "actions", "episode_return"):
        assert torch.equal(out[k], again[k]) and torch.equal(out[k], other[k]), k
