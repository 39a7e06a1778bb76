"""GPU tests of the map scoring pass (csrc/score.hip: ippm_score_maps; VecEnv.score_maps) and of the per-step curves built on it
(COMATrainer.curves_on): constructed maps against float64 (O.target_entropy / O.f1_counts on the float64 sigmoid of the very float32
log-odds uploaded), the nearly saturated map that decides which entropy form the kernel must use, determinism (run to run, alone
against in a batch, against the older single-purpose passes), the curves of every policy against the oracle flying the actions the
device reports, and that curves_on leaves the trainer as it found it."""
import numpy as np
import pytest

import ipp_oracle as O
from configs import make_params

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_hip_features import square            # noqa: E402  (the 45 x 45 / 42 x 42 grids of that file's edge45 / narrow42 cases)
from test_hip_ig_planner import sigmoid64       # noqa: E402

RTOL = 1e-5      # README: float outputs within 1e-5 relative
DELTA = 1e-5     # O.F1_DECIDABLE_LOGODDS


# ---- the kernel through the C-ABI, on maps and truth planes of the test's own ----------------------------------------------------------

class Scorer:
    """One library context (no env): uploads row-major maps in the context's storage layout and calls ippm_score_maps."""

    def __init__(self, params, tiled=False):
        from ippmarl import _ffi
        from ippmarl.derived import DerivedConstants
        self.ffi = _ffi
        self.d = DerivedConstants(params)
        self.ctx = _ffi.Context(self.d)
        self.ctx.call("ippm_set_map_layout", 1 if tiled else 0)
        self.tiled = tiled
        self.dev = torch.device("cuda:0")
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def upload(self, maps, truth):
        """maps float32 [M,gx,gy] row-major, truth {0,1} [K,gx,gy] -> device tensors (storage layout, bit-packed planes)."""
        from ippmarl.vec_env import tiles_view
        m = tiles_view(torch.from_numpy(np.ascontiguousarray(maps)), self.tiled).contiguous().to(self.dev)
        return m, torch.from_numpy(self.d.pack_truth(truth)).to(self.dev)

    def score(self, maps, truth, mpt, delta=DELTA):
        M = maps.shape[0]
        words = np.zeros(1, dtype=np.int64)
        self.ctx.call("ippm_score_scratch", M, words.ctypes.data)
        scratch = torch.full((int(words[0]),), float("nan"), dtype=torch.float64, device=self.dev)
        ent = torch.full((M,), float("nan"), dtype=torch.float64, device=self.dev)        # every output element is written:
        counts = torch.full((M, 3, 3), -7, dtype=torch.int64, device=self.dev)            # the caller zeroes nothing
        p = self.ffi.ptr
        self.ctx.call("ippm_score_maps", p(maps), p(truth), mpt, float(delta), p(ent), p(counts), p(scratch), M, self.stream)
        return ent.cpu().numpy(), counts.cpu().numpy()

    def old_passes(self, maps, truth, mpt, thresholds):
        M = maps.shape[0]
        p = self.ffi.ptr
        ent = torch.zeros(M, dtype=torch.float64, device=self.dev)
        self.ctx.call("ippm_weighted_entropy", p(maps), p(truth), mpt, p(ent), M, self.stream)
        out = []
        for thr in thresholds:
            c = torch.zeros(M, 3, dtype=torch.int64, device=self.dev)
            self.ctx.call("ippm_f1_counts", p(maps), p(truth), mpt, float(thr), p(c), M, self.stream)
            out.append(c.cpu().numpy())
        return ent.cpu().numpy(), np.stack(out, 1)


def constructed_maps(d, n_maps, rng):
    """float32 log-odds [n_maps,gx,gy]: the prior as background, and cells drawn from exactly 0, the "exactly cancelled" +-1e-7, observed
    values +-0.5 .. +-6 (a fixed ladder and a continuous draw), the clip +-lc and beyond it +-12."""
    lc = np.float32(d.logit_clip)
    ladder = np.array([0.0, 1e-7, -1e-7, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 3.3, -3.3, 4.7, -4.7, 6.0, -6.0, lc, -lc, 12.0, -12.0], dtype=np.float32)
    shape = (n_maps, d.grid_x, d.grid_y)
    maps = np.full(shape, np.float32(d.logit_prior), dtype=np.float32)
    kind = rng.random_sample(shape)
    pick = ladder[rng.randint(0, len(ladder), size=shape)]
    cont = (rng.uniform(0.5, 6.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)
    maps = np.where(kind < 0.45, pick, np.where(kind < 0.8, cont, maps)).astype(np.float32)
    maps[:, -1, -3:] = np.array([lc, -1e-7, 2.0], dtype=np.float32)      # the last cells of a map (its tail where the grid has one)
    return maps


def truth_planes(d, k, rng, first):
    """k planes {0,1} [gx,gy] cycling through all 0, all 1, a checkerboard of single cells, a random plane and the inverse checkerboard,
    starting at `first`."""
    xs, ys = np.meshgrid(np.arange(d.grid_x), np.arange(d.grid_y), indexing="ij")
    checker = ((xs + ys) & 1).astype(np.uint8)
    kinds = [np.zeros_like(checker), np.ones_like(checker), checker, (rng.random_sample(checker.shape) < 0.4).astype(np.uint8), 1 - checker]
    return np.stack([kinds[(first + q) % len(kinds)] for q in range(k)])


def assert_decidable(maps):
    """No cell within 1e-6 of a threshold (0, +-1e-5) other than the exactly-cancelled ones (|L| <= 1e-7): every count is an integer
    that any correct implementation reproduces."""
    a = np.abs(maps.astype(np.float64))
    cancelled = a <= np.float64(np.float32(1e-7))
    assert np.all(cancelled | (a >= 1e-6 + DELTA)), "a cell sits within 1e-6 of a threshold"
    assert cancelled.any() and (maps == 0).any()


def assert_scores(d, maps, truth, mpt, ent, counts, msg=""):
    prob = sigmoid64(maps)
    for m in range(maps.shape[0]):
        t = truth[m // mpt]
        n_target = int(t.sum())
        want = O.target_entropy(d, prob[m].copy(), t.astype(np.float64)) * n_target if n_target else 0.0
        if n_target == 0:
            assert ent[m] == 0.0, (msg, m)
        else:
            np.testing.assert_allclose(ent[m], want, rtol=RTOL, atol=0, err_msg=f"{msg} map {m}")
        for k, thr in enumerate((DELTA, 0.0, -DELTA)):
            assert tuple(int(v) for v in counts[m, k]) == O.f1_counts(prob[m], t, thr), (msg, m, thr)
        assert counts[m, 0, 0] + counts[m, 0, 2] == n_target


GRIDS = {
    # id: (config, overrides, tiled, (gx, gy))                what only it reaches
    "edge45": ("default", square(110.0, 13), False, (45, 45)),      # 2025 cells = 1 mod 4: maps from the second on at 4-byte alignment, a tail cell
    "narrow42": ("default", square(110.0, 12), False, (42, 42)),    # the one-cell-per-lane grids of the step kernels; part of one workgroup
    "small_rows": ("small", {}, False, (128, 128)),                   # two parts per map
    "small_tiles": ("small", {}, True, (128, 128)),
    "rect_tiles": ("small", dict(environment__x_dim=50, environment__y_dim=100), True, (128, 256)),   # gx != gy in the tile walk, four parts
    "small_prior03": ("small", dict(mapping__prior=0.3), False, (128, 128)),   # a background at logit(0.3)
}


@pytest.mark.parametrize("n_maps,mpt", [(1, 1), (5, 1), (5, 3), (1, 3)])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_constructed_maps_against_float64(grid, n_maps, mpt):
    config, over, tiled, dims = GRIDS[grid]
    params = make_params(config, **over)
    d = O.Derived(params)
    s = Scorer(params, tiled)
    assert (s.d.grid_x, s.d.grid_y) == dims == (d.gx, d.gy)
    rng = np.random.RandomState(1000 + 10 * n_maps + mpt + len(grid))
    maps = constructed_maps(s.d, n_maps, rng)
    truth = truth_planes(s.d, -(-n_maps // mpt), rng, first=0 if mpt == 1 else 2)
    assert_decidable(maps)
    if grid == "small_prior03":
        assert s.d.prior == 0.3 and np.any(maps == np.float32(np.log(0.3 / 0.7)))
    ent, counts = s.score(*s.upload(maps, truth), mpt)
    assert_scores(d, maps, truth, mpt, ent, counts, grid)


# ---- the saturated case ----------------------------------------------------------------------------------------------------------------

def entropy64(l, lc):
    a = np.minimum(np.abs(np.float64(l)), np.float64(lc))
    e = np.exp(-a)
    return np.log2(1 + e) + a * np.log2(np.e) * e / (1 + e)


def entropy32_log_form(l, lc):
    """ippm_entropy_l in NumPy float32: log2(1 + e) with 1 + e rounded to float32."""
    f = np.float32
    a = np.minimum(np.abs(f(l)), f(lc))
    e = np.exp(-a).astype(f)
    dd = f(1) + e
    return np.log2(dd).astype(f) + (a * f(1.44269504)) * (e / dd)


def entropy32_series_form(l, lc):
    """ippm_entropy_from_e in NumPy float32: the series of log2(1 + e) below e = 2^-6."""
    f = np.float32
    a = np.minimum(np.abs(f(l)), f(lc))
    e = np.exp(-a).astype(f)
    dd = f(1) + e
    series = e * (f(1.44269504) + e * (f(-0.72134752) + e * (f(0.48089835) - f(0.36067376) * e)))
    lg = np.where(e < f(0.015625), series, np.log2(dd).astype(f)).astype(f)
    return lg + (a * f(1.44269504)) * (e / dd)


def test_saturated_maps_need_the_series_form():
    """One 128 x 128 map whose target cells all sit at |L| = 9.2096, one with all of them at the clip: the float32 form of
    ippm_entropy_l misses float64 by 5.8e-5 on the first (NumPy float32 emulation, checked here), the series form holds 8.8e-7 --
    and the kernel is held to 1e-5."""
    params = make_params("small")
    d = O.Derived(params)
    s = Scorer(params)
    lc = np.float32(s.d.logit_clip)
    near = np.float32(9.2096)
    assert near < lc
    h64 = entropy64(near, lc)
    err_log = abs(float(entropy32_log_form(near, lc)) - h64) / h64
    err_series = abs(float(entropy32_series_form(near, lc)) - h64) / h64
    print(f"|L| = 9.2096: log2(1 + e) form {err_log:.2e}, series form {err_series:.2e}; "
          f"at the clip {abs(float(entropy32_log_form(lc, lc)) - entropy64(lc, lc)) / entropy64(lc, lc):.2e}")
    assert 3e-5 < err_log < 1e-4 and err_series < 2e-6
    rng = np.random.RandomState(7)
    truth = (rng.random_sample((2, 128, 128)) < 0.5).astype(np.uint8)
    sign = rng.choice([-1.0, 1.0], size=(2, 128, 128)).astype(np.float32)
    maps = (rng.uniform(0.5, 6.0, size=(2, 128, 128)).astype(np.float32) * sign)
    maps[0][truth[0] == 1] = (near * sign[0])[truth[0] == 1]
    maps[1][truth[1] == 1] = (lc * sign[1])[truth[1] == 1]
    ent, counts = s.score(*s.upload(maps, truth), 1)
    want = [O.target_entropy(d, sigmoid64(maps[m]), truth[m].astype(np.float64)) * int(truth[m].sum()) for m in range(2)]
    np.testing.assert_allclose(want[0], entropy64(near, lc) * int(truth[0].sum()), rtol=1e-9)     # the oracle is the float64 definition
    print("device against float64:", [abs(ent[m] - want[m]) / want[m] for m in range(2)])
    np.testing.assert_allclose(ent, want, rtol=RTOL, atol=0)
    assert_scores(d, maps, truth, 1, ent, counts, "saturated")


# ---- determinism -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", ["edge45", "small_rows", "rect_tiles"])
def test_scores_are_deterministic_and_agree_with_the_single_passes(grid):
    config, over, tiled, _ = GRIDS[grid]
    params = make_params(config, **over)
    s = Scorer(params, tiled)
    rng = np.random.RandomState(31)
    maps = constructed_maps(s.d, 5, rng)
    truth = truth_planes(s.d, 5, rng, first=1)
    dm, dt = s.upload(maps, truth)
    ent, counts = s.score(dm, dt, 1)
    ent2, counts2 = s.score(dm, dt, 1)
    assert np.array_equal(ent.view(np.uint64), ent2.view(np.uint64)) and np.array_equal(counts, counts2)
    for m in range(5):      # a map scored alone = the same map scored in the batch, bit for bit (its storage starts elsewhere: 45 x 45)
        e1, c1 = s.score(dm[m:m + 1].clone(), dt[m:m + 1].clone(), 1)
        assert e1.view(np.uint64)[0] == ent.view(np.uint64)[m] and np.array_equal(c1[0], counts[m]), m
    thresholds = (np.float32(DELTA), 0.0, -np.float32(DELTA))
    old_ent, old_counts = s.old_passes(dm, dt, 1, thresholds)
    assert np.array_equal(counts, old_counts)
    np.testing.assert_allclose(ent, old_ent, rtol=1e-4, atol=0)      # (a sanity link to ippm_weighted_entropy, not the yardstick)


@pytest.mark.parametrize("config,n_maps", [("c2", 40), ("c5", 3)])
def test_parts_per_map_do_not_depend_on_the_batch(config, n_maps):
    """256 x 256 (8 parts a map) and 1024 x 1024 (128 parts): a map of a batch against the same map alone, bit for bit, and the
    counts against ippm_f1_counts."""
    s = Scorer(make_params(config))
    gen = torch.Generator(device=s.dev).manual_seed(5)
    gx, gy = s.d.grid_x, s.d.grid_y
    maps = (torch.rand(n_maps, gx, gy, device=s.dev, generator=gen) * 12 - 6).round(decimals=2)      # (no cell within 1e-3 of a threshold but 0)
    truth = torch.randint(0, 256, (n_maps, s.d.truth_bytes), device=s.dev, generator=gen, dtype=torch.int32).to(torch.uint8)
    ent, counts = s.score(maps, truth, 1)
    for m in (0, n_maps // 2, n_maps - 1):
        e1, c1 = s.score(maps[m:m + 1].clone(), truth[m:m + 1].clone(), 1)
        assert e1.view(np.uint64)[0] == ent.view(np.uint64)[m] and np.array_equal(c1[0], counts[m]), m
    old_ent, old_counts = s.old_passes(maps, truth, 1, (np.float32(DELTA), 0.0, -np.float32(DELTA)))
    assert np.array_equal(counts, old_counts)
    np.testing.assert_allclose(ent, old_ent, rtol=1e-4, atol=0)


# ---- curves against the oracle ---------------------------------------------------------------------------------------------------------

SEED, FIRST = 77, 21
PREFS = [0.05, 0.3, 0.1, 0.25, 0.2, 0.1]


def oracle_curves(params, ep_no, actions):
    """The coma_test loop (coma_test.py:98-196) on one episode flying ``actions[t][i]`` under the device's Philox streams: the global map
    fuses the start measurements and then, every step, the measurements taken right after the move -- no lag.
    -> (target entropies [T+1], F1 [T+1], the counts O.record_f1_counts logged at +-1e-5)."""
    d = O.Derived(params)
    holder, seen = {}, {}

    def correctness(i, s, shape):
        pos = holder["ep"].agents[i]["position"]
        _, fc = O.project_field_of_view(d, pos)
        return O.philox_correctness(SEED, ep_no, i, s, fc, d.gy, O.noise_of_altitude(pos[2]))

    def choose(i, t, mask, obs):
        assert mask[int(actions[t][i])] == 1, (ep_no, t, i, "the device flew an action the oracle masks")
        return int(actions[t][i])

    ep = O.OracleEpisode(params, ep_no, correctness, choose, comm_draw=lambda i, j, t: O.philox_comm_draw(SEED, ep_no, i, j, t),
                         build_features=False, exact=True)
    holder["ep"] = ep
    real_sense = ep._sense

    def sense(i, s):
        real_sense(i, s)
        seen[(i, s)] = ep.agents[i]["map2communicate"]

    ep._sense = sense
    n = d.n_agents
    g = O.init_prior_map(ep.d)
    with O.record_f1_counts() as counts:
        ent, f1 = [O.target_entropy(ep.d, g.copy(), ep.truth)], [O.f1_target(g, ep.truth)]
        for t in range(d.budget + 1):
            ep.step(t)
            if t == 0:
                g = O.fuse_map(ep.d, g, {i: dict(map2communicate=seen[(i, 0)]) for i in range(n)}, None, "global")
            g = O.fuse_map(ep.d, g, [seen[(i, t + 1)] for i in range(n)], None, "global")
            ent.append(O.target_entropy(ep.d, g.copy(), ep.truth))
            f1.append(O.f1_target(g, ep.truth))
    return ent, f1, counts


def assert_curves_match_oracle(out, params_of_env, E, T):
    ent, f1, counts, acts = (out[k].cpu().numpy() for k in ("target_entropy", "f1", "f1_counts", "actions"))
    assert ent.shape == (E, T + 1) and f1.shape == (E, T + 1) and counts.shape == (E, T + 1, 3, 3) and acts.shape[:2] == (T, E)
    assert not out["faults"].any()
    for e in range(E):
        want_ent, want_f1, want_counts = oracle_curves(params_of_env[e], FIRST + e, acts[:, e])
        np.testing.assert_allclose(ent[e], want_ent, rtol=RTOL, atol=0, err_msg=f"env {e}")
        for k in range(T + 1):
            strict, lax = counts[e, k, 0].astype(np.float64), counts[e, k, 2].astype(np.float64)
            assert tuple(counts[e, k, 0].tolist()) == want_counts[k][0], (e, k, "log-odds > +1e-5")
            assert tuple(counts[e, k, 2].tolist()) == want_counts[k][1], (e, k, "log-odds > -1e-5")
            # F1 at p > 0.5: exactly-cancelled cells are rounding noise on either side -- inside the bracket
            worst = 2 * strict[0] / max(2 * strict[0] + lax[1] + strict[2], 1)
            best = 2 * lax[0] / max(2 * lax[0] + strict[1] + lax[2], 1)
            assert worst - 1e-9 <= f1[e, k] <= best + 1e-9 and worst - 1e-9 <= want_f1[k] <= best + 1e-9, (e, k)
        assert ent[e, 0] == pytest.approx(1.0) or params_of_env[e]["mapping"]["prior"] != 0.5
        assert ent[e, -1] <= ent[e, 0]      # (a team that never reaches the target region leaves it at 1)


class StubActor(torch.nn.Module):
    """Fixed preferences: the greedy choice is a function of the masks alone, so the oracle can follow."""

    def forward(self, obs, eps):
        return torch.tensor(PREFS).to(obs.device).expand(obs.shape[0], -1).contiguous(), None


CURVE_CASES = {
    # id: (policy, overrides, forced layout, team sizes)
    "random": ("random", {}, None, None),
    "ig": ("ig", {}, None, None),
    "explicit": ("explicit", {}, None, None),
    "actor": ("actor", {}, None, None),
    "random_tiles": ("random", {}, "1", None),
    "random_prior03": ("random", dict(mapping__prior=0.3), None, None),      # every fusion through the row walker
    "random_teams": ("random", {}, None, [1, 2, 3]),
}


@pytest.mark.parametrize("case", list(CURVE_CASES))
def test_curves_match_the_oracle(case, monkeypatch):
    from ippmarl.trainer import COMATrainer
    policy, over, layout, teams = CURVE_CASES[case]
    if layout is not None:
        monkeypatch.setenv("IPPM_MAP_TILED", layout)
    E = 3
    params = make_params("small", experiment__missions__n_agents=3, **over)
    tr = COMATrainer(params, n_envs=E, philox_seed=SEED, first_episode=FIRST, team_sizes=teams)
    if layout == "1":
        assert tr.env.tiled
    if over:
        assert tr.env.d.prior == 0.3
    episodes = list(range(FIRST, FIRST + E))
    actions = None
    if policy == "actor":
        tr.actor = StubActor()
    if policy == "explicit":      # a fixed valid table: what the random policy flies on these episodes, handed back as plain numbers
        actions = COMATrainer(params, n_envs=E, philox_seed=SEED, first_episode=FIRST).curves_on(episodes, "random")["actions"].cpu().numpy().copy()
        with pytest.raises(ValueError):
            tr.curves_on(episodes, "explicit")
    out = tr.curves_on(episodes, policy, actions=actions)
    if policy == "explicit":
        assert np.array_equal(out["actions"].cpu().numpy(), actions)
    per_env = [params] * E if teams is None else [make_params("small", experiment__missions__n_agents=n, **over) for n in teams]
    # (mixed teams: env e is a run of the oracle with n_agents = teams[e], which reads the first teams[e] columns of the actions)
    assert_curves_match_oracle(out, per_env, E, tr.T)
    with pytest.raises(ValueError):
        tr.curves_on(episodes, "lawnmower")
    if teams is not None:
        with pytest.raises(Exception, match="one team size"):
            tr.curves_on(episodes, "ig")


# ---- curves_on disturbs nothing --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("policy", ["random", "ig"])
def test_curves_on_agrees_with_returns_on(policy):
    from ippmarl.trainer import COMATrainer
    params = make_params("small")
    tr = COMATrainer(params, n_envs=6, philox_seed=SEED, first_episode=5)
    episodes = list(range(40, 46))
    want = tr.returns_on(episodes, policy)
    out = tr.curves_on(episodes, policy)
    assert float(out["episode_return"].mean()) == want["episode_return"]
    assert float(out["absolute_return"].mean()) == want["absolute_return"]
    assert float(out["f1"][:, -1].contiguous().mean()) == want["final_f1"]
    # (returns_on's entropy is ippm_weighted_entropy's float32 form)
    np.testing.assert_allclose(float(out["target_entropy"][:, -1].mean()), want["final_target_entropy"], rtol=1e-4)
    assert int(out["faults"].ne(0).sum()) == want["faults"]


def test_curves_on_leaves_the_trainer_as_it_was():
    """A training rollout after curves_on = one without it (same wave counter, same epsilon, same transitions), and the curves = those
    computed step by step through the clone path (global_map_with_pending + f1_counts), counts exactly."""
    from ippmarl.trainer import COMATrainer
    from ippmarl.vec_env import POLICY_UNIFORM
    params = make_params("small")

    def fresh():
        torch.manual_seed(3)
        return COMATrainer(params, n_envs=4, philox_seed=SEED, first_episode=5)

    a, b = fresh(), fresh()
    episodes = [60, 61, 62, 63]
    out = a.curves_on(episodes, "random")
    assert a.wave == 0 and a.filled == 0 and a.eps == b.eps
    sa, sb = a.rollout("train"), b.rollout("train")
    assert sa == sb and a.wave == b.wave == 1 and a.eps == b.eps and a.filled == b.filled == 1
    for name in ("buf_obs", "buf_state", "buf_action", "buf_mask", "buf_reward"):
        assert torch.equal(getattr(a, name)[0], getattr(b, name)[0]), name
    # the clone path, per step, on the other trainer
    env = b.env
    env.reset(torch.as_tensor(episodes, dtype=torch.int64))
    thresholds = (DELTA, 0.0, -DELTA)
    ents, counts = [b.map_metrics()[0]], [torch.stack([b.f1_counts(None, thr) for thr in thresholds], 1)]
    for t in range(b.T):
        env.build_observations(t, features=False)
        env.steps(t, policy=POLICY_UNIFORM, features=False)
        pending = b.global_map_with_pending()
        ents.append(b.map_metrics(pending)[0])
        counts.append(torch.stack([b.f1_counts(pending, thr) for thr in thresholds], 1))
    assert torch.equal(out["f1_counts"], torch.stack(counts, 1))
    np.testing.assert_allclose(out["target_entropy"].cpu().numpy(), torch.stack(ents, 1).cpu().numpy(), rtol=1e-4, atol=0)


def test_score_maps_on_env_tensors():
    """VecEnv.score_maps: the global maps by default, the local maps (N maps per truth plane), and a copy; its derived figures."""
    from ippmarl.vec_env import VecEnv, POLICY_UNIFORM
    params = make_params("small")
    env = VecEnv(params, 3, philox_seed=SEED)
    d = O.Derived(params)
    env.reset([7, 8, 9])
    for t in range(3):
        env.build_observations(t, features=False)
        env.steps(t, policy=POLICY_UNIFORM, features=False)
    truth = env.truth_map.numpy()
    g = env.score_maps()
    loc = env.score_maps(env.local)
    assert g.entropy_sum.shape == (3,) and g.counts.shape == (3, 3, 3) and loc.entropy_sum.shape == (12,) and loc.counts.shape == (12, 3, 3)
    glob = env.posterior_global().cpu().numpy().astype(np.float64)
    local = env.posterior_local().cpu().numpy().astype(np.float64)
    for e in range(3):
        np.testing.assert_allclose(float(g.target_entropy[e]), O.target_entropy(d, glob[e].copy(), truth[e].astype(np.float64)), rtol=RTOL)
        assert tuple(g.counts[e, 0].tolist()) == O.f1_counts(glob[e], truth[e], DELTA)
        for i in range(4):
            np.testing.assert_allclose(float(loc.target_entropy[4 * e + i]), O.target_entropy(d, local[e, i].copy(), truth[e].astype(np.float64)),
                                       rtol=RTOL)
            assert tuple(loc.counts[4 * e + i, 2].tolist()) == O.f1_counts(local[e, i], truth[e], -DELTA)
    tp, fp, fn = (g.counts[:, 1, k].double() for k in range(3))
    assert torch.equal(g.target_entropy, g.entropy_sum / (tp + fn)) and torch.equal(g.f1, 2 * tp / (2 * tp + fp + fn))
    again = env.score_maps(env.glob.clone(), delta=DELTA)
    assert torch.equal(again.entropy_sum, g.entropy_sum) and torch.equal(again.counts, g.counts)
    with pytest.raises(ValueError):
        env.score_maps(env.glob[:2])
