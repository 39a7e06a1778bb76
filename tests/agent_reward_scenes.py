"""Constructed scenes for k_agent_rewards (csrc/agent_rewards.hip, ippm_agent_rewards): the DeepQ per-agent reward on inputs an
episode never flies.  Plain module: tests/test_agent_reward_scenes_cpu.py (census, proofs) and tests/test_hip_agent_rewards_constructed.py
(the device) import the same scenes and the same references.

The reference (sums_ref): for agent i, in float64 log-odds, a = clip(K, +-lc) + (lm[bit] - logit(prior)) inside its footprint and
clip(K) - logit(prior) outside, then the oracle's own reward arithmetic on sigmoid(K), sigmoid(a) (O.shannon_entropy, O.class_weights:
what O.reward_sums does, for all agents of an env at once) and rewards_of.  Pinned to the oracle's DeepQ path by a CPU test.

Three kinds of scene sets:
  A1  the scene sets of tests/test_hip_constructed_rects.py (make_scenes, Sim, Runner), one more check per step; two more grids here
      (AR_GRIDS: prior 0.3 on the 34- and on a 128-cell grid);
  A2  value sets ("values128", "values_nf"): one fixed mid-grid footprint whose cells and a ring around it take classes of K -- 0, the
      class-weight threshold and the clip with their float32 neighbours, values a deferred clamp leaves (+-2 lc, +-1e30, +-inf on the
      noise-free configuration), and +-wt - lm so that a lands on and beside the threshold -- under both bits and every altitude;
  A3  geometry sets: footprints of every alignment, thin ones, ones at the borders, the contract's largest, empty ones, over a smooth
      map that differs from env to env.
A set is a DirectSet: what the caller of ippm_agent_rewards writes (K, code tiles, sense records) plus the float64 reference and the
host model of the device code (model_agent: the float32 restatement, and the one-line changes the census must be able to see)."""
import contextlib
import functools

import numpy as np

import test_hip_constructed_rects as R
import ipp_oracle as O
from configs import make_params

RTOL = R.RTOL
EMPTY = R.EMPTY
F32 = np.float32

# two more grids for A1, in the format of test_hip_constructed_rects.GRIDS: (how the params are made, shifts, steps, random scenes)
AR_GRIDS = {
    # one cell per lane AND the whole-grid walk: k_agent_rewards<1, true, false>; 34 x 34 = 1156 items, the item loop runs twice
    "34p": (("set", "default", dict(sensor__pixel__number_x=4, sensor__pixel__number_y=4, mapping__prior=0.3)), [(0, 0), (1, 2), (2, 0), (3, 2)], 2, 8),
    # 128 x 32 groups = 4096 items: the item loop of the SHIFT path runs four times (the 48p grid stays below 1024)
    "128p": (("set", "small", dict(mapping__prior=0.3)), [(1, 2)], 2, 4),
}


@contextlib.contextmanager
def _registered(grid):
    """test_hip_constructed_rects.geom builds a Geom from its GRIDS table and caches it; the entry is lent to the table for the one
    call that builds it (the table is as it was afterwards; every later geom(grid) is answered from the cache)."""
    R.GRIDS[grid] = AR_GRIDS[grid]
    try:
        yield
    finally:
        del R.GRIDS[grid]


def geom(grid):
    """(Depends on R.geom being an lru_cache over a lookup in R.GRIDS, and on this function being the first to ask for a grid of
    AR_GRIDS: every user of the new grids -- grid(), a1_reference, the GPU test's RewardRunner -- calls it before R.geom / R.make_scenes /
    R.Sim / R.Runner see the name.)"""
    if grid in AR_GRIDS and grid not in R.GRIDS:
        with _registered(grid):
            return R.geom(grid)
    return R.geom(grid)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference and the restatement, for the agents of one env at once
# ---------------------------------------------------------------------------------------------------------------------------------
def after_maps(g, K, rects, bits, lm):
    """float64 [n, gx, gy]: a_i of every agent.  K log-odds [gx, gy]; rects [n, 4] = [yu, yd, xl, xr]; bits[i] uint8 [h, w];
    lm [n, 2]: the measurement's log-odds (not yet minus logit(prior))."""
    K = np.asarray(K, dtype=np.float64)
    base = np.clip(K, -g.lc, g.lc) - g.lp
    A = np.repeat(base[None], len(rects), axis=0)
    for i, (yu, yd, xl, xr) in enumerate(np.asarray(rects, dtype=np.int64)):
        if xr > xl and yd > yu:
            A[i, xl:xr, yu:yd] += np.where(np.asarray(bits[i]) != 0, np.float64(lm[i][1]), np.float64(lm[i][0]))
    return A


def sums_ref(g, K, rects, bits, lm):
    """-> (S [n, 2] = (S1_i, S2_i), T = sum w(K) H(K)) in float64 by the oracle's arithmetic (O.reward_sums per agent, vectorised)."""
    K = np.asarray(K, dtype=np.float64)
    pk = R._sigmoid(K)
    wk = O.class_weights(pk)
    hb = O.shannon_entropy(pk.copy())
    pa = R._sigmoid(after_maps(g, K, rects, bits, lm))
    w = O.class_weights(pa)
    ha = O.shannon_entropy(pa)
    return np.stack([np.sum(w * (hb[None] - ha), axis=(1, 2)), np.sum(w * hb[None], axis=(1, 2))], axis=1), float(np.sum(wk * hb))


def rewards_of(g, s1, s2):
    """R.rewards_of on arrays, with the oracle's 0 / 0 = nan (utils/reward.py divides NumPy floats)."""
    s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 22.0 * (s1 / s2) - 0.5, 10.0 * (s1 / (g.gx * g.gy)) - 0.17


def lm_record(g, lm):
    """The two floats of a sense record: measurement log-odds minus logit(prior), formed in float32 as the plan kernel forms them."""
    return (np.asarray(lm, dtype=F32) - F32(g.lp)).astype(F32)


def weight32(L, wt, ge=False):
    """ippm_weight_l on float32 log-odds."""
    L = np.asarray(L, dtype=F32)
    up = (L >= F32(wt)) if ge else (L > F32(wt))
    return np.where(up, F32(1), np.where(L < -F32(wt), F32(0), F32(0.5))).astype(F32)


def entropy32(L, lc):
    """ippm_entropy_l in float32 NumPy (R.reward_sums' restatement)."""
    one = F32(1)
    a = np.minimum(np.abs(np.asarray(L, dtype=F32)), F32(lc)).astype(F32)
    ex = np.exp(-a).astype(F32)
    return (np.log2(one + ex) + (a * F32(1.44269504)) * (ex / (one + ex))).astype(F32)


def entropy64(L, lc):
    """entropy_l_f64: the SHIFT path's entropy of a float32 log-odds value."""
    a = np.minimum(np.abs(np.asarray(L, dtype=np.float64)), np.float64(F32(lc)))
    ex = np.exp(-a)
    return np.log2(1.0 + ex) + a * 1.4426950408889634 * (ex / (1.0 + ex))


def weighted_entropy32(g, K32):
    """T as the restatement has it: float32 per-cell terms of w(K) H(K), summed in float64 (float64 entropies on the SHIFT path)."""
    w = weight32(K32, g.d.logit_weight_thr)
    if g.shift:
        return float(np.sum(w.astype(np.float64) * entropy64(K32, g.lc)))
    return float(np.sum((w * entropy32(K32, g.lc)).astype(np.float64)))


# ---------------------------------------------------------------------------------------------------------------------------------
# host model of the device code
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("clip dropped", "weight from K", "ge at wt", "code column off", "tile alignment dropped", "T left out", "lm swapped",
             "row bound inclusive")


def items_of(g, rect, tiled):
    """The kernel's item count for a footprint (csrc/agent_rewards.hip: xa .. items)."""
    yu, yd, xl, xr = (int(v) for v in rect)
    vec, fp = g.d.vec, xr > xl and yd > yu
    xa, xb = (0, g.gx) if g.shift else ((xl, xr) if fp else (0, 0))
    ya, yb = (0, g.gy) if g.shift else (yu, yd)
    y0 = ya & ~(vec - 1)
    groups = (yb - y0 + vec - 1) // vec if xb > xa else 0
    x0 = (xa & ~3) if tiled else xa
    rows = xb - x0
    return (((rows + 3) >> 2) * groups * 4) if tiled else rows * groups


def instantiation(g, tiled):
    return "k_agent_rewards<%d, %s, %s>" % (g.d.vec, str(bool(g.shift)).lower(), str(bool(tiled)).lower())


def model_bits(g, rect, tile, col_off=0, drop_align=False):
    """The measurement bits the kernel reads for the cells of a footprint, through tile_index(x - xl, y - (yu & ~3), S) and a byte
    load that returns 0 outside the tile.  col_off: the byte one group column further; drop_align: y - yu in place of y - (yu & ~3)."""
    yu, yd, xl, xr = (int(v) for v in rect)
    S, vec = g.d.tile_stride, g.d.vec
    tile = np.asarray(tile, dtype=np.uint8)
    ys, row = np.arange(yu, yd), np.arange(xr - xl)[:, None]
    ygrp = ys & ~(vec - 1)                                   # first column of the lane's group: y0 + g VEC, y0 = yu & ~(VEC - 1)
    col = ygrp - (yu if drop_align else (yu & ~3))
    if vec == 4:
        idx = row * (S >> 2) + ((col >> 2) + col_off)[None, :]
        shift = (ys - ygrp)[None, :]
    else:
        idx = row * S + (col + col_off)[None, :]
        shift = np.zeros((1, len(ys)), dtype=np.int64)
    ok = (idx >= 0) & (idx < tile.size)
    byte = np.where(ok, tile[np.clip(idx, 0, tile.size - 1)], 0).astype(np.int64)
    return ((byte >> shift) & 1).astype(np.uint8)


def model_agent(g, K32, rect, tile, lmrec, T, mutate=None):
    """(S1, S2) of one agent as the device code computes them, vectorised over the cells it walks: float32 per-cell terms summed in
    float64 (prior 0.5), the float64 chain rounded once and float64 entropies (SHIFT).  `mutate`: one of MUTATIONS."""
    yu, yd, xl, xr = (int(v) for v in rect)
    lc, wt = F32(g.lc), g.d.logit_weight_thr
    fp = xr > xl and yd > yu
    lm0, lm1 = (F32(lmrec[1]), F32(lmrec[0])) if mutate == "lm swapped" else (F32(lmrec[0]), F32(lmrec[1]))
    ge = mutate == "ge at wt"
    t_in = 0.0 if mutate == "T left out" else float(T)
    # ("row bound inclusive": the row x = xb is loaded, but `rowin` keeps it out of the footprint and, SHIFT, it < items keeps it out of
    #  the grid: its weights are 0 either way -- the change alters no value, see profiles/r22/README.md)
    if not fp and not g.shift:
        return 0.0, t_in
    sel = None
    if fp:
        bits = model_bits(g, rect, tile, col_off=1 if mutate == "code column off" else 0, drop_align=mutate == "tile alignment dropped")
        sel = np.where(bits != 0, lm1, lm0).astype(F32)
    if g.shift:
        b = np.asarray(K32, dtype=F32)
        kc = b.astype(np.float64) if mutate == "clip dropped" else np.clip(b.astype(np.float64), -np.float64(lc), np.float64(lc))
        a64 = kc - g.lp
        if fp:
            a64[xl:xr, yu:yd] = kc[xl:xr, yu:yd] + sel.astype(np.float64)
        with np.errstate(over="ignore"):
            a = a64.astype(F32)
        wb = weight32(b, wt, ge).astype(np.float64)
        wa = wb if mutate == "weight from K" else weight32(a, wt, ge).astype(np.float64)
        hb, ha = entropy64(b, lc), entropy64(a, lc)
        return float(np.sum(wa * (hb - ha))), t_in + float(np.sum((wa - wb) * hb))
    b = np.asarray(K32, dtype=F32)[xl:xr, yu:yd]
    with np.errstate(invalid="ignore", over="ignore"):
        a = ((b if mutate == "clip dropped" else np.clip(b, -lc, lc)) + sel).astype(F32)
    wb = weight32(b, wt, ge)
    wa = wb if mutate == "weight from K" else weight32(a, wt, ge)
    hb, ha = entropy32(b, lc), entropy32(a, lc)
    return float(np.sum((wa * (hb - ha)).astype(np.float64))), t_in + float(np.sum(((wa - wb) * hb).astype(np.float64)))


# ---------------------------------------------------------------------------------------------------------------------------------
# grids of the direct-call sets
# ---------------------------------------------------------------------------------------------------------------------------------
class Grid:
    """What the references need of a configuration (the members of test_hip_constructed_rects.Geom they read)."""

    def __init__(self, name, params):
        from ippmarl.derived import DerivedConstants
        self.grid, self.params = name, params
        self.d = d = DerivedConstants(params, philox_seed=R.SEED)
        self.o = O.Derived(params)
        self.o.exact = True
        self.N = d.n_agents
        self.gx, self.gy = d.grid_x, d.grid_y
        self.hmax, self.wmax = min(2 * max(d.radius_x), self.gx - 1), min(2 * max(d.radius_y), self.gy - 1)
        self.lc, self.lp = d.logit_clip, d.logit_prior
        self.shift = d.prior != 0.5
        self.lm = np.asarray(d.logit_meas, dtype=F32)
        self.tiles_ok = (not self.shift) and d.vec == 4 and self.gx % 4 == 0 and self.gy % 8 == 0


@functools.lru_cache(maxsize=None)
def grid(name):
    if name in R.GRIDS or name in AR_GRIDS:
        return Grid(name, geom(name).params)
    if name == "204":       # the smallest multiple-of-4 grid whose largest footprint takes more than 1024 items: 72 rows x 19 groups
        return Grid(name, make_params("small", **R._TEAM, sensor__pixel__number_x=24, sensor__pixel__number_y=24))
    if name == "256":       # config 2's grid: 90 rows x 24 groups, more than 2048 items
        return Grid(name, make_params("c2", **R._TEAM))
    if name == "nf42":      # the noise-free configuration of test_hip_deepq.py (a 42-cell grid): 20 m measures with log-odds -inf / +inf
        from test_hip_deepq import NOISE_FREE
        return Grid(name, make_params("small", **dict(R._TEAM, **NOISE_FREE)))
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------------------------
# a set of direct-call scenes
# ---------------------------------------------------------------------------------------------------------------------------------
def smooth_map(g, e):
    """A smooth map that is different in every env: crosses both class-weight thresholds and both clips (values up to 1.5 lc)."""
    x, y = np.arange(g.gx, dtype=np.float64)[:, None], np.arange(g.gy, dtype=np.float64)[None, :]
    K = 1.1 * g.lc * np.sin(0.213 * x + 0.37 * e + 0.5) * np.cos(0.171 * y - 0.113 * e) + 0.4 * g.lc * np.sin(0.0531 * (x + 2.0 * y) + 0.7 * e)
    return K.astype(F32)


class DirectSet:
    """E envs of N agents for direct calls of ippm_agent_rewards: K [E, gx, gy] float32 log-odds, rects [E, N, 4], bits[e][i] uint8
    [h, w], lm [E, N, 2] float32 measurement log-odds, tags[e][i]."""

    def __init__(self, name, g, K, rects, bits, lm, tags):
        self.name, self.g = name, g
        self.K = np.ascontiguousarray(K, dtype=F32)
        self.rects = np.asarray(rects, dtype=np.int64)
        self.bits, self.tags = bits, tags
        self.lm = np.asarray(lm, dtype=F32)
        self.E, self.N = self.rects.shape[:2]
        assert self.N == g.N and self.K.shape == (self.E, g.gx, g.gy) and self.lm.shape == (self.E, self.N, 2)
        for e in range(self.E):
            for i in range(self.N):
                r = self.rects[e, i]
                R.check_rect(g, r, "footprint" if R._some(r) else "empty")
                assert np.asarray(bits[e][i]).shape == (r[3] - r[2], r[1] - r[0])

    @functools.cached_property
    def code(self):
        out = np.zeros((self.E, self.N, self.g.d.tile_bytes), dtype=np.uint8)
        for e in range(self.E):
            for i in range(self.N):
                if R._some(self.rects[e, i]):
                    out[e, i] = self.g.d.pack_tile(self.rects[e, i], self.bits[e][i])
        return out

    @functools.cached_property
    def cell_mask(self):
        """Code tiles with every bit set that belongs to a footprint cell (the bits a stale tile must not disturb)."""
        out = np.zeros_like(self.code)
        for e in range(self.E):
            for i in range(self.N):
                r = self.rects[e, i]
                if R._some(r):
                    out[e, i] = self.g.d.pack_tile(r, np.ones((r[3] - r[2], r[1] - r[0]), dtype=np.uint8))
        return out

    def stale_code(self, fill):
        """The code tiles with every byte and bit outside the footprints' cells replaced: fill = 0xFF, or a seed for random bytes."""
        junk = np.full_like(self.code, 0xFF) if fill == 0xFF else np.random.RandomState(fill).randint(0, 256, size=self.code.shape).astype(np.uint8)
        return ((junk & ~self.cell_mask) | self.code).astype(np.uint8)

    @functools.cached_property
    def records(self):
        rec = np.zeros((self.E, self.N, 8), dtype=np.int32)
        rec[..., 0:4] = self.rects
        rec[..., 4:6] = lm_record(self.g, self.lm).view(np.int32)
        return rec

    @functools.cached_property
    def ref(self):
        """float64: S [E, N, 2] with the reference's own T, T [E], D = S2 - T [E, N] (what a caller's T is added to)."""
        S, T = np.zeros((self.E, self.N, 2)), np.zeros(self.E)
        for e in range(self.E):
            S[e], T[e] = sums_ref(self.g, self.K[e], self.rects[e], self.bits[e], self.lm[e])
        return dict(S=S, T=T, D=S[..., 1] - T[:, None])

    def model(self, mutate=None, T=None):
        """The host model: S [E, N, 2] for T [E] (default: the restatement's own weighted entropy of K)."""
        T = self.model_T if T is None else np.broadcast_to(np.asarray(T, dtype=np.float64), (self.E,))
        rec = lm_record(self.g, self.lm)
        S = np.zeros((self.E, self.N, 2))
        for e in range(self.E):
            for i in range(self.N):
                S[e, i] = model_agent(self.g, self.K[e], self.rects[e, i], self.code[e, i], rec[e, i], T[e], mutate)
        return S

    @functools.cached_property
    def model_T(self):
        return np.array([weighted_entropy32(self.g, self.K[e]) for e in range(self.E)])

    @functools.cached_property
    def restated(self):
        return self.model()

    @functools.cached_property
    def weighted_cells(self):
        """[E, N]: cells whose class weight is not 0 before or after (the cells that carry an entropy error into the sums)."""
        wt = self.g.d.logit_weight_thr
        out = np.zeros((self.E, self.N), dtype=np.int64)
        for e in range(self.E):
            A = after_maps(self.g, self.K[e], self.rects[e], self.bits[e], self.lm[e])
            wk = weight32(self.K[e], wt) != 0
            for i in range(self.N):
                yu, yd, xl, xr = self.rects[e, i]
                m = (weight32(A[i], wt) != 0) | wk
                out[e, i] = int(m.sum()) if self.g.shift else int(m[xl:xr, yu:yd].sum())
        return out

    def bound(self, S):
        """The project's bound on (S1_i, S2_i) -- rtol 1e-5 beside sums_atol of S2 (check_deepq_batch, _check_env_step) -- for
        reference sums S [.., 2]: [.., 2]."""
        S = np.asarray(S, dtype=np.float64)
        atol = np.vectorize(lambda s2: R.sums_atol(self.g, s2))(S[..., 1])
        return RTOL * np.abs(S) + atol[..., None]


def _pad(g, agents, filler=None):
    """Groups (tag, rect, level, bit pattern) agents into envs of N; the last env is filled up with empty footprints (prior 0.5) or `filler`."""
    agents = list(agents)
    while len(agents) % g.N:
        agents.append(("pad", filler if filler is not None else EMPTY, 0, 0))
    return [agents[k:k + g.N] for k in range(0, len(agents), g.N)]


def _bits(rect, pattern, seed):
    yu, yd, xl, xr = rect
    h, w = xr - xl, yd - yu
    if pattern == "ones":
        return np.ones((h, w), dtype=np.uint8)
    if pattern == "zeros":
        return np.zeros((h, w), dtype=np.uint8)
    if pattern in ("checker", "inverse"):
        c = ((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1).astype(np.uint8)
        return c if pattern == "checker" else (1 - c).astype(np.uint8)
    return np.random.RandomState(seed).randint(0, 2, size=(h, w)).astype(np.uint8)


def _build(name, g, envs, K):
    """envs: lists of N (tag, rect, altitude level, bit pattern)."""
    rects = np.array([[a[1] for a in env] for env in envs], dtype=np.int64)
    lm = np.array([[g.lm[a[2] % len(g.lm)] for a in env] for env in envs], dtype=F32)
    bits = [[_bits(a[1], a[3], 977 * e + i) for i, a in enumerate(env)] for e, env in enumerate(envs)]
    tags = [[a[0] for a in env] for env in envs]
    return DirectSet(name, g, K, rects, bits, lm, tags)


# ---- A3: geometry --------------------------------------------------------------------------------------------------------------
def _filler(g):
    return (g.gy - 5, g.gy - 2, g.gx - 4, g.gx - 2)


def geometry_agents(g, full):
    """(tag, rect, level, pattern) of a geometry set.  full: every alignment combination, thin and border footprints (the small grids);
    otherwise the contract's largest footprint at four shifts and at the far corner, and the rest at one shift."""
    out = []
    n = 0

    def add(tag, rect):
        nonlocal n
        out.append((tag, tuple(int(v) for v in rect), n % 3, "random"))
        n += 1

    if full:
        # every (yu % 8, yd % 4) x (xl % 4, xr % 4): 5 .. 8 cells wide and tall
        for a in range(8):
            for yd4 in range(4):
                for b in range(4):
                    for xr4 in range(4):
                        yu, xl = 8 + a, 8 + b
                        w, h = 5 + (yd4 - (yu + 5)) % 4, 5 + (xr4 - (xl + 5)) % 4
                        add("align", (yu, yu + w, xl, xl + h))
    for h in (1, 2, 3):
        for w in (1, 2, 3):
            for k in (range(4) if full else (1,)):
                add("thin", (9 + k, 9 + k + w, 6 + k, 6 + k + h))
                add("thin", (5 + k, 5 + k + w, 3, 3 + min(g.hmax, 9)))            # thin across a tall one's rows ...
                add("thin", (3, 3 + min(g.wmax, 9), 7 + k, 7 + k + h))            # ... and along a wide one's columns
    sy, sx = min(g.wmax, 7), min(g.hmax, 6)
    for k in (range(4) if full else (2,)):
        add("border", (0, sy + k, 0, sx))
        add("border", (g.gy - 1 - sy - k, g.gy - 1, g.gx - 1 - sx, g.gx - 1))
        add("border", (0, sy, g.gx - 2 - k, g.gx - 1))
        add("border", (g.gy - 2 - k, g.gy - 1, 0, sx + k))
        add("border", (0, g.wmax, 5 + k, 7 + 2 * k))
        add("border", (g.gy - 1 - g.wmax, g.gy - 1, g.gx - 1 - g.hmax, g.gx - 1))
    for dy, dx in ((0, 0), (1, 2), (2, 3), (3, 1)):
        add("largest", (2 + dy, 2 + dy + g.wmax, 1 + dx, 1 + dx + g.hmax))
    # (prior != 0.5 too: the kernel then walks the whole grid with a = clip(K) - logit(prior), as after_maps has it)
    for r in (EMPTY, (4, 9, 6, 6), (5, 5, 3, 9)):
        add("empty", r)
        add("empty", r)
    return out


GEOMETRY = {"48": True, "46": True, "34": True, "48p": True, "34p": True, "204": False, "256": False}


@functools.lru_cache(maxsize=None)
def geometry_set(name):
    """The geometry set of a grid; its first scene is repeated in the middle and at the end of the batch (the e / ei indexing)."""
    g = grid(name)
    envs = _pad(g, geometry_agents(g, GEOMETRY[name]), _filler(g) if g.shift else None)
    first = envs[0]
    envs = envs + [first]
    envs.insert(len(envs) // 2, first)
    copies = [k for k, env in enumerate(envs) if env is first]
    assert len(copies) == 3 and copies[0] == 0 and copies[-1] == len(envs) - 1
    K = np.stack([smooth_map(g, e) for e in range(len(envs))])
    for k in copies[1:]:
        K[k] = K[0]
    ds = _build("geometry_" + name, g, envs, K)
    for k in copies[1:]:      # the same scene: the same measurement bits too
        ds.bits[k] = ds.bits[0]
    ds.copies = copies
    return ds


def team_sizes(ds):
    """n_active [E] for the switched-off-agents run: 1 .. N flying agents, in turn (ippm_set_team_sizes)."""
    return np.array([1 + (3 * e) % ds.N for e in range(ds.E)], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def free_set():
    """An all-free map (every weight 0 before and after) with T = 0: S1 = S2 = 0, the oracle's 0 / 0."""
    g = grid("48")
    env = [("free", (10 + i, 18 + i, 9, 20), 0, "zeros") for i in range(g.N)]
    return _build("free_48", g, [env], np.full((1, g.gx, g.gy), -5.0, dtype=F32))


# ---- A2: values ----------------------------------------------------------------------------------------------------------------
def _step(v, k):
    """The float32 k ulps away from v (k < 0: towards -inf)."""
    v = F32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf if k > 0 else -np.inf), dtype=F32)
    return v


def ref_weight(L64):
    """The reference's class weight of a float64 log-odds value: on the probability, 0.499 / 0.501 and np.round (O.class_weights)."""
    L64 = np.asarray(L64, dtype=np.float64)
    return O.class_weights(R._sigmoid(np.atleast_1d(L64))).reshape(L64.shape)


def agrees(g, K, lmrec=None):
    """Does the float32 log-odds rule give the reference's class weight -- for K itself (lmrec None) or for a = clip(K) + lmrec?"""
    K = F32(K)
    if lmrec is None:
        return float(weight32(K, g.d.logit_weight_thr)) == float(ref_weight(np.float64(K)))
    kc = np.clip(K, -F32(g.lc), F32(g.lc))
    a32 = F32(kc + F32(lmrec))
    a64 = np.float64(np.clip(np.float64(K), -g.lc, g.lc)) + np.float64(lmrec)      # (lmrec: prior 0.5 here, the record is the log-odds)
    return float(weight32(a32, g.d.logit_weight_thr)) == float(ref_weight(a64))


@functools.lru_cache(maxsize=None)
def value_classes(name):
    """label -> float32 K, and the record of how far each threshold neighbour had to step: [(label, side, ulps)].
    Around +-wt (for K itself) and around +-wt - lm (for a = K + lm of that altitude and bit) the values are the nearest float32 on
    either side on which the float32 rule and the reference's probability rule agree, and the value itself if they agree on it."""
    g = grid(name)
    wt, lc = F32(g.d.logit_weight_thr), F32(g.lc)
    vals, steps = {"0": F32(0)}, []

    def around(label, centre, lmrec):
        centre = F32(centre)
        if agrees(g, centre, lmrec):
            vals[label] = centre
        steps.append((label, "on", 0 if agrees(g, centre, lmrec) else None))
        for side, name_ in ((-1, "-"), (1, "+")):
            k = 1
            while not agrees(g, _step(centre, side * k), lmrec):
                k += 1
            vals[label + name_] = _step(centre, side * k)
            steps.append((label, name_, k))

    for sg, sn in ((1, "+"), (-1, "-")):
        around(sn + "wt", sg * wt, None)
        for k in (-1, 0, 1):
            vals[f"{sn}lc{k:+d}"] = _step(sg * lc, k)
        vals[sn + "2lc"] = F32(sg * 2) * lc
        vals[sn + "1e30"] = F32(sg * 1e30)
        if name == "nf42":
            vals[sn + "inf"] = F32(sg * np.inf)
    for lvl, pair in enumerate(g.lm):
        for b, l in enumerate(pair):
            if np.isfinite(l):
                for sg, sn in ((1, "+"), (-1, "-")):
                    around(f"{sn}wt-lm{lvl}{b}", F32(sg * wt - l), l)
    return vals, steps


# the fixed footprint [yu, yd, xl, xr] of the value sets: 16 rows x 18 columns, yu % 4 = 1, yd % 4 = 3 (128 cells); 12 x 14 (42 cells)
FOOT = {"128": (49, 67, 54, 70), "nf42": (13, 27, 15, 27)}
RING = 1


@functools.lru_cache(maxsize=None)
def value_set(name):
    """"values128": the three altitudes of the 128-cell grid; "values_nf": the noise-free configuration (42 cells, one cell per lane; 15 m and 20 m, +-inf)."""
    g = grid("128" if name == "values128" else "nf42")
    vals, _ = value_classes(g.grid)
    labels = sorted(vals)
    foot = FOOT[g.grid]
    yu, yd, xl, xr = foot
    levels = len(g.lm)
    pats = [(lvl, p) for lvl in range(levels) for p in ("checker", "inverse")]
    pats += [(0, "ones"), (levels - 1, "zeros"), (levels - 1, "ones"), (0, "zeros")]
    env = [(f"values/{lvl}/{p}", foot, lvl, p) for lvl, p in pats[:g.N]]
    E = 6
    K = np.stack([smooth_map(g, e) for e in range(E)])
    label_of = np.full((E, g.gx, g.gy), -1, dtype=np.int64)
    box = [(x, y) for x in range(xl - RING, xr + RING) for y in range(yu - RING, yd + RING)]
    for e in range(E):
        for n, (x, y) in enumerate(box):
            k = (n * 7 + 13 * e) % len(labels)       # 7 is coprime to the number of labels' usual counts; the census checks the coverage
            K[e, x, y] = vals[labels[k]]
            label_of[e, x, y] = k
    ds = _build(name, g, [env] * E, K)
    ds.labels, ds.label_of = labels, label_of
    return ds


DIRECT_SETS = [("values128", "rows"), ("values128", "tiles"), ("values_nf", "rows")] + \
              [("geometry_" + n, lay) for n in GEOMETRY for lay in (("rows", "tiles") if n in ("48", "256") else ("rows",))]


def direct_set(name):
    if name.startswith("geometry_"):
        return geometry_set(name[len("geometry_"):])
    return free_set() if name == "free_48" else value_set(name)


# the reward tolerances of check_deepq_batch
def reward_tol(rel, ab):
    return RTOL * np.abs(rel) + 1e-6 + RTOL * 0.5, RTOL * np.abs(ab) + 1e-6 + RTOL * 0.17


def reward_cutoff(S):
    """Where the reward is compared with the reference: the sums' bound has an absolute part of 1e-6 that does not shrink with S2; it
    reaches 22 S1 / S2 as 22 * 1e-6 * (1 + |S1 / S2|) / |S2|, which stays inside the rewards' own absolute 1e-6 only for
    |S2| >= 22 (1 + |S1 / S2|).  Below that the reward is checked against the device's own sums alone."""
    S = np.asarray(S, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(S[..., 1]) >= 22.0 * (1.0 + np.abs(S[..., 0] / S[..., 1]))


# ---------------------------------------------------------------------------------------------------------------------------------
# A1: the reference of a step of the scene sets of test_hip_constructed_rects
# ---------------------------------------------------------------------------------------------------------------------------------
A1_FORMS = [("48", "rows"), ("48", "tiles"), ("46", "rows"), ("128", "rows"), ("34", "rows"), ("48p", "rows"), ("128x512", "tiles"),
            ("34p", "rows"), ("128p", "rows")]


def a1_step_reference(g, sim, t, obs, dtype=np.float64):
    """After sim.fuse(t) and obs = sim.sense(t): S [E, N, 2] and T [E] of the agents' new footprints rects[t + 1] over the global map
    the fusion of step t left, in float64 (the reference) or in the restatement's arithmetic (dtype float32, from a float32 Sim)."""
    E = sim.E
    S, T = np.zeros((E, R.N, 2)), np.zeros(E)
    for e, sc in enumerate(sim.scenes):
        rects = sc["rects"][t + 1]
        lm = np.asarray(g.d.logit_meas, dtype=F32)[sc["alts"][t + 1]]
        if dtype == np.float64:
            S[e], T[e] = sums_ref(g, sim.glob[e], rects, obs[e], lm)
        else:
            K32 = sim.glob[e].astype(F32)
            T[e] = weighted_entropy32(g, K32)
            rec = lm_record(g, lm)
            for i in range(R.N):
                tile = g.d.pack_tile(rects[i], obs[e][i]) if R._some(rects[i]) else np.zeros(g.d.tile_bytes, dtype=np.uint8)
                S[e, i] = model_agent(g, K32, rects[i], tile, rec[i], T[e])
    return S, T


@functools.lru_cache(maxsize=None)
def a1_reference(grid, restated=False, stride=1):
    """Per step (S [E, N, 2], T [E]) of every `stride`-th scene of a grid: the float64 reference, or the restatement on a float32 Sim."""
    g = geom(grid)
    scenes = R.make_scenes(grid)[::stride]
    dtype = np.float32 if restated else np.float64
    sim = R.Sim(grid, dtype, scenes=scenes)
    out = []
    for t in range(g.steps):
        sim.fuse(t)
        out.append(a1_step_reference(g, sim, t, sim.sense(t), dtype))
    return out
