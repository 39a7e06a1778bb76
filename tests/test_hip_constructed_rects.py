"""The map kernels -- K3 (sense and update), the plan kernel's tile-item builder, the tile fusion, the row walker -- on CONSTRUCTED
rectangles (include/ippmarl.h: ippm_plan_step / ippm_fuse_step / ippm_sense_step, ippm_fuse_local / ippm_fuse_global_reward).

Every other parity test feeds these kernels the footprints an episode flies: an 11-point lattice times three altitudes, 33 column
intervals per axis and grid, 7 - 11 of the 16 (first column % 4, end column % 4) pairs, no two footprints that abut, none closer
than a 4-cell group on the 512-wide grids.  Nothing in the C-ABI ties the kernels to such rectangles: ippm_plan_step reads `rect`
from the caller, ippm_sense_step the sense records, the deferred-clamp state is six words of `ws`.  Here a SCENE is one env whose
eight agents publish hand-made rectangles [yu, yd, xl, xr] with hand-made measurement bits, altitudes, a directed comm matrix,
initial maps and initial deferred-clamp state, stepped two or three times through the env's own members (reset, build_observations,
_sense from sense records), so that what one fusion leaves unclamped is carried into the next.  All scenes of a grid are the envs
of ONE VecEnv.  The reference is the literal recursion of mappings.py:82-124 in float64 log-odds (Sim below; pinned to
O.fuse_map / O.bayes_update by a CPU test).

Scene families (make_scenes): (a) two and three rectangles side by side, gaps of 0 .. 5 cells starting at every position of a
group, along columns and along rows; (b) nested, identical, partially overlapping and disjoint rectangles in every op order, the
outer one of the largest size the contract admits; (c) rectangles 1, 2, 3 cells wide or tall, alone and across another; (d)
rectangles against row 0 / column 0 and ending at grid_x - 1 / grid_y - 1 (46 wide: the overhanging group); (e) eight DIFFERENT
rectangles around one core plus the two clamp-only ops: nine ops, every item with its own mask; (f) clamp-only ops -- WS_FLAG_A
with a box larger than a footprint, disjoint from and overlapping the messages, WS_FLAG_S with and without messages, a map that
hears nobody for one or two steps (the box grows) and then receives; (g) empty rectangles as sources, as the last source and as
the only ones; (h) seeded random scenes.  Each family is laid out at every (dy, dw) shift of ALIGNS[grid]; the sensing of a step
takes the published rectangles one agent further, so K3 meets every rectangle too and every later fusion another op order.

What the scene sets reach (counted by the host model of the plan kernel below, test_scene_sets_reach_what_they_claim; "gaps":
(gap, gap start % 4) pairs of side-by-side ops of one slab out of 24, "masks": distinct op masks of tile items, "7+": items met
by seven or more ops):

    grid      scenes steps  (yu%4,yd%4)  column gaps  row gaps  masks  7+     forms (layout / area sums)
    48          379    3      16 / 16      24 / 24    24 / 24    326   yes    rows, tiles / untracked, tracked: k_fuse_tiles, k_sense_tiles<4>
    46          379    3      16 / 16      24 / 24    24 / 24    328   yes    rows (rows 4-byte aligned: the MIS instantiations)
    34          379    3      16 / 16      24 / 24    24 / 24    371   yes    rows: one cell per lane, k_fuse_rows<1>, k_sense_update (tracked)
    48p         376    3      16 / 16      24 / 24    24 / 24    413   yes    prior 0.3: k_fuse_rows<4, .., true> (SHIFT), float64 chain
    128         127    2      16 / 16      24 / 24    24 / 24    200   yes    rows: three altitudes, three pairs of measurement log-odds
    128x512      77    2      16 / 16      24 / 24    11 / 24    248   yes    rows (whole-line rounding in the builder and K3), tiles
    256x512      77    2      16 / 16      24 / 24    13 / 24    295   yes    rows: footprint rows of 46 groups, K3 shape (2,2,0), cooperative emission
    204x512      77    2      16 / 16      24 / 24    13 / 24    299   yes    rows: config 5's cells on a 10 m x 25 m world, rows of 91 groups, K3 (4,3,0)

(tile storage adds the rectangles' x % 4 and y % 8: all 4 and all 8 occur on every grid.)  On the 512-wide grids family (a2)
puts eight rectangles side by side with gaps of 0 .. 5 and 33 cells: the rounded intervals of the first seven swallow their
neighbours' gaps (a few hundred plans per grid lose an interval to the rounding), the eighth stays apart.  Prior 0.3 runs without empty rectangles (an agent without a footprint publishes no
message there, include/ippmarl.h: `rect`): fillers take their place and family (g) is left out.
"""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ipp-marl_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ipp_oracle as O  # noqa: E402
from configs import make_params  # noqa: E402
from conftest import assert_posteriors  # noqa: E402

N = 8               # agents of every scene: plans of up to nine ops
SEED = 0xC0457      # Philox key of the envs
EMPTY = (0, 0, 0, 0)
RTOL = 1e-5

_TEAM = dict(experiment__missions__n_agents=N, experiment__uav__communication_range=100, experiment__uav__failure_rate=0.5,
             experiment__uav__fix_range=True)
_FLAT = dict(experiment__constraints__min_altitude=15, experiment__constraints__max_altitude=15, experiment__constraints__num_actions=9)
ALL16 = [(dy, dw) for dy in range(4) for dw in range(4)]
# grid -> (how the params are made, (dy, dw) shifts of every family, steps, random scenes)
GRIDS = {
    "48": (("nine", 48, {}), ALL16, 3, 36),
    "46": (("nine", 46, {}), ALL16, 3, 36),
    "34": (("set", "default", dict(sensor__pixel__number_x=4, sensor__pixel__number_y=4)), ALL16, 3, 36),
    "48p": (("nine", 48, dict(mapping__prior=0.3)), ALL16, 3, 36),
    "128": (("set", "small", {}), [(0, 0), (1, 2), (2, 0), (3, 2)], 2, 24),
    "128x512": (("set", "small", dict(environment__x_dim=50, environment__y_dim=200)), [(1, 2)], 2, 12),
    "256x512": (("set", "c4", dict(environment__x_dim=25, environment__y_dim=50)), [(1, 2)], 2, 12),
    # config 5's resolution on the smallest world whose lattice holds eight UAVs and whose rows hold a footprint of more than 64 groups
    "204x512": (("set", "c5", dict(environment__x_dim=10, environment__y_dim=25)), [(1, 2)], 2, 12),
}
# (grid, map layout, area sums tracked)
FORMS = [("48", "rows", False), ("48", "rows", True), ("48", "tiles", False), ("48", "tiles", True), ("46", "rows", False),
         ("46", "rows", True), ("128", "rows", False), ("128", "rows", True), ("34", "rows", False), ("34", "rows", True),
         ("48p", "rows", False), ("48p", "rows", True), ("128x512", "rows", False), ("128x512", "rows", True),
         ("128x512", "tiles", False), ("256x512", "rows", False), ("204x512", "rows", False)]


def _grid_params(grid):
    how, base, over = GRIDS[grid][0]
    if how == "nine":   # the 46- and 48-cell grids of test_items_met_by_nine_ops_match_oracle
        from test_hip_env_parity import _NINE_OP_GRIDS
        return make_params("small", **_TEAM, **_FLAT, **_NINE_OP_GRIDS[base], **over)
    return make_params(base, **dict(_TEAM, **over))


class Geom:
    """The sizes a grid's scenes are laid out by."""

    def __init__(self, grid):
        from ippmarl.derived import DerivedConstants
        self.grid = grid
        self.params = _grid_params(grid)
        self.d = d = DerivedConstants(self.params, philox_seed=SEED)
        self.o = O.Derived(self.params)
        self.o.exact = True
        assert d.n_agents == N and (d.grid_x, d.grid_y) == (self.o.gx, self.o.gy)
        self.gx, self.gy = d.grid_x, d.grid_y
        self.hmax, self.wmax = min(2 * max(d.radius_x), self.gx - 1), min(2 * max(d.radius_y), self.gy - 1)   # the contract's largest rectangle
        self.sx, self.sy = min(self.hmax - 3, (self.gx - 19) // 3), min(self.wmax - 3, (self.gy - 19) // 3)   # three side by side fit
        self.n_alt = d.space_z
        self.lc, self.lp = d.logit_clip, d.logit_prior
        self.shift = d.prior != 0.5
        self.round = self.gy % 32 == 0 and self.gy >= 512     # whole-line rounding of row-major rows (ippm_plan_step, ippm_sense_step)
        self.aligns, self.steps, self.n_random = GRIDS[grid][1:]


@functools.lru_cache(maxsize=None)
def geom(grid):
    return Geom(grid)


# ---------------------------------------------------------------------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------------------------------------------------------------------
def check_rect(g, r, kind="footprint"):
    """Raises unless `r` = [yu, yd, xl, xr] is inside the contract of its kind: a "footprint" (published or sensed: the code tiles
    and K3's launch are sized from the radii, and the clipped footprint of the reference never includes the last row or column),
    an "empty" one (no cells, inside the grid) or a carried "box" (WS_RECT_A: a union of footprints, any box inside the grid)."""
    yu, yd, xl, xr = (int(v) for v in r)
    if not (0 <= yu <= yd <= g.gy - 1 and 0 <= xl <= xr <= g.gx - 1):
        raise ValueError(f"{kind} {list(r)}: outside the {g.gx} x {g.gy} grid (or reversed)")
    if kind == "empty":
        if yd > yu and xr > xl:
            raise ValueError(f"empty {list(r)}: has cells")
        return
    if yd == yu or xr == xl:
        raise ValueError(f"{kind} {list(r)}: no cells")
    if kind == "footprint" and (yd - yu > 2 * max(g.d.radius_y) or xr - xl > 2 * max(g.d.radius_x)):
        raise ValueError(f"footprint {list(r)}: larger than the largest footprint {2 * max(g.d.radius_x)} x {2 * max(g.d.radius_y)}")


def _some(r):
    return r[1] > r[0] and r[3] > r[2]


def check_scene(g, sc):
    for t in range(sc["rects"].shape[0]):
        for i in range(N):
            check_rect(g, sc["rects"][t, i], "footprint" if _some(sc["rects"][t, i]) else "empty")
    for m in range(N + 1):
        if sc["flag_a"][m]:
            check_rect(g, sc["rect_a"][m], "box")
    for t in range(sc["comm"].shape[0]):
        assert all(sc["comm"][t, i, i] == 1 for i in range(N))
    assert sc["alts"].min() >= 0 and sc["alts"].max() < g.n_alt


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------
def _cols(span, other):      # side by side along the columns: span = (yu, yd), other = (xl, xr)
    return (span[0], span[1], other[0], other[1])


def _rows(span, other):      # ... along the rows
    return (other[0], other[1], span[0], span[1])


def _raw(family, rects, **kw):
    return dict(family=family, rects0=list(rects) + [EMPTY] * (N - len(rects)), **kw)


def _family_a(g):
    out = []
    for mk, s, so in ((_cols, g.sy, g.sx), (_rows, g.sx, g.sy)):
        for gap in range(6):
            for dy, dw in (g.aligns if len(g.aligns) >= 4 or mk is _rows else [(0, 0), (1, 2), (2, 0), (3, 2)]):
                a0 = 4 + dy
                w1 = s + dw
                b0 = a0 + w1 + gap
                c0 = b0 + s + (gap + 3) % 6
                o0 = 3 + dw       # staggered on the other axis: the slabs' op sets differ
                out.append(_raw("a", [mk((a0, a0 + w1), (o0, o0 + so + 2)), mk((b0, b0 + s), (o0 + 1, o0 + so)),
                                      mk((c0, c0 + s), (o0 + 2, o0 + so + 3))]))
    return out


def _family_a2(g):
    """Eight rectangles side by side on a 512-wide grid: gaps of 0 .. 5 cells, then one of 33 (more than a 128-byte line)."""
    out = []
    w = min(g.wmax - 3, 40)
    for dy in range(4):
        rects, y = [], 4 + dy
        for k, gap in enumerate([0, 1, 2, 3, 4, 5, 33, 0]):
            wk = w - 3 + (k + dy) % 4
            rects.append((y, y + wk, 5 + k, 5 + k + g.sx))
            y += wk + gap
        assert y < g.gy - 1
        out.append(_raw("a2", rects))
    return out


def _family_b(g):
    out = []
    wb, hb = min(g.wmax, g.gy - 12), min(g.hmax, g.gx - 12)
    for dy, dw in g.aligns:
        outer = (4 + dy, 4 + dy + wb - 3 + dw, 4 + dw, 4 + dw + hb - 3)
        inner = (outer[0] + 2, outer[1] - 3, outer[2] + 1, outer[3] - 2)
        py, px = outer[0] + wb // 2, outer[2] + hb // 2
        part = (py, min(g.gy - 2, py + wb - 3), px, min(g.gx - 2, px + hb - 3))
        if g.gy - 2 - (outer[1] + 3) >= 2:      # beside the outer one, or (square worlds of one footprint and a half) below it
            apart = (outer[1] + 3, min(g.gy - 2, outer[1] + 3 + g.sy), 5, 5 + g.sx)
        else:
            apart = (5, 5 + g.sy, outer[3] + 3, min(g.gx - 2, outer[3] + 3 + g.sx))
        shapes = dict(O=outer, I=inner, D=apart, P=part)
        for order in ("OID", "ODI", "IOD", "IDO", "DOI", "DIO"):      # the last op: inner, outer, apart
            out.append(_raw("b", [shapes[k] for k in order] + ([part] if order[0] != "O" else [])))
        out.append(_raw("b", [outer, outer, inner, outer]))           # identical ones
    return out


def _family_c(g):
    out = []
    for t in (1, 2, 3):
        for dy in range(4):
            c = 6 + dy
            thin_cols = (c, c + t, 4, 4 + g.sx + 3)
            thin_rows = (4 + dy, 4 + dy + g.sy + 3, c + 1, c + 1 + t)
            across = (3, 3 + g.sy, 5, 5 + g.sx)
            dot = (g.gy - 6 - dy, g.gy - 6 - dy + t, g.gx - 7, g.gx - 7 + t)
            comm = np.ones((N, N), dtype=np.uint8)
            for i, j in ((4, 0), (5, 1), (6, 3)):      # alone: maps that hear one thin rectangle and nothing else
                comm[i] = 0
                comm[i, i] = comm[i, j] = 1
            out.append(_raw("c", [thin_cols, thin_rows, across, dot], comm=comm))
    return out


def _family_d(g):
    out = []
    for dw in range(4):
        out.append(_raw("d", [(0, g.sy + dw, 0, g.sx), (g.gy - 1 - g.sy - dw, g.gy - 1, g.gx - 1 - g.sx, g.gx - 1),
                              (0, g.sy, g.gx - 4 - dw, g.gx - 1), (g.gy - 3 - dw, g.gy - 1, 0, g.sx + dw),
                              (5 + dw, 7 + dw, 0, g.hmax), (0, g.wmax, 5, 7 + dw),
                              (g.gy - 1 - g.wmax, g.gy - 1, g.gx - 1 - g.hmax, g.gx - 1)]))
    return out


def _family_e(g):
    out = []
    by, bx = min(g.wmax - 7, g.gy // 2 - 9), min(g.hmax - 7, g.gx // 2 - 9)
    ext = [(by, 0, 0, 0), (0, by, 0, 0), (0, 0, bx, 0), (0, 0, 0, bx), (by // 2, by // 2, 1, 1), (1, 1, bx // 2, bx // 2),
           (by // 2, 0, bx // 2, 0), (0, by // 2, 0, bx // 2)]
    for dy, dw in g.aligns:
        cy, cx = g.gy // 2 - 2 + dy, g.gx // 2 - 2 + dw
        rects = [(cy - a, cy + 4 + b + (dw if k == 1 else 0), cx - c, cx + 4 + e) for k, (a, b, c, e) in enumerate(ext)]
        box = (cy - 1, cy + 6, cx - 1, cx + 5)
        out.append(_raw("e", rects, flag_a={m: box for m in range(N + 1)}, flag_s=set(range(N))))
    return out


def _family_f(g):
    out = []
    quiet = np.ones((N, N), dtype=np.uint8)
    for i in (3, 4, 5):
        quiet[i] = 0
        quiet[i, i] = 1
    for dy in range(4):
        base = [(4 + dy, 4 + dy + g.sy, 4, 4 + g.sx), (6 + dy + g.sy // 2, 6 + dy + g.sy // 2 + g.sy, 6, 6 + g.sx),
                (5, 5 + g.sy, 3 + g.sx // 2, 3 + g.sx // 2 + g.sx), (g.gy - 3 - g.sy, g.gy - 3, g.gx - 3 - g.sx, g.gx - 3),
                (8 + dy, 9 + dy + g.sy, g.gx - 5 - g.sx, g.gx - 5), (g.gy - 4 - g.sy - dy, g.gy - 4, 7, 7 + g.sx)]
        big = (2, g.gy - 3, 2, g.gx - 3)                                  # larger than any footprint
        far = (g.gy - 9, g.gy - 2, g.gx - 9, g.gx - 2)
        over = (2 + dy, 2 + dy + g.sy + 5, 2, min(g.gx - 2, 2 + 2 * g.sx))
        # the global map and local 0: the big box; local 1: a box apart from its messages; local 2: one that overlaps them, and its own
        # rectangle; local 3: its own rectangle and nothing received (the box is born); local 4: both and nothing received (the box grows);
        # local 5 hears nobody until the last step
        steps = [quiet] * (g.steps - 1) + [np.ones((N, N), dtype=np.uint8)]
        out.append(_raw("f", base, comm=steps, flag_a={N: big, 0: big, 1: far, 2: over, 4: far, 5: over}, flag_s={2, 3, 4, 5},
                        alts=np.zeros(N, dtype=np.int64)))
    return out


def _family_g(g):
    body = [(4, 4 + g.sy, 4, 4 + g.sx), (6, 6 + g.sy, 5 + g.sx // 2, 5 + g.sx // 2 + g.sx), (3 + g.sy // 2, 3 + g.sy // 2 + g.sy, 6, 6 + g.sx)]
    lonely = np.ones((N, N), dtype=np.uint8)
    lonely[0] = 0
    lonely[0, 0] = lonely[0, 7] = 1            # local 0 hears one agent, and that one has no footprint
    box = (3, 3 + g.sy, 3, 3 + g.sx)
    return [_raw("g", body + [(4, 9, 6, 6), EMPTY, EMPTY, EMPTY, (5, 5, 3, 9)], flag_a={N: box, 1: box}),    # no rows / no columns, the last source
            _raw("g", body, comm=lonely, flag_a={0: box, N: box}, flag_s={0}),
            _raw("g", [EMPTY] * N, flag_a={N: box, 2: box}, flag_s={3})]                                       # nobody has a footprint


def _random_rect(g, rs, small):
    h = int(rs.randint(1, (min(g.hmax, 9) if small else g.hmax) + 1))
    w = int(rs.randint(1, (min(g.wmax, 9) if small else g.wmax) + 1))
    xl, yu = int(rs.randint(0, g.gx - h)), int(rs.randint(0, g.gy - w))
    return (yu, yu + w, xl, xl + h)


def _random_box(g, rs):
    y = np.sort(rs.choice(g.gy, 2, replace=False))
    x = np.sort(rs.choice(g.gx, 2, replace=False))
    return (int(y[0]), int(y[1]), int(x[0]), int(x[1]))


def _family_h(g):
    out = []
    for k in range(g.n_random):
        rs = np.random.RandomState(7000 + k)

        def team():
            n = int(rs.randint(2, N + 1))
            who = set(rs.choice(N, n, replace=False).tolist())
            return [_random_rect(g, rs, rs.rand() < 0.3) if i in who else EMPTY for i in range(N)]

        comm = []
        for _ in range(g.steps):
            c = (rs.rand(N, N) < 0.6).astype(np.uint8)
            c[np.arange(N), np.arange(N)] = 1
            comm.append(c)
        out.append(_raw("h", team(), comm=comm, steps=[team() for _ in range(g.steps)],
                        flag_a={m: _random_box(g, rs) for m in range(N + 1) if rs.rand() < 0.3},
                        flag_s={i for i in range(N) if rs.rand() < 0.3}, alts=rs.randint(0, g.n_alt, size=(g.steps + 1, N))))
    return out


def _filler(g, k):
    """Prior != 0.5: an agent without a footprint publishes no message; a small rectangle in the far corner takes its place."""
    xl = g.gx - 4 - 3 * k
    return (g.gy - 5, g.gy - 2, xl, xl + 2)


# Initial maps whose float32 restatement does not keep half of every bound (test_float32_restatement_keeps_half_of_every_bound) are not
# used: these scenes draw theirs from another seed.  (Nine ops and a sensing per step on the one-altitude grids: up to thirty float32
# roundings of a cell that stays next to -logit_clip, where one rounding is 5e-7 of p.)
RESEED = {('48', 324): 104324, ('48', 329): 104329, ('48', 339): 104339, ('46', 323): 304323, ('46', 325): 404325, ('46', 328): 204328,
          ('46', 332): 104332, ('46', 339): 104339}


def _finish(g, raw, idx):
    T = g.steps
    rects = np.zeros((T + 1, N, 4), dtype=np.int64)
    rects[0] = raw["rects0"]
    for t in range(T):      # what is sensed at the end of step t: given, or the published rectangles one agent further
        rects[t + 1] = raw["steps"][t] if raw.get("steps") else np.roll(rects[t], -1, axis=0)
    if g.shift:
        for t in range(T + 1):
            for i in range(N):
                if not _some(rects[t, i]):
                    rects[t, i] = _filler(g, i)
    comm = raw.get("comm")
    if comm is None:
        comm = np.ones((N, N), dtype=np.uint8)
    comm = np.array(comm, dtype=np.uint8)
    comm = np.broadcast_to(comm, (T, N, N)).copy() if comm.ndim == 2 else comm
    alts = raw.get("alts")
    if alts is None:
        alts = (np.arange(N)[None, :] + 2 * np.arange(T + 1)[:, None]) % g.n_alt
    alts = np.broadcast_to(np.asarray(alts, dtype=np.int64) % g.n_alt, (T + 1, N)).copy()
    flag_a = np.zeros(N + 1, dtype=np.int64)
    rect_a = np.zeros((N + 1, 4), dtype=np.int64)
    for m, box in (raw.get("flag_a") or {}).items():
        flag_a[m], rect_a[m] = 1, box
    flag_s = np.zeros(N, dtype=np.int64)
    for i in (raw.get("flag_s") or ()):
        flag_s[i] = 1 if _some(rects[0, i]) else 0     # (K3 sets it for a footprint it wrote)
    sc = dict(family=raw["family"], name=f"{raw['family']}{idx}", rects=rects, comm=comm, alts=alts, flag_a=flag_a, rect_a=rect_a, flag_s=flag_s,
              seed=RESEED.get((g.grid, idx), 4000 + idx), episode=11 + 7 * idx)
    check_scene(g, sc)
    return sc


@functools.lru_cache(maxsize=None)
def make_scenes(grid):
    g = geom(grid)
    raws = _family_a(g) + (_family_a2(g) if g.round else []) + _family_b(g) + _family_c(g) + _family_d(g) + _family_e(g) + _family_f(g)
    raws += ([] if g.shift else _family_g(g)) + _family_h(g)
    return [_finish(g, raw, k) for k, raw in enumerate(raws)]


def initial_state(g, sc):
    """(local [N, gx, gy], global [gx, gy] float32 log-odds, measurement bits of the published rectangles): a state the device could be
    in -- values beyond +-logit_clip (+-inf among them) only inside WS_RECT_A of a map whose WS_FLAG_A is set and inside the own
    rectangle of a local map whose WS_FLAG_S is set; a third of the cells still at the prior."""
    rs = np.random.RandomState(sc["seed"])
    lc32 = np.float32(g.lc)
    maps = np.clip(rs.uniform(-g.lc, g.lc, size=(N + 1, g.gx, g.gy)).astype(np.float32), -lc32, lc32)
    maps[rs.rand(N + 1, g.gx, g.gy) < 0.3] = np.float32(g.lp)

    def heat(m, r):
        yu, yd, xl, xr = r
        v = rs.uniform(-1.7 * g.lc, 1.7 * g.lc, size=(xr - xl, yd - yu)).astype(np.float32)
        v[rs.rand(*v.shape) < 0.05] = np.inf
        v[rs.rand(*v.shape) < 0.05] = -np.inf
        maps[m, xl:xr, yu:yd] = v

    for m in range(N + 1):
        if sc["flag_a"][m]:
            heat(m, sc["rect_a"][m])
    for i in range(N):
        if sc["flag_s"][i]:
            heat(i, sc["rects"][0, i])
    bits = [rs.randint(0, 2, size=(r[3] - r[2], r[1] - r[0])).astype(np.uint8) for r in sc["rects"][0]]
    return maps[:N], maps[N], bits


# ---------------------------------------------------------------------------------------------------------------------------------
# host model of the planner (csrc/step_small.hip: plan_map, tile_build_map)
# ---------------------------------------------------------------------------------------------------------------------------------
def plan_model(st, takes, rects, i, is_global):
    """plan_map: st = [flag_a, rect_a (4), flag_s] of the map (updated in place), takes = the agents whose messages it receives,
    rects = the published rectangles.  -> (ops [(type, src, rect)], index of the last op or -1, the branches taken)."""
    branches = set()
    if not takes:
        if not is_global and st[5]:
            own = list(rects[i])
            if st[0]:
                st[1:5] = [min(st[1], own[0]), max(st[2], own[1]), min(st[3], own[2]), max(st[4], own[3])]
                branches.add("carry with merge")
            else:
                st[1:5] = own
                branches.add("carry without merge")
            st[0], st[5] = 1, 0
        return [], -1, branches
    ops = []
    if st[0] and _some(st[1:5]):
        ops.append((0, -1, tuple(st[1:5])))
        branches.add("clamp from A")
    if not is_global and st[5] and _some(rects[i]):
        ops.append((0, -1, tuple(rects[i])))
        branches.add("clamp from S")
    last = -1
    for j in sorted(takes):
        if _some(rects[j]):
            ops.append((1, j, tuple(rects[j])))
        if j == max(takes):
            last = len(ops) - 1 if _some(rects[j]) else -1
            if not _some(rects[j]):
                branches.add("empty last source")
            st[1:5] = list(rects[j])
    st[0], st[5] = 0, 0
    return ops, last, branches


def plan_regions(ops, gy, round_mask=0):
    """tile_build_map on row-major maps: the (slab, column interval) regions of a plan as (xa, xb, g0, g1, op mask) in 4-cell groups,
    intervals rounded outwards to multiples of round_mask + 1 groups before they are merged."""
    G = (gy + 3) // 4
    edges = sorted({r[2] for _, _, r in ops} | {r[3] for _, _, r in ops})
    out = []
    for xa, xb in zip(edges, edges[1:]):
        act = sorted((k for k, (_, _, r) in enumerate(ops) if r[2] <= xa < r[3]), key=lambda k: (ops[k][2][0], k))
        g0 = g1 = mask = 0
        for k in act:
            yu, yd = ops[k][2][:2]
            lo, hi = (yu >> 2) & ~round_mask, min(G, (((yd + 3) >> 2) + round_mask) & ~round_mask)
            if mask and lo > g1:
                out.append((xa, xb, g0, g1, mask))
                mask = 0
            if not mask:
                g0, g1 = lo, hi
            else:
                g1 = max(g1, hi)
            mask |= 1 << k
        if mask:
            out.append((xa, xb, g0, g1, mask))
    return out


def side_gaps(ops, axis):
    """(gap, gap start % 4) of neighbouring ops of one slab along `axis` (0: columns inside a slab of rows, 1: rows inside a slab of
    columns) that leave 0 .. 5 uncovered cells between them."""
    lo, hi, a, b = (0, 1, 2, 3) if axis == 0 else (2, 3, 0, 1)
    edges = sorted({r[a] for _, _, r in ops} | {r[b] for _, _, r in ops})
    found = set()
    for ea in edges[:-1]:
        act = sorted((r[lo], r[hi]) for _, _, r in ops if r[a] <= ea < r[b])
        end = None
        for s, e in act:
            if end is not None and 0 <= s - end <= 5:
                found.add((s - end, end % 4))
            end = e if end is None else max(end, e)
    return found


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference: mappings.py:82-124 in log-odds
# ---------------------------------------------------------------------------------------------------------------------------------
def _sigmoid(L):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-L.astype(np.float64)))


def assert_maps(got_p, want_logodds, msg):
    """assert_posteriors(strict): every cell of every map within 1e-5 relative -- env by env, to keep the temporaries small."""
    for e in range(len(got_p)):
        assert_posteriors(got_p[e], _sigmoid(want_logodds[e]), strict=True, msg=f"{msg}, env {e}")


class Sim:
    """The scenes of a grid stepped on the host.  float64: the reference -- for every received message in ascending source order clip
    the WHOLE grid to +-lc, subtract logit(prior) everywhere, add the measurement's log-odds inside its rectangle (a message without a
    footprint adds nothing and, prior 0.5, shifts nothing); a map that receives nothing is untouched; K3: cells of the rectangle get
    clip(L) + l(truth xor flip) - logit(prior).  float32: the same chain in the device's number format (prior != 0.5: the chain of
    a fusion in float64, rounded once, as csrc/fuse.hip says it does), the headroom check of the tolerances."""

    def __init__(self, grid, dtype=np.float64, scenes=None):
        self.g = g = geom(grid)
        self.scenes = make_scenes(grid) if scenes is None else scenes
        self.dtype = dtype
        self.E = len(self.scenes)
        self.local = np.zeros((self.E, N, g.gx, g.gy), dtype=dtype)
        self.glob = np.zeros((self.E, g.gx, g.gy), dtype=dtype)
        self.bits, self.state = [], []
        for e, sc in enumerate(self.scenes):
            lo, gl, bits = initial_state(g, sc)
            self.local[e], self.glob[e] = lo, gl
            self.bits.append(bits)
            self.state.append([[int(sc["flag_a"][m])] + [int(v) for v in sc["rect_a"][m]] + [int(sc["flag_s"][m]) if m < N else 0]
                               for m in range(N + 1)])
        f32 = dtype == np.float32
        self.lc = np.float32(g.lc) if f32 else g.lc
        self.lm = g.d.logit_meas if f32 else g.d.logit_meas.astype(np.float64)      # (the reference forms them in float32)
        self.lp = np.float32(g.lp) if f32 else g.lp
        self.truth = [O.make_truth(g.o, sc["episode"]).astype(np.uint8) for sc in self.scenes]

    def _fuse(self, L, msgs):
        g = self.g
        chain = L.astype(np.float64) if (self.dtype == np.float32 and g.shift) else L
        lc, lp = (g.lc, g.lp) if chain.dtype == np.float64 else (self.lc, self.lp)
        for (yu, yd, xl, xr), bits, lm in msgs:
            np.clip(chain, -lc, lc, out=chain)
            if g.shift:
                chain -= lp
            if xr > xl and yd > yu:
                chain[xl:xr, yu:yd] += np.where(bits != 0, lm[1], lm[0]).astype(chain.dtype)
        L[...] = chain

    def fuse(self, t):
        """The fusions of step t.  -> per env: plans [(ops, last, branches, takes)] of the N + 1 maps, (S1, S2)."""
        g = self.g
        plans, sums = [], []
        for e, sc in enumerate(self.scenes):
            rects, alts = sc["rects"][t], sc["alts"][t]
            msg = [(tuple(rects[j]), self.bits[e][j], self.lm[alts[j]]) for j in range(N)]
            env_plans = []
            for m in range(N + 1):
                takes = list(range(N)) if m == N else [j for j in range(N) if j != m and sc["comm"][t, m, j]]
                ops, last, br = plan_model(self.state[e][m], takes, rects, m, m == N)
                env_plans.append((ops, last, br, takes))
                if m < N:
                    self._fuse(self.local[e, m], [msg[j] for j in takes])
            before = self.glob[e].copy()
            self._fuse(self.glob[e], msg)
            plans.append(env_plans)
            sums.append(reward_sums(g, before, self.glob[e], self.dtype))
        return plans, np.array(sums)

    def sense(self, t):
        """K3 of step t (stage t + 1) at the rectangles rects[t + 1].  -> per env and agent the observation bits."""
        g = self.g
        obs = []
        for e, sc in enumerate(self.scenes):
            row = []
            for i in range(N):
                yu, yd, xl, xr = r = tuple(int(v) for v in sc["rects"][t + 1, i])
                if not _some(r):
                    row.append(np.zeros((xr - xl, yd - yu), dtype=np.uint8))
                    continue
                k = sc["alts"][t + 1, i]
                ok = O.philox_correctness(SEED, sc["episode"], i, t + 1, r, g.gy, O.noise_of_altitude(g.d.altitudes[k]))
                bits = (self.truth[e][xl:xr, yu:yd] ^ (1 - ok).astype(np.uint8)).astype(np.uint8)
                cells = self.local[e, i, xl:xr, yu:yd]
                lm = self.lm[k]
                add = np.where(bits != 0, lm[1] - self.lp, lm[0] - self.lp).astype(self.dtype)
                cells[...] = np.clip(cells, -self.lc, self.lc) + add
                row.append(bits)
            obs.append(row)
            self.bits[e] = row
        return obs


def reward_sums(g, before, after, dtype=np.float64):
    """(S1, S2) of utils/reward.py:68-82 from log-odds maps: the oracle's own (float64), or per-cell float32 terms summed in float64."""
    if dtype == np.float64:
        return O.reward_sums(g.o, _sigmoid(before), _sigmoid(after))
    wt = np.float32(g.d.logit_weight_thr)

    def entropy(L):      # ippm_entropy_l (csrc/ippm_internal.h): H = log2(1 + e) + a log2(e_) e / (1 + e), a = min(|L|, lc), e = exp(-a)
        one = np.float32(1)
        a = np.minimum(np.abs(L), np.float32(g.lc)).astype(np.float32)
        ex = np.exp(-a).astype(np.float32)
        return (np.log2(one + ex) + (a * np.float32(1.44269504)) * (ex / (one + ex))).astype(np.float32)

    w = np.where(after > wt, np.float32(1), np.where(after < -wt, np.float32(0), np.float32(0.5)))
    hb, ha = entropy(before), entropy(after)
    return float(np.sum((w * (hb - ha)).astype(np.float64))), float(np.sum((w * hb).astype(np.float64)))


def rewards_of(g, s1, s2):
    return 22.0 * (s1 / s2) - 0.5, 10.0 * (s1 / (g.gx * g.gy)) - 0.17


def sums_atol(g, s2):
    """_check_env_step's bound on S1 and S2: atol = 1e-6 + s_scale |S2| with its s_scale per regime (rtol = 1e-5 beside it)."""
    noise_free = any(z not in (5, 10, 15) for z in g.d.altitudes)
    s_scale = 1e-6 if g.d.prior != 0.5 else (2e-7 if noise_free else 2e-8)
    return 1e-6 + s_scale * abs(s2)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
def test_contract_helper_rejects_each_kind_of_bad_rectangle():
    g = geom("48")
    check_rect(g, (0, 16, 0, 16))
    check_rect(g, (31, 47, 31, 47))
    check_rect(g, (5, 5, 3, 9), "empty")
    check_rect(g, (0, 47, 0, 47), "box")
    for bad, kind in [((-1, 8, 0, 8), "footprint"), ((0, 8, -1, 8), "footprint"),         # left of / above the grid
                      ((40, 48, 0, 8), "footprint"), ((0, 8, 40, 48), "footprint"),       # the last column / row
                      ((9, 5, 0, 8), "footprint"), ((0, 8, 9, 5), "footprint"),           # reversed
                      ((5, 5, 0, 8), "footprint"), ((0, 8, 5, 5), "footprint"),           # no cells, not declared empty
                      ((0, 17, 0, 8), "footprint"), ((0, 8, 0, 17), "footprint"),         # wider / taller than the largest footprint
                      ((0, 8, 0, 8), "empty"), ((0, 48, 0, 8), "box"), ((3, 3, 0, 8), "box")]:
        with pytest.raises(ValueError):
            check_rect(g, bad, kind)
    sc = dict(make_scenes("48")[0])
    sc["rects"] = sc["rects"].copy()
    sc["rects"][1, 2] = (0, 30, 0, 8)
    with pytest.raises(ValueError):
        check_scene(g, sc)


@functools.lru_cache(maxsize=None)
def study(grid):
    return _study(grid, None)


def _study(grid, scenes):
    """The scenes of a grid stepped by the reference and by its float32 restatement: what the plans reach, and how far the two are apart."""
    g = geom(grid)
    ref, f32 = Sim(grid, scenes=scenes), Sim(grid, np.float32, scenes=scenes)
    lc32 = float(np.float32(g.lc))
    reach = dict(align=set(), xy=set(), col_gaps=set(), row_gaps=set(), masks=set(), branches=set(), long_items=0, long_with_single=0,
                 swallowed=0, kept_apart=0, max_groups=0)
    worst = {k: np.zeros(ref.E) for k in ("maps", "s1", "s2", "rel", "abs")}      # per scene, as fractions of the bound

    def apart(a, b):
        out = np.zeros(len(a))
        for e in range(len(a)):
            pa, pb = _sigmoid(a[e]), _sigmoid(b[e])
            with np.errstate(divide="ignore", invalid="ignore"):
                out[e] = float(np.nanmax(np.where(pa == pb, 0.0, np.abs(pa - pb) / np.abs(pb)))) / RTOL
        return out

    for t in range(g.steps):
        plans, sums = ref.fuse(t)
        _, sums32 = f32.fuse(t)
        for e in range(ref.E):
            for m, (ops, last, br, takes) in enumerate(plans[e]):
                reach["branches"] |= br
                # the flags the fusion leaves: WS_FLAG_A where the last op's rectangle holds a value beyond the clip
                for sim in (ref, f32):
                    if takes:
                        L = sim.glob[e] if m == N else sim.local[e, m]
                        r = ops[last][2] if last >= 0 else None
                        cells = L if (g.shift and ops) else (L[r[2]:r[3], r[0]:r[1]] if r else np.zeros(0))
                        sim.state[e][m][0] = int(bool((np.abs(cells) > lc32).any()))
                for tp, _, r in ops:
                    reach["align"].add((r[0] % 4, r[1] % 4))
                    reach["xy"].add(("x", r[2] % 4))
                    reach["xy"].add(("y", r[0] % 8))
                    if tp == 1:      # (a message: a footprint, whose rows K3 walks too)
                        reach["max_groups"] = max(reach["max_groups"], ((r[1] + 3) >> 2) - (r[0] >> 2))
                if not ops:
                    continue
                reach["col_gaps"] |= side_gaps(ops, 0)
                reach["row_gaps"] |= side_gaps(ops, 1)
                regions = plan_regions(ops, g.gy, 7 if g.round else 0)
                pops = [bin(mask).count("1") for *_, mask in regions]
                reach["masks"] |= {(len(ops), mask) for *_, mask in regions}
                if max(pops) >= 7 and len({r for _, _, r in ops}) >= 7:
                    reach["long_items"] += 1
                    reach["long_with_single"] += 1 if 1 in pops else 0
                if g.round:
                    plain = plan_regions(ops, g.gy, 0)
                    reach["swallowed"] += 1 if len(regions) < len(plain) else 0
                    reach["kept_apart"] += 1 if any(a[:2] == b[:2] and a is not b for a in regions for b in regions) else 0
            s1, s2 = sums[e]
            worst["s1"][e] = max(worst["s1"][e], abs(sums32[e, 0] - s1) / (RTOL * abs(s1) + sums_atol(g, s2)))
            worst["s2"][e] = max(worst["s2"][e], abs(sums32[e, 1] - s2) / (RTOL * abs(s2) + sums_atol(g, s2)))
            (rel, ab), (rel32, ab32) = rewards_of(g, s1, s2), rewards_of(g, *sums32[e])
            worst["rel"][e] = max(worst["rel"][e], abs(rel32 - rel) / (RTOL * abs(rel) + 1e-6 + RTOL * 0.5))
            worst["abs"][e] = max(worst["abs"][e], abs(ab32 - ab) / (RTOL * abs(ab) + 1e-6 + RTOL * 0.17))
        worst["maps"] = np.maximum(worst["maps"], np.maximum(apart(f32.local, ref.local), apart(f32.glob, ref.glob)))
        ref.sense(t)
        f32.sense(t)
        for e in range(ref.E):
            for i in range(N):     # WS_FLAG_S where K3 wrote a value beyond the clip
                r = ref.scenes[e]["rects"][t + 1, i]
                for sim in (ref, f32):
                    if _some(r) and (np.abs(sim.local[e, i, r[2]:r[3], r[0]:r[1]]) > lc32).any():
                        sim.state[e][i][5] = 1
        worst["maps"] = np.maximum(worst["maps"], apart(f32.local, ref.local))
    return reach, worst


@pytest.mark.parametrize("grid", list(GRIDS))
def test_scene_sets_reach_what_they_claim(grid):
    g = geom(grid)
    reach, _ = study(grid)
    print(grid, len(make_scenes(grid)), {k: (len(v) if isinstance(v, set) else v) for k, v in reach.items()})
    assert len(reach["align"]) == 16, sorted(reach["align"])
    assert len(reach["xy"]) == 12, sorted(reach["xy"])
    assert reach["col_gaps"] >= {(gap, ph) for gap in range(6) for ph in range(4)}, sorted(reach["col_gaps"])
    if len(g.aligns) > 1:       # (the 512-wide grids lay the row families out at one shift: every gap, not at every row phase)
        assert reach["row_gaps"] >= {(gap, ph) for gap in range(6) for ph in range(4)}, sorted(reach["row_gaps"])
    else:
        assert {gap for gap, _ in reach["row_gaps"]} == set(range(6)) and len(reach["row_gaps"]) >= 10
    assert reach["long_items"] > 0 and reach["long_with_single"] > 0           # an item met by 7+ different rectangles, neighbours met by one
    want = {"clamp from A", "clamp from S", "carry with merge", "carry without merge"} | (set() if g.shift else {"empty last source"})
    assert reach["branches"] == want, reach["branches"]
    if g.round:
        assert reach["swallowed"] > 0 and reach["kept_apart"] > 0              # a rounded interval swallows a neighbour's gap; a wide gap survives
    # the forms the module docstring promises for this grid
    groups = reach["max_groups"]
    assert g.d.vec == (1 if grid == "34" else 4)
    assert (groups > 32) == (grid in ("256x512", "204x512")) and (groups > 64) == (grid == "204x512")


def test_float64_restatement_equals_the_oracle():
    """Sim against O.fuse_map / O.bayes_update in probabilities (exact mode), map by map, on a handful of scenes per prior."""
    for grid, picks in (("48", ("a", "b", "e", "f", "g", "h")), ("48p", ("a", "e", "f", "h")), ("128", ("b", "h"))):
        g = geom(grid)
        chosen = []
        for fam in picks:
            chosen += [sc for sc in make_scenes(grid) if sc["family"] == fam][:2]
        sim = Sim(grid, scenes=chosen)
        for t in range(g.steps):
            before = _sigmoid(sim.local), _sigmoid(sim.glob)
            bits_t = [list(b) for b in sim.bits]
            sim.fuse(t)
            for e, sc in enumerate(chosen):
                m2c = []
                for j in range(N):
                    yu, yd, xl, xr = sc["rects"][t, j]
                    m = np.full((g.gx, g.gy), 0.5, dtype=np.float32)
                    if _some(sc["rects"][t, j]):
                        m[xl:xr, yu:yd] = g.d.meas_value[sc["alts"][t, j]][bits_t[e][j]]
                    m2c.append(m)
                for i in range(N):
                    others = [m2c[j] for j in range(N) if j != i and sc["comm"][t, i, j]]
                    want = O.fuse_map(g.o, before[0][e, i].copy(), others, i, "global")
                    np.testing.assert_allclose(_sigmoid(sim.local[e, i]), want, rtol=1e-9, atol=0, err_msg=f"{grid} {sc['name']} t={t} local {i}")
                want = O.fuse_map(g.o, before[1][e].copy(), m2c, None, "global")
                np.testing.assert_allclose(_sigmoid(sim.glob[e]), want, rtol=1e-9, atol=0, err_msg=f"{grid} {sc['name']} t={t} global")
            before = _sigmoid(sim.local)
            obs = sim.sense(t)
            for e, sc in enumerate(chosen):
                for i in range(N):
                    yu, yd, xl, xr = sc["rects"][t + 1, i]
                    want = before[e, i].copy()
                    if _some(sc["rects"][t + 1, i]):
                        meas = g.d.meas_value[sc["alts"][t + 1, i]][obs[e][i]]
                        want[xl:xr, yu:yd] = O.bayes_update(want[xl:xr, yu:yd], meas, g.o.prior)
                    np.testing.assert_allclose(_sigmoid(sim.local[e, i]), want, rtol=1e-9, atol=0, err_msg=f"{grid} {sc['name']} t={t} K3 {i}")


@pytest.mark.parametrize("grid", list(GRIDS))
def test_float32_restatement_keeps_half_of_every_bound(grid):
    """The tolerances of the GPU tests are the suite's own; what they are asked of is arithmetic a float32 chain can do: the same
    scenes in float32 NumPy stay within HALF of each bound (worst figure / bound printed), so a failure on the device is the kernel's."""
    _, worst = study(grid)
    print(grid, {k: round(float(v.max()), 4) for k, v in worst.items()})
    for k, v in worst.items():
        assert v.max() <= 0.5, (grid, k, make_scenes(grid)[int(v.argmax())]["name"], float(v.max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
def _starts(g):
    """Eight distinct lattice points a few metres apart (a pair at distance 0 always hears each other)."""
    span = min(g.d.space_x, 4)
    assert (N + span - 1) // span <= g.d.space_y
    return [[g.d.spacing * (i % span), g.d.spacing * (i // span), 15] for i in range(N)]


class Runner:
    """One VecEnv whose envs are the scenes of a grid, driven through the env's own members: reset(), the state overwritten,
    build_observations() for plan and fusion (or, `standalone`, ippm_comm_matrix + ippm_fuse_local + ippm_fuse_global_reward),
    _sense() from hand-written sense records."""

    def __init__(self, grid, layout, track, standalone=False):
        import torch
        from ippmarl import _ffi
        from ippmarl.vec_env import VecEnv
        self.torch, self._ffi = torch, _ffi
        self.g = g = geom(grid)
        self.scenes = make_scenes(grid)
        self.E = E = len(self.scenes)
        self.standalone = standalone
        self.env = env = VecEnv(g.params, E, philox_seed=SEED, track_area=track, map_layout=layout)
        assert env.tiled == (layout == "tiles") and (env.d.grid_x, env.d.grid_y) == (g.gx, g.gy)
        dev = env.device
        env.reset([sc["episode"] for sc in self.scenes], start_positions=torch.tensor([_starts(g)] * E, dtype=torch.int32))
        local = np.zeros((E, N, g.gx, g.gy), dtype=np.float32)
        glob = np.zeros((E, g.gx, g.gy), dtype=np.float32)
        code = np.zeros((E, N, env.d.tile_bytes), dtype=np.uint8)
        ws = np.zeros((E, N + 1, 6), dtype=np.int32)
        for e, sc in enumerate(self.scenes):
            local[e], glob[e], bits = initial_state(g, sc)
            for i in range(N):
                if _some(sc["rects"][0, i]):
                    code[e, i] = env.d.pack_tile(sc["rects"][0, i], bits[i])
            ws[e, :, 0], ws[e, :, 1:5], ws[e, :N, 5] = sc["flag_a"], sc["rect_a"], sc["flag_s"]
        env.local.copy_(env.tiles_view(torch.from_numpy(local).to(dev)))
        env.glob.copy_(env.tiles_view(torch.from_numpy(glob).to(dev)))
        env.code.copy_(torch.from_numpy(code).to(dev))
        env.ws[..., 0:6] = torch.from_numpy(ws).to(dev)
        self.rects = torch.from_numpy(np.stack([sc["rects"] for sc in self.scenes]).astype(np.int32)).to(dev)      # [E, T + 1, N, 4]
        self.alts = np.stack([sc["alts"] for sc in self.scenes])                                                     # [E, T + 1, N]
        self.draws = torch.from_numpy(np.stack([sc["comm"] for sc in self.scenes]).astype(np.float64)).to(dev)      # 1.0 passes, 0.0 fails
        self._publish(0)
        env.rect.copy_(self.rects[:, 0])
        # the global maps were replaced: T, the running weighted entropy, is seeded again (include/ippmarl.h, ippm_fuse_global_reward)
        ent = torch.zeros(E, dtype=torch.float64, device=dev)
        env.ctx.call("ippm_weighted_entropy", env._p(env.glob), None, 1, _ffi.ptr(ent), E, env.stream)
        env.sums.zero_()
        env.sums[:, 2] = ent
        if track:
            env.rebuild_area()
        torch.cuda.synchronize()

    def _publish(self, t):
        """The altitudes of the measurements rects[t] (the plan kernel takes a message's log-odds from the z of `pos`)."""
        env, torch = self.env, self.torch
        z = np.asarray(env.d.altitudes)[self.alts[:, t]]
        env.pos[..., 2] = torch.from_numpy(z.astype(np.int32)).to(env.device)

    def rows(self, maps):
        return self.env.rows_view(maps)

    def fuse(self, t):
        env = self.env
        draws = self.draws[:, t].contiguous()
        if self.standalone:
            env.comm_matrix(t, draws)
            env.fuse_local()
            env.ctx.call("ippm_fuse_global_reward", env._p(env.glob), env._p(env.code), env._p(env.rect), env._p(env.pos), env._p(env.ws),
                         env._p(env.sums), env._p(env.reward), env.E, env.stream)
        else:
            env.build_observations(t, comm_draws=draws, features=False)
            env._pending_t = None

    def sense(self, t):
        """K3 of step t from sense records written here as ippm_plan_step's K1 writes them (include/ippmarl.h, rect_next)."""
        env, torch, d = self.env, self.torch, self.env.d
        self._publish(t + 1)
        lm = (np.asarray(d.logit_meas, dtype=np.float32) - np.float32(d.logit_prior)).view(np.int32)       # [levels, 2] float bits
        thr = np.asarray(d.flip_threshold).astype(np.uint32).view(np.int32)
        k = self.alts[:, t + 1]
        rec = np.zeros((self.E, N, 8), dtype=np.int32)
        rec[..., 0:4] = self.rects[:, t + 1].cpu().numpy()
        rec[..., 4:6] = lm[k]
        rec[..., 6] = thr[k]
        env.rect_next.copy_(torch.from_numpy(rec).to(env.device))
        if self.standalone:   # (ippm_fuse_global_reward has completed the step's reward itself)
            env.ctx.call("ippm_sense_step", env._p(env.episode), env._p(env.pos), env._p(env.truth), env._p(env.local), None, env._p(env.code),
                         env._p(env.rect_next), env._p(env.rect), env._p(env.ws), env._area_arg, None, None, t + 1, -1, env.E, env.stream)
        else:
            env._sense(t + 1, close_step=True)

    def fresh_area(self):
        env, torch = self.env, self.torch
        fresh = torch.zeros_like(env.area)
        env.ctx.call("ippm_area_sums", env._p(env.local), self._ffi.ptr(fresh), env.E * N, N, 0, env.stream)
        env.ctx.call("ippm_area_sums", env._p(env.glob), self._ffi.ptr(fresh), env.E, 1, N, env.stream)
        return fresh

    def check_area(self, tag):
        """The bound of test_tracked_area_sums_equal_a_streaming_recomputation (area averages lie in [0, 1])."""
        G = self.g.gx * self.g.gy
        np.testing.assert_allclose(self.env.area.cpu().numpy() / G, self.fresh_area().cpu().numpy() / G, rtol=0, atol=3e-7, err_msg=tag)


def _kernels(grid, layout, track):
    """The instantiations a form must run, as ippm_read_kernel_times spells them (include/ippmarl.h)."""
    g = geom(grid)
    tr, mis = str(track).lower(), str(g.gy % 4 != 0).lower()
    if g.d.vec == 1:
        return "k_fuse_rows<1, %s, 10, false>" % tr, ("k_sense_update" if track else "k_sense_tiles<1, false, false, true, false, false, false>")
    if g.shift:
        fuse = "k_fuse_rows<4, %s, 18, true>" % tr
    else:
        fuse = "k_fuse_tiles<%s, %s%s>" % (mis, tr, ", true" if layout == "tiles" else "")
    sense = "k_sense_tiles<4, %s, false, true, true, %s, %s" % (mis, tr, str(layout == "tiles").lower())
    if not track and g.gy % 4 == 0:      # the closing K3 of the env-only step: its workgroup shape by the widest footprint row
        groups = (2 * max(g.d.radius_y) + 3) // 4 + 1
        shape = (1, 3, 0) if (layout == "tiles" and groups <= 32) else ((2, 2, 1) if groups <= 32 else ((2, 2, 0) if groups <= 64 else (4, 3, 0)))
        sense += ", %d, %d, %d" % shape if shape != (4, 3, 0) else ""     # (4 wavefronts x 3 loads, parts first: the launch site's default, unspelt)
    return fuse, sense + ">"


def _op_mask(g, E, plans):
    """bool [E, N + 1, gx, gy]: the cells inside an op rectangle of the map's plan (prior != 0.5: a plan with a message walks the whole grid)."""
    mask = np.zeros((E, N + 1, g.gx, g.gy), dtype=bool)
    for e in range(E):
        for m, (ops, _, _, _) in enumerate(plans[e]):
            if g.shift and any(tp for tp, _, _ in ops):
                mask[e, m] = True
            for _, _, (yu, yd, xl, xr) in ops:
                mask[e, m, xl:xr, yu:yd] = True
    return mask


@pytest.mark.gpu
@pytest.mark.parametrize("grid,layout,track", FORMS)
def test_constructed_scenes_match_the_reference(grid, layout, track):
    """Every scene of the grid, every step, in one form of the batched step: every cell of every map at 1e-5 (assert_posteriors,
    strict), cells outside every op rectangle bit-equal to what was there, plans and deferred-clamp state word for word against the
    host model, S1 / S2 / both rewards within _check_env_step's bounds, tracked area sums within the streaming recomputation's
    bound, code tiles and published rectangles bit for bit, no fault, no rejected work list -- and the kernels the form names ran."""
    import torch
    g = geom(grid)
    run = Runner(grid, layout, track)
    env, E = run.env, run.E
    sim = Sim(grid)
    lc32 = float(np.float32(g.lc))
    assert env._tile_form == (g.d.vec == 4 and not g.shift)
    for t in range(g.steps):
        before_l, before_g = run.rows(env.local).clone(), run.rows(env.glob).clone()
        env.profile = t == 0
        run.fuse(t)
        plans, sums = sim.fuse(t)
        assert np.array_equal(env.comm.cpu().numpy(), np.stack([sc["comm"][t] for sc in run.scenes])), t
        raw_l, raw_g = run.rows(env.local), run.rows(env.glob)
        assert_maps(env.posterior_local().cpu().numpy(), sim.local, f"fused local maps, step {t}")
        assert_maps(env.posterior_global().cpu().numpy(), sim.glob, f"global maps, step {t}")
        keep = torch.from_numpy(~_op_mask(g, E, plans)).to(env.device)
        assert torch.equal(raw_l[keep[:, :N]], before_l[keep[:, :N]]) and torch.equal(raw_g[keep[:, N]], before_g[keep[:, N]]), t
        if track:
            run.check_area(f"fusion of step {t}")
        # plans and deferred-clamp state: the host model word for word; WS_FLAG_A from what the last op's rectangle holds on the device
        ws = env.ws.cpu().numpy()
        maps = np.concatenate([raw_l.cpu().numpy(), raw_g.cpu().numpy()[:, None]], axis=1)
        for e in range(E):
            for m, (ops, last, _, takes) in enumerate(plans[e]):
                st, w = sim.state[e][m], ws[e, m]
                tag = (run.scenes[e]["name"], t, m)
                assert w[8] == len(ops), tag
                if takes:
                    if ops:
                        assert w[13] == last, tag
                        got = [(int(w[16 + 8 * k]), int(w[17 + 8 * k]), tuple(int(v) for v in w[19 + 8 * k:23 + 8 * k])) for k in range(len(ops))]
                        assert got == [(tp, src, tuple(int(v) for v in r)) for tp, src, r in ops], tag
                    r = ops[last][2] if last >= 0 else None
                    cells = maps[e, m] if (g.shift and ops) else (maps[e, m, r[2]:r[3], r[0]:r[1]] if r else np.zeros(0))
                    st[0] = int(bool((np.abs(cells) > lc32).any()))
                assert list(w[0:6]) == st, (tag, list(w[0:6]), st)
        # K3 from the sense records
        mid_l = raw_l.clone()
        run.sense(t)
        obs = sim.sense(t)
        if t == 0:
            env.profile = False
            times = env.event_times_us()
            assert (times["fuse"]["kernel"], times["sense"]["kernel"]) == _kernels(grid, layout, track), times
        raw_l = run.rows(env.local)
        assert_maps(env.posterior_local().cpu().numpy(), sim.local, f"local maps after K3, step {t}")
        assert torch.equal(run.rows(env.glob), raw_g), t
        rects = run.rects[:, t + 1].cpu().numpy()
        assert np.array_equal(env.rect.cpu().numpy(), rects), t
        inside = np.zeros((E, N, g.gx, g.gy), dtype=bool)
        code, maps, ws1 = env.code.cpu().numpy(), raw_l.cpu().numpy(), env.ws.cpu().numpy()
        for e in range(E):
            for i in range(N):
                yu, yd, xl, xr = r = rects[e, i]
                if _some(r):
                    inside[e, i, xl:xr, yu:yd] = True
                    assert np.array_equal(env.d.unpack_tile(r, code[e, i]), obs[e][i]), (run.scenes[e]["name"], t, i)
                    if (np.abs(maps[e, i, xl:xr, yu:yd]) > lc32).any():
                        sim.state[e][i][5] = 1
                assert list(ws1[e, i, 0:6]) == sim.state[e][i], (run.scenes[e]["name"], t, i, list(ws1[e, i, 0:6]), sim.state[e][i])
        keep = torch.from_numpy(~inside).to(env.device)
        assert torch.equal(raw_l[keep], mid_l[keep]), t
        if track:
            run.check_area(f"sensing of step {t}")
        # the step's reward, completed by K3
        got_s, got_r = env.sums[:, :2].cpu().numpy(), env.reward.cpu().numpy()
        for e in range(E):
            s1, s2 = sums[e]
            rel, ab = rewards_of(g, s1, s2)
            tag = f"{run.scenes[e]['name']} step {t}"
            np.testing.assert_allclose(got_s[e], [s1, s2], rtol=RTOL, atol=sums_atol(g, s2), err_msg=tag)
            np.testing.assert_allclose(got_r[e, 0], rel, rtol=RTOL, atol=1e-6 + RTOL * 0.5, err_msg=tag)
            np.testing.assert_allclose(got_r[e, 1], ab, rtol=RTOL, atol=1e-6 + RTOL * 0.17, err_msg=tag)
    assert env.counters()["work_list_rejects"] == 0 and int(env.fault.abs().sum()) == 0


# grid -> the forms that must agree bit for bit: (layout, area sums tracked, stand-alone entry points)
AGREE = {
    "48": [("rows", False, False), ("rows", True, False), ("tiles", False, False), ("tiles", True, False), ("rows", False, True), ("tiles", False, True)],
    "46": [("rows", False, False), ("rows", True, False), ("rows", False, True)],
    "128": [("rows", False, False), ("rows", True, False), ("rows", False, True)],
    "34": [("rows", False, False), ("rows", True, False), ("rows", False, True)],
    "48p": [("rows", False, False), ("rows", True, False), ("rows", False, True)],
    "128x512": [("rows", False, False), ("tiles", False, False), ("rows", False, True)],
    "256x512": [("rows", False, False), ("rows", False, True)],
    "204x512": [("rows", False, False), ("rows", False, True)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("grid", list(AGREE))
def test_forms_agree_bit_for_bit(grid):
    """The same scenes in every form of a grid, in lock step: tile items against the row walker (the stand-alone ippm_fuse_local +
    ippm_fuse_global_reward run k_fuse_rows on every grid), rows against tile storage, tracked against untracked, batched against
    stand-alone -- every cell of every map bitwise after every fusion and every sensing, the deferred-clamp state and the code tiles
    too; reward sums to the summation order of their float64 atomics."""
    import torch
    g = geom(grid)
    runs = [Runner(grid, *form) for form in AGREE[grid]]
    first = runs[0]
    for t in range(g.steps):
        for phase in ("fuse", "sense"):
            for form, run in zip(AGREE[grid], runs):
                run.env.profile = form[2] and t == 0 and phase == "fuse"
                getattr(run, phase)(t)
                if run.env.profile:      # the stand-alone entry points are the row walker, whatever the grid
                    assert run.env.event_times_us()["fuse"]["kernel"].startswith("k_fuse_rows<"), form
            for form, run in zip(AGREE[grid][1:], runs[1:]):
                tag = (grid, form, t, phase)
                assert torch.equal(run.rows(run.env.local), first.rows(first.env.local)), tag
                assert torch.equal(run.rows(run.env.glob), first.rows(first.env.glob)), tag
                assert torch.equal(run.env.ws[..., 0:6], first.env.ws[..., 0:6]), tag
                assert torch.equal(run.env.comm, first.env.comm), tag
                if phase == "sense":
                    assert torch.equal(run.env.code, first.env.code) and torch.equal(run.env.rect, first.env.rect), tag
                    # (T is seeded by ippm_weighted_entropy's float32 block sums in storage order: test_tile_storage's bound)
                    torch.testing.assert_close(run.env.sums[:, :3], first.env.sums[:, :3], rtol=1e-6, atol=1e-6)
                    torch.testing.assert_close(run.env.reward, first.env.reward, rtol=1e-6, atol=1e-6)
    for run in runs:
        assert run.env.counters()["work_list_rejects"] == 0 and int(run.env.fault.abs().sum()) == 0
