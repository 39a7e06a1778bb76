"""Constructed positions, ranges and draws for the comm matrix (comm_pair in csrc/step_small.hip: k_comm behind ippm_comm_matrix, and
inline in k_plan_step with lanes as ordered pairs).  Plain module: tests/test_comm_scenes_cpu.py (census) and
tests/test_hip_comm_constructed.py (the device) import the same cases.

A CASE is one batch: E envs of N agents with positions written straight into `pos`, one configured range and failure rate (they are
members of the context), per-env float32 ranges or none (then cfg.comm_range, a double, decides), explicit draws or none (then
Philox), a stage t, episode ids, team sizes or none.  The expected [E, N, N] bytes are O.received_set per row with the same draws --
O.philox_comm_draw where the device draws -- and the range the device compares with: cfg.comm_range, or float(np.float32(r)).
Every comparison is bit for bit.

Families (cases()):
  range/...    pairs at every lattice offset of a 5 x 9 x 5 box (the Pythagorean (3,4,0), (0,3,4), (4,0,3) among them: 25.0 m), under
               cfg.comm_range = the distance of a target offset and its float64 neighbours (integer distances and sqrt(d2) of non-squares),
               range 0 and 100; per-env float32 ranges at the float32 nearest to each pair's own sqrt(d2) and its float32 neighbours;
  draws/...    explicit draws at the failure rate, its float64 neighbours, 0.0 and 1 - 2^-53, different for (i, j) and (j, i), with a
               co-located pair under a failing draw and a pair out of range under a passing one; failure rate 0 (draws moot);
  philox/...   failure rate = one of the batch's own Philox draws (a multiple of 2^-32: that pair passes with equality) and the next
               double above it (it fails); episode ids below and above 2^32, two of them equal in their low 32 bits; stages
               0, 1, 255, 256, 65535; 16 agents;
  team/...     1, 2, 8, 9, 16 agents (one pair, one sweep of 64 ordered pairs, two, four) and 1, 63, 64, 65 envs; team sizes
               0, 1, n - 1, n with a non-flying agent co-located with a flying one."""
import functools
import itertools

import numpy as np

import ipp_oracle as O
from configs import make_params

SEED = 0xC0337A7
SPACING = 5
BASE = (20, 20, 5)       # the first agent of a pair: offsets of 0 .. 4 / -4 .. 4 lattice steps and 0 .. 4 levels stay inside the 50 m world


def params_for(n_agents, comm_range, failure_rate):
    """The 128-cell grid with five altitudes (5 .. 25 m), so that every position of the box is a lattice point."""
    return make_params("small", experiment__missions__n_agents=int(n_agents), experiment__uav__communication_range=comm_range,
                       experiment__uav__failure_rate=failure_rate, experiment__uav__fix_range=True, experiment__constraints__max_altitude=25)


@functools.lru_cache(maxsize=None)
def philox_draw(episode, i, j, t):
    return O.philox_comm_draw(SEED, episode, i, j, t)


class Case:
    def __init__(self, name, n, comm_range, failure_rate, pos, t=0, episode=None, range32=None, draws=None, n_active=None):
        self.name, self.n, self.comm_range, self.failure_rate, self.t = name, int(n), float(comm_range), float(failure_rate), int(t)
        self.pos = np.ascontiguousarray(pos, dtype=np.int32)
        self.E = len(self.pos)
        assert self.pos.shape == (self.E, self.n, 3)
        self.episode = np.arange(3, 3 + self.E, dtype=np.int64) if episode is None else np.ascontiguousarray(episode, dtype=np.int64)
        self.range32 = None if range32 is None else np.ascontiguousarray(range32, dtype=np.float32)
        self.draws = None if draws is None else np.ascontiguousarray(draws, dtype=np.float64)
        self.n_active = None if n_active is None else np.ascontiguousarray(n_active, dtype=np.int32)
        # batched: the case also runs through VecEnv, whose per-env float32 range array always decides -- every case but those whose
        # cfg.comm_range is a double that no float32 equals (the float64 neighbours of a distance, sqrt(d2) of a non-square)
        self.batched = self.range32 is not None or float(np.float32(self.comm_range)) == self.comm_range
        assert self.draws is None or self.draws.shape == (self.E, self.n, self.n)
        assert (self.pos >= 0).all() and (self.pos[..., :2] <= 50).all() and (self.pos[..., 2] >= 5).all() and (self.pos[..., 2] <= 25).all()
        assert (self.pos % SPACING == 0).all()

    @property
    def params(self):
        return params_for(self.n, self.comm_range, self.failure_rate)

    def range_of(self, e):
        """The double the device compares the distance with."""
        return self.comm_range if self.range32 is None else float(np.float32(self.range32[e]))

    def draw(self, e, i, j):
        if self.draws is not None:
            return float(self.draws[e, i, j])
        return philox_draw(int(self.episode[e]), i, j, self.t)

    @functools.cached_property
    def expected(self):
        """uint8 [E, N, N]: O.received_set row by row; with team sizes, rows and columns >= n_active[e] are zero (the batched step)."""
        out = np.zeros((self.E, self.n, self.n), dtype=np.uint8)
        for e in range(self.E):
            na = self.n if self.n_active is None else int(self.n_active[e])
            positions = [self.pos[e, k].astype(np.int64) for k in range(na)]
            for i in range(na):
                draws = [self.draw(e, i, j) if self.failure_rate > 0 else 0.0 for j in range(na)]
                for j in O.received_set(positions, i, self.range_of(e), self.failure_rate, draws):
                    out[e, i, j] = 1
        return out

    @functools.cached_property
    def expected_whole_team(self):
        """What ippm_comm_matrix gives: it does not look at team sizes."""
        if self.n_active is None:
            return self.expected
        return Case(self.name, self.n, self.comm_range, self.failure_rate, self.pos, self.t, self.episode, self.range32, self.draws).expected


# ---------------------------------------------------------------------------------------------------------------------------------
# host model of comm_pair, and the changes the expected bytes must be able to tell apart
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("lt at range", "gt at failure rate", "d2 == 0 dropped", "i and j swapped in the counter", "episode truncated to 32 bits",
             "stage truncated to 8 bits", "float32 range not widened")


def model(case, mutate=None):
    """comm_pair for every ordered pair of a case (team sizes as the batched step applies them)."""
    out = np.zeros((case.E, case.n, case.n), dtype=np.uint8)
    f = case.failure_rate
    for e in range(case.E):
        na = case.n if case.n_active is None else int(case.n_active[e])
        if case.range32 is None:
            rng = case.comm_range
        else:
            rng = np.float32(case.range32[e]) if mutate == "float32 range not widened" else float(np.float32(case.range32[e]))
        ep = int(case.episode[e])
        for i in range(na):
            for j in range(na):
                d = case.pos[e, i].astype(np.int64) - case.pos[e, j].astype(np.int64)
                d2 = int((d * d).sum())
                u = 1.0
                if f > 0.0:
                    if case.draws is not None:
                        u = float(case.draws[e, i, j])
                    else:
                        a, b = (j, i) if mutate == "i and j swapped in the counter" else (i, j)
                        u = philox_draw(ep & 0xFFFFFFFF if mutate == "episode truncated to 32 bits" else ep, a, b,
                                        case.t & 0xFF if mutate == "stage truncated to 8 bits" else case.t)
                ok = d2 == 0 and mutate != "d2 == 0 dropped"
                if d2 > 0 or mutate == "d2 == 0 dropped":
                    dist = np.sqrt(np.float64(d2))
                    if mutate == "float32 range not widened" and case.range32 is not None:
                        near = np.float32(dist) <= rng       # the distance rounded to the range's format
                    else:
                        near = dist < rng if mutate == "lt at range" else dist <= rng
                    if near and (u > f if mutate == "gt at failure rate" else u >= f):
                        ok = True
                out[e, i, j] = 1 if ok else 0
    return out


def relations(case):
    """{("range" | "draw", "<" | "=" | ">", decides)} over the ordered pairs i != j of a case: how the distance stands to the range
    and the draw to the failure rate, and whether that relation alone decides the byte (the other condition holds)."""
    out = set()
    f = case.failure_rate
    for e in range(case.E):
        na = case.n if case.n_active is None else int(case.n_active[e])
        for i, j in itertools.permutations(range(na), 2):
            d = case.pos[e, i].astype(np.int64) - case.pos[e, j].astype(np.int64)
            d2 = int((d * d).sum())
            if d2 == 0:
                continue
            dist, rng = float(np.sqrt(np.float64(d2))), case.range_of(e)
            u = case.draw(e, i, j) if f > 0 else 1.0
            rel = lambda a, b: "<" if a < b else ("=" if a == b else ">")      # noqa: E731
            out.add(("range", rel(dist, rng), u >= f))
            if f > 0:
                out.add(("draw", rel(u, f), dist <= rng))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
OFFSETS = [(a, b, c) for a in range(5) for b in range(-4, 5) for c in range(5)]      # lattice steps; (0, 0, 0): co-located
TARGETS = [(1, 0, 0), (3, 4, 0), (0, 3, 4), (1, 2, 2), (2, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 0), (4, 4, 2)]


def _pairs():
    pos = np.zeros((len(OFFSETS), 2, 3), dtype=np.int32)
    pos[:, 0] = BASE
    pos[:, 1] = np.asarray(BASE) + SPACING * np.asarray(OFFSETS)
    return pos


def _d2(off):
    return SPACING * SPACING * sum(v * v for v in off)


def _lattice_team(n, E, seed):
    """E envs of n agents on distinct lattice points (agents 0 and n - 1 co-located in every third env)."""
    rs = np.random.RandomState(seed)
    pos = np.zeros((E, n, 3), dtype=np.int32)
    for e in range(E):
        pts = rs.permutation(11 * 11 * 5)[:n]
        pos[e, :, 0], pos[e, :, 1], pos[e, :, 2] = SPACING * (pts % 11), SPACING * ((pts // 11) % 11), 5 + SPACING * (pts // 121)
        if n > 1 and e % 3 == 0:
            pos[e, n - 1] = pos[e, 0]
    return pos


def _edge_draws(f):
    return [f, np.nextafter(f, 0.0), np.nextafter(f, 1.0), 0.0, 1.0 - 2.0 ** -53, 0.5 * f, 0.5 * (1.0 + f)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    pairs = _pairs()
    # ---- ranges: cfg.comm_range (a double) at a target's distance and its float64 neighbours
    seen = set()
    for off in TARGETS:
        d2 = _d2(off)
        if d2 in seen:
            continue
        seen.add(d2)
        r = float(np.sqrt(np.float64(d2)))
        for tag, v in (("at", r), ("below", float(np.nextafter(r, 0.0))), ("above", float(np.nextafter(r, np.inf)))):
            out.append(Case(f"range/cfg/{d2}/{tag}", 2, v, 0.0, pairs))
    out.append(Case("range/cfg/zero", 2, 0.0, 0.0, pairs))
    out.append(Case("range/cfg/100", 2, 100.0, 0.0, pairs))
    # ... per-env float32 ranges: the float32 nearest to each pair's own distance (widened, it lies just below, on or just above it)
    own = np.sqrt(np.array([_d2(o) for o in OFFSETS], dtype=np.float64)).astype(np.float32)
    for tag, v in (("nearest", own), ("below", np.nextafter(own, np.float32(-1))), ("above", np.nextafter(own, np.float32(np.inf)))):
        out.append(Case(f"range/float32/{tag}", 2, 25.0, 0.0, pairs, range32=np.maximum(v, np.float32(0))))
    # ---- explicit draws, different for (i, j) and (j, i)
    f = 0.35
    n = 4
    edge = _edge_draws(f)
    E = len(edge)
    pos = np.zeros((E, n, 3), dtype=np.int32)
    pos[:] = [(10, 10, 15), (10, 15, 15), (10, 10, 15), (50, 50, 25)]       # 0 and 2 co-located; 3 out of range (58.3 m)
    draws = np.zeros((E, n, n))
    for e in range(E):
        for i in range(n):
            for j in range(n):
                draws[e, i, j] = edge[(e + 2 * i + 3 * j + (1 if i > j else 0)) % len(edge)]
    draws[:, 0, 2], draws[:, 2, 0] = 0.0, np.nextafter(f, 0.0)             # co-located under failing draws
    draws[:, 0, 3], draws[:, 3, 0] = 1.0 - 2.0 ** -53, f                    # out of range under passing draws
    draws[:, 0, 1], draws[:, 1, 0] = f, np.nextafter(f, 0.0)               # 0 hears 1 with equality, 1 does not hear 0
    out.append(Case("draws/edges", n, 25.0, f, pos, draws=draws))
    out.append(Case("draws/moot", n, 25.0, 0.0, pos, draws=np.zeros_like(draws)))
    # ---- Philox draws: the failure rate is one of the batch's own draws, and the next double above it
    episodes = np.array([7, 2 ** 32 - 1, 2 ** 32 + 7, 2 ** 40 + 3, 5 * 2 ** 32 + 11], dtype=np.int64)     # (7 and 2^32 + 7: the same low word)
    team = _lattice_team(16, len(episodes), 99)
    for t, (e_star, i_star, j_star) in zip((0, 1, 255, 256, 65535), ((2, 15, 3), (0, 1, 14), (3, 12, 13), (2, 3, 15), (4, 15, 0))):
        u = O.philox_comm_draw(SEED, int(episodes[e_star]), i_star, j_star, t)
        assert 0.0 < u < 1.0 and (team[e_star, i_star] != team[e_star, j_star]).any()
        for tag, v in (("equal", u), ("above", float(np.nextafter(u, 1.0)))):
            c = Case(f"philox/t{t}/{tag}", 16, 100.0, v, team, t=t, episode=episodes)
            c.star = (e_star, i_star, j_star)
            out.append(c)
    # ---- team and batch sizes
    for n, E in ((1, 65), (2, 65), (8, 65), (9, 65), (16, 65), (9, 1), (9, 63), (9, 64)):
        out.append(Case(f"team/n{n}/E{E}", n, 15.0, 0.3, _lattice_team(n, E, 1000 + 17 * n + E), t=3))
    for n in (8, 9):
        E = 12
        pos = _lattice_team(n, E, 2000 + n)
        pos[:, n - 1] = pos[:, 0]                                             # the last agent sits on the first: it flies in some envs only
        sizes = np.array([(0, 1, n - 1, n)[e % 4] for e in range(E)], dtype=np.int32)
        out.append(Case(f"team/sizes/n{n}", n, 100.0, 0.3, pos, t=2, n_active=sizes))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


def published(c):
    """Published rectangles [E, N, 4] for the plans: the footprints of the positions, every fifth agent's left empty."""
    from ippmarl.derived import DerivedConstants
    d = DerivedConstants(c.params, philox_seed=SEED)
    rect = np.zeros((c.E, c.n, 4), dtype=np.int32)
    for e in range(c.E):
        for i in range(c.n):
            if (e + i) % 5 != 4:
                rect[e, i] = d.footprint(c.pos[e, i])[1]
    return rect


def plan_sources(c, comm, rect):
    """For every local map i of every env: the sources of the type-1 ops a plan built from row i of `comm` holds -- the set bits other
    than i, ascending, without agents whose published rectangle is empty (plan_model of test_hip_constructed_rects.py)."""
    out = []
    for e in range(c.E):
        na = c.n if c.n_active is None else int(c.n_active[e])
        out.append([[j for j in range(c.n) if j != i and comm[e, i, j] and rect[e, j, 1] > rect[e, j, 0] and rect[e, j, 3] > rect[e, j, 2]]
                    if i < na else [] for i in range(c.n)])
    return out
