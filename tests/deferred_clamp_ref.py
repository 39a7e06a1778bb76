"""NumPy model of the deferred clamp's BOOKKEEPING (csrc/step_small.hip plan_map, csrc/settle.hip), one map.

Three ways to keep one belief map through the same sequence of events:

  literal   the reference: a fusion clips EVERY cell of the map before every op; only the outputs of its last op can stay out of range
  eager     the plans as they always were: flagged rectangles (region A, the agent's last footprint) become clamp-only ops ahead of a
            fusion's real ops
  deferring a plan made with `defer` pushes no clamp-only op: the rectangles join the backlog's OWED box, `settle()` clips the cells of the
            box that are not legitimately unclamped when somebody looks

Events: `sense(rect, delta)` (K3: clip the input inside the footprint, add), `plan_and_fuse(ops, defer)` with ops = [(rect, delta), ...]
(empty: the agent heard nobody), `settle()`.  Rectangles are (yu, yd, xl, xr): columns [yu, yd) x rows [xl, xr).  Only what decides
WHICH cells are clipped WHEN is modelled -- no measurements, no lanes, no 4-cell groups."""
import numpy as np

LC = 9.21   # the clip bound in log-odds, ln(0.9999 / 0.0001) to three digits: any value will do


def _empty(r):
    return r is None or r[1] <= r[0] or r[3] <= r[2]


def _hull(a, b):
    if _empty(a):
        return b
    if _empty(b):
        return a
    return (min(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3]))


def _sl(r):
    return (slice(r[2], r[3]), slice(r[0], r[1]))


class Literal:
    """The reference's recursion: full-grid clip at every op of a fusion."""

    def __init__(self, n=32):
        self.L = np.zeros((n, n), dtype=np.float32)

    def sense(self, rect, delta):
        s = _sl(rect)
        self.L[s] = np.clip(self.L[s], -LC, LC) + delta

    def plan_and_fuse(self, ops, defer=False):
        for rect, delta in ops:
            self.L = np.clip(self.L, -LC, LC)
            self.L[_sl(rect)] += delta

    def settle(self):
        pass


class Planned:
    """The planner's bookkeeping: ws flags / RECT_A as plan_map keeps them, and (cap is not None) the clamp backlog."""

    def __init__(self, n=32, cap=None):
        self.L = np.zeros((n, n), dtype=np.float32)
        self.flag_a, self.rect_a, self.flag_s, self.rect_s = False, None, False, None
        self.cap = cap                       # None: no backlog registered
        self.owed, self.legit, self.overflowed = None, [], False
        self.fused_cells = 0                 # cells the fusions loaded and stored
        self.settled_cells = 0               # cells a settle changed
        self.plans_deferred = 0

    # K3: clips its input inside the footprint, adds; remembers the footprint if it left anything out of range
    def sense(self, rect, delta):
        s = _sl(rect)
        self.L[s] = np.clip(self.L[s], -LC, LC) + delta
        self.rect_s = rect
        self.flag_s = bool((np.abs(self.L[s]) > LC).any())

    def plan_and_fuse(self, ops, defer=False):
        ops = [(r, d) for r, d in ops if not _empty(r)] if ops else []
        if not ops:    # heard nobody: the map is untouched, the footprint left behind joins region A
            if self.flag_s:
                if self.cap is not None and not self.overflowed:
                    if not self.legit and self.flag_a:
                        self.legit.append(self.rect_a)      # RECT_A still is the last fusion's own rectangle
                    if len(self.legit) < self.cap:
                        self.legit.append(self.rect_s)
                    else:
                        self.overflowed = True
                self.rect_a = _hull(self.rect_a, self.rect_s) if self.flag_a else self.rect_s
                self.flag_a, self.flag_s = True, False
            return
        ca = self.rect_a if self.flag_a else None
        cs = self.rect_s if self.flag_s else None
        if self.cap is not None:
            if defer and not self.overflowed:
                self.owed = _hull(_hull(self.owed, ca), cs)
                ca = cs = None
                self.plans_deferred += 1
            else:
                ca = _hull(ca, self.owed)
                self.owed = None
            self.legit, self.overflowed = [], False
        touched = np.zeros(self.L.shape, dtype=bool)
        for r in (ca, cs):
            if not _empty(r):
                touched[_sl(r)] = True
                self.L[_sl(r)] = np.clip(self.L[_sl(r)], -LC, LC)
        for rect, delta in ops:           # every op clips its own input
            s = _sl(rect)
            touched[s] = True
            self.L[s] = np.clip(self.L[s], -LC, LC) + delta
        last = ops[-1][0]
        keep = np.zeros(self.L.shape, dtype=bool)
        keep[_sl(last)] = True
        out = touched & ~keep             # every stored cell but the last op's is clipped on output
        self.L[out] = np.clip(self.L[out], -LC, LC)
        self.fused_cells += int(touched.sum())
        self.rect_a = last
        self.flag_a = bool((np.abs(self.L[_sl(last)]) > LC).any())
        self.flag_s = False

    def legit_rects(self):
        """What is legitimately unclamped right now, as ippm_settle_clamps reads it."""
        rects = list(self.legit)
        if not self.legit and self.flag_a:
            rects.append(self.rect_a)
        if self.flag_s:
            rects.append(self.rect_s)
        return rects

    def settle(self):
        if self.cap is None or _empty(self.owed):
            return
        owed = np.zeros(self.L.shape, dtype=bool)
        owed[_sl(self.owed)] = True
        for r in self.legit_rects():
            owed[_sl(r)] = False
        clipped = np.clip(self.L, -LC, LC)
        self.settled_cells += int((owed & (clipped != self.L)).sum())
        self.L = np.where(owed, clipped, self.L)
        if not self.overflowed:
            self.owed = None

    def flags(self):
        return (self.flag_a, self.rect_a if self.flag_a else None, self.flag_s, self.rect_s if self.flag_s else None)


def random_rect(rng, n=32, lo=3, hi=12):
    h, w = int(rng.integers(lo, hi)), int(rng.integers(lo, hi))
    x, y = int(rng.integers(0, n - h + 1)), int(rng.integers(0, n - w + 1))
    return (y, y + w, x, x + h)


def random_events(rng, steps, n=32, p_alone=0.4, p_look=0.25):
    """A step = one plan (messages from up to three neighbours, or nobody), its fusion, then K3 at a new footprint.  The deltas push
    cells far past the bound (a noise-free sensor).  -> [("fuse", ops) | ("sense", rect, delta) | ("look",)]"""
    ev = [("sense", random_rect(rng, n), float(rng.choice([-30.0, 30.0])))]
    for _ in range(steps):
        if rng.random() < p_look:
            ev.append(("look",))
        k = 0 if rng.random() < p_alone else int(rng.integers(1, 4))
        ev.append(("fuse", [(random_rect(rng, n), float(rng.choice([-30.0, 30.0, 4.0]))) for _ in range(k)]))
        ev.append(("sense", random_rect(rng, n), float(rng.choice([-30.0, 30.0, 2.0]))))
    ev.append(("look",))
    return ev
