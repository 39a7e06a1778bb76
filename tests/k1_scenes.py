"""Constructed scenes for K1 (csrc/ippm_k1.h::k1_env: boundary mask, order-dependent collision mask, action choice, move, fault word)
and their expected results from the oracle alone.  Plain module: tests/test_k1_scenes_cpu.py asserts the census of what the scenes
reach, tests/test_hip_k1_constructed.py runs them on the device and compares bit for bit.

A scene is ONE env: start positions [N, 3], team size, policy, t, episode id, and ``probs`` or ``actions``.  The policy and t are
arguments of a launch, so the scenes of an action set are batched per (N, policy, t): ``groups()``.

Everything is built on the ``small`` parameter set (11 x 11 x 3 lattice, spacing 5 m, altitudes 5 / 10 / 15 m)."""
import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import ipp_oracle as O
from configs import make_params

SEED = 0x5EED1234567ABC            # Philox key with both halves set (the key words are seed and seed >> 32)
ACTION_SETS = (4, 6, 9, 27)
TEAMS = (1, 2, 3, 4, 16)           # the contexts' n_agents
FAULT_WORK_OVERFLOW = 0x40000000   # IPPM_FAULT_WORK_OVERFLOW (include/ippmarl.h): sticky bit of fault[e]
STALE = 0x2A5                      # empty-mask bits "left over from the last step" that this step must replace
POLICY_EXPLICIT, POLICY_UNIFORM, POLICY_SAMPLE, POLICY_ARGMAX = 0, 1, 2, 3
# episode ids below and above 2^32 (the Philox counter takes ep and ep >> 32)
EPISODES = (0, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 2 ** 40 + 3, 2 ** 62 + 1)
MUTANTS = ("no_guard", "j_le_i", "col27_4_only")   # one-line changes of K1 the scenes must notice (tests/test_k1_scenes_cpu.py)


def params_for(A: int, N: int):
    return make_params("small", experiment__constraints__num_actions=A, experiment__missions__n_agents=N)


@functools.lru_cache(maxsize=None)
def derived(A: int) -> O.Derived:
    return O.Derived(params_for(A, 4))   # (nothing the scenes use depends on the team size)


@dataclass
class Scene:
    family: str
    pos: np.ndarray                      # [N, 3] int
    policy: int
    t: int = 0
    ep: int = 1
    n_active: Optional[int] = None       # None: all N fly
    actions: Optional[np.ndarray] = None  # [N] (policy 0)
    probs: Optional[np.ndarray] = None   # [N, A] float32 (policies 2, 3)
    fault0: int = 0                      # fault[e] before the step
    tags: tuple = field(default_factory=tuple)

    @property
    def N(self):
        return len(self.pos)

    @property
    def n(self):
        return self.N if self.n_active is None else self.n_active


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle's evaluation of one scene
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _boundary(A: int, p: tuple) -> np.ndarray:
    m = O.action_mask(derived(A), np.array(p))
    m.setflags(write=False)
    return m


def rule_key(A: int, rel) -> tuple:
    """What O.collision_rule looks at: the (dx, dy) offset for 4 / 6 / 9 actions (altitude ignored), (dx, dy, dz) for 27."""
    return (int(rel[0]), int(rel[1])) if A != 27 else (int(rel[0]), int(rel[1]), int(rel[2]))


@functools.lru_cache(maxsize=None)
def rule_keys(A: int):
    keys = set()
    for dx in range(-2, 3):
        for dy in range(-2, 3):
            for dz in range(-2, 3):
                if O.collision_rule(A, (dx, dy, dz)):
                    keys.add(rule_key(A, (dx, dy, dz)))
    return sorted(keys)


def _collide(d, A, p, m, other, mutant):
    """O.apply_collision_mask for one moved agent -- or one of the three one-line mutants of the device code."""
    if mutant is None or mutant == "j_le_i":
        return O.apply_collision_mask(d, p, m, [other])
    rel = O.position_to_index(d, other) - O.position_to_index(d, p)
    z = O.collision_rule(A, rel)
    if mutant == "col27_4_only" and A == 27 and z == [4, 22]:
        z = [4]
    if not z:
        return m
    if A == 6 and mutant != "no_guard":
        if np.sum(m) > 1:
            m[z] = 0
    elif A == 9:
        for a in z:
            m[a] = 0
            if np.count_nonzero(m) == 0:
                m[a] = 1
    else:
        m[z] = 0
    return m


def evaluate(A: int, sc: Scene, mutant: Optional[str] = None, events: Optional[list] = None):
    """(mask [N, A] uint8, action [N] int32, new positions [N, 3] int32, fault word) of the scene.  ``events``: a list that receives one
    record per (agent i, moved agent j < i) whose offset matches a collision rule, and one per agent (tests/test_k1_scenes_cpu.py)."""
    d = derived(A)
    N, n = sc.N, sc.n
    pos = np.array(sc.pos, dtype=np.int64)
    start = pos.copy()
    mask = np.zeros((N, A), dtype=np.uint8)
    act = np.zeros(N, dtype=np.int32)
    flt = 0
    for i in range(n):
        p = pos[i].copy()
        bm = _boundary(A, tuple(int(v) for v in p))
        m = bm.copy()
        for j in range(i + 1 if mutant == "j_le_i" else i):
            before = m.copy()
            m = _collide(d, A, p, m, pos[j], mutant)
            if events is not None:
                z = O.collision_rule(A, O.position_to_index(d, pos[j]) - O.position_to_index(d, p))
                z_pre = O.collision_rule(A, O.position_to_index(d, start[j]) - O.position_to_index(d, p))
                if z or z_pre:
                    events.append(dict(kind="pair", i=i, j=j, key=rule_key(A, O.position_to_index(d, pos[j]) - O.position_to_index(d, p)) if z else None,
                                       effect=bool((before != m).any()), pre=bool(z_pre), post=bool(z),
                                       guard_blocked=bool(z) and A == 6 and before.sum() <= 1 and any(before[a] for a in z),
                                       restored=bool(z) and A == 9 and before.sum() == 1 and before[z[0]] == 1))
        if events is not None:
            later = any(O.collision_rule(A, O.position_to_index(d, start[j]) - O.position_to_index(d, p)) for j in range(i + 1, n))
            events.append(dict(kind="agent", i=i, popcount=int(m.sum()), boundary_popcount=int(bm.sum()), later_adjacent=later,
                               unmasked=bool((m == bm).all())))
        if mutant is None and i > 0:   # the oracle's own call, all moved agents at once: the same thing
            assert np.array_equal(m, O.apply_collision_mask(d, p, bm.copy(), [pos[j] for j in range(i)]))
        a = -1
        if m.sum() == 0:
            flt |= 1 << i                       # the reference's torch.multinomial raises here
        elif sc.policy == POLICY_EXPLICIT:
            a = int(sc.actions[i])
        elif sc.policy == POLICY_UNIFORM:
            a = O.uniform_valid_action(O.philox_action_word(SEED, sc.ep, i, sc.t), m)
        elif sc.policy == POLICY_ARGMAX:
            a = int(np.argmax(sc.probs[i] * m))   # (0 when every valid action has probability 0 -- masked or not)
        else:
            try:
                a = O.sample_masked_action(O.philox_action_word(SEED, sc.ep, i, sc.t), (sc.probs[i] * m).astype(np.float32))
            except ValueError:
                flt |= 1 << i
        if a < 0 or a >= A:
            a = int(np.flatnonzero(bm)[0]) if bm.any() else 0   # keep the state sane: first boundary-valid action
        pos[i] = O.action_to_position(d, p, a)
        act[i] = a
        mask[i] = m.astype(np.uint8)
    return mask, act, pos.astype(np.int32), (sc.fault0 & FAULT_WORK_OVERFLOW) | flt


def on_lattice(A: int, pos) -> bool:
    d = derived(A)
    pos = np.asarray(pos)
    return bool((pos[:, 0] >= 0).all() and (pos[:, 0] <= d.x_dim_m).all() and (pos[:, 1] >= 0).all() and (pos[:, 1] <= d.y_dim_m).all()
                and (pos[:, 2] >= d.min_altitude).all() and (pos[:, 2] <= d.max_altitude).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------------------
def _cell(A, ix, iy, iz):
    d = derived(A)
    return np.array([ix * d.spacing, iy * d.spacing, d.min_altitude + iz * d.spacing], dtype=np.int64)


def _inside(A, p):
    return on_lattice(A, np.asarray(p)[None])


def approach(A, landing, pick=0):
    """(start, action) of an agent that lands on ``landing`` by a boundary-valid move; ``pick`` chooses among the possible ones.  None if the
    landing point is outside the lattice."""
    if not _inside(A, landing):
        return None
    off = O.action_offsets(A, derived(A).spacing)
    ways = [(np.asarray(landing) - off[a], a) for a in range(A) if off[a].any() and _inside(A, np.asarray(landing) - off[a])]
    return ways[pick % len(ways)]


def explicit(A, family, pos, lead=None, tags=(), **kw):
    """A policy-0 scene: agents named in ``lead`` take the given action, every other one the first action its own mask admits."""
    lead = lead or {}
    pos = np.array(pos, dtype=np.int64)
    sc = Scene(family, pos, POLICY_EXPLICIT, actions=np.zeros(len(pos), dtype=np.int32), tags=tuple(tags), **kw)
    for i in range(sc.n):
        if i in lead:
            sc.actions[i] = lead[i]
        else:   # (the mask of agent i depends on the moves of the agents before it only)
            m, _, _, _ = evaluate(A, Scene(family, pos[:i + 1], POLICY_EXPLICIT, actions=sc.actions[:i + 1]))
            sc.actions[i] = int(np.flatnonzero(m[i])[0]) if m[i].any() else 0
    return sc


def boundary_scenes(A):
    """One agent on every one of the 363 lattice points; one env per boundary-valid move of the point."""
    d = derived(A)
    out = []
    for ix in range(d.space_x):
        for iy in range(d.space_y):
            for iz in range(d.space_z):
                p = _cell(A, ix, iy, iz)
                for a in np.flatnonzero(_boundary(A, tuple(int(v) for v in p))):
                    out.append(Scene("boundary", p[None], POLICY_EXPLICIT, actions=np.array([a], dtype=np.int32)))
    return out


def border_classes(A):
    """Agent 1's places in the pair scenes: every combination of {low border, interior, high border} per axis (the first one listed is the
    interior)."""
    d = derived(A)
    xs, ys, zs = (0, d.space_x // 2, d.space_x - 1), (0, d.space_y // 2, d.space_y - 1), (0, d.space_z // 2, d.space_z - 1)
    cells = [(x, y, z) for x in xs for y in ys for z in zs]
    interior = (xs[1], ys[1], zs[1])
    return [interior] + [c for c in cells if c != interior]


def pair_scenes(A):
    """Agent 0, driven by an explicit action, lands at every lattice offset {-2..2}^2 x {every level} from agent 1."""
    d = derived(A)
    out = []
    for k, (x1, y1, z1) in enumerate(border_classes(A)):
        p1 = _cell(A, x1, y1, z1)
        for ox in range(-2, 3):
            for oy in range(-2, 3):
                for lz in range(d.space_z):
                    way = approach(A, _cell(A, x1 + ox, y1 + oy, lz), pick=k + ox + 5 * oy + lz)
                    if way is None:
                        continue
                    out.append(explicit(A, "pairs", [way[0], p1], lead={0: way[1]}, tags=(("offset", (ox, oy, lz - z1)),)))
    return out


def _key_cell(A, centre, key, lz=None):
    dz = key[2] if len(key) == 3 else 0
    return _cell(A, centre[0] + key[0], centre[1] + key[1], (centre[2] + dz) if lz is None else lz)


def chain_scenes(A):
    """Three and four agents: masks that accumulate over several j < i, the same rule met twice, neighbours adjacent only before or only
    after their own move, adjacent agents that come later in the order, and every scene again with the agent order reversed."""
    d = derived(A)
    keys = rule_keys(A)
    mid = (d.space_x // 2, d.space_y // 2, d.space_z // 2)
    out = []
    # the same rule twice: agents 0 and 1 both land at the offset `key` from agent 2 -> the second match changes nothing
    for k, key in enumerate(keys):
        w0, w1 = approach(A, _key_cell(A, mid, key), pick=k), approach(A, _key_cell(A, mid, key), pick=k + 3)
        out.append(explicit(A, "chains", [w0[0], w1[0], _cell(A, *mid)], lead={0: w0[1], 1: w1[1]}, tags=("twice",)))
    # three different neighbours of agent 3, in the interior and in the corner (where the boundary mask has few bits already)
    for centre in (mid, (0, 0, 0), (d.space_x - 1, d.space_y - 1, d.space_z - 1), (0, d.space_y - 1, 1)):
        near = [key for key in keys if _inside(A, _key_cell(A, centre, key))]
        for k in range(len(near)):
            trio = [near[k], near[(k + 1) % len(near)], near[(k + 2) % len(near)]]
            ways = [approach(A, _key_cell(A, centre, key), pick=k + q) for q, key in enumerate(trio)]
            out.append(explicit(A, "chains", [w[0] for w in ways] + [_cell(A, *centre)], lead={q: w[1] for q, w in enumerate(ways)},
                                tags=("accumulate",)))
    # the 6-action guard (popc(m) > 1, once per rule) and the 9-action restore: corner agents whose mask is down to one bit
    if A == 6:
        for lz in range(d.space_z):   # bottom corner: up, +y, +x -> one bit left when the same-column rule arrives
            ways = [approach(A, _cell(A, 1, 0, lz)), approach(A, _cell(A, 0, 1, lz)), approach(A, _cell(A, 0, 0, (lz + 1) % d.space_z), pick=lz)]
            for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
                out.append(explicit(A, "chains", [ways[q][0] for q in order] + [_cell(A, 0, 0, 0)], lead={s: ways[q][1] for s, q in enumerate(order)},
                                    tags=("guard",)))
    if A == 9:
        for corner, offs in (((0, 0, 1), ((0, 1), (1, 0), (1, 1))), ((d.space_x - 1, 0, 0), ((-1, 0), (-1, 1), (0, 1)))):
            for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
                ways = [approach(A, _cell(A, corner[0] + offs[q][0], corner[1] + offs[q][1], corner[2]), pick=q) for q in order]
                out.append(explicit(A, "chains", [w[0] for w in ways] + [_cell(A, *corner)], lead={s: w[1] for s, w in enumerate(ways)},
                                    tags=("restore",)))
    # adjacent only BEFORE its own move (agent 0 steps away from agent 2) / only AFTER it (agent 1 steps up to agent 2)
    off = O.action_offsets(A, d.spacing)
    find = lambda v: next(a for a in range(A) if tuple(off[a]) == tuple(np.array(v) * d.spacing))  # noqa: E731
    for centre in (mid, (2, 3, 0)):
        c = np.array(centre)
        out.append(explicit(A, "chains", [_cell(A, *(c + (1, 0, 0))), _cell(A, *(c + (0, 2, 0))), _cell(A, *c)],
                            lead={0: find((1, 0, 0)), 1: find((0, -1, 0))}, tags=("before_after",)))
        out.append(explicit(A, "chains", [_cell(A, *(c + (0, -1, 0))), _cell(A, *(c + (-2, 0, 0))), _cell(A, *c)],
                            lead={0: find((0, -1, 0)), 1: find((1, 0, 0))}, tags=("before_after",)))
    # an adjacent agent that comes LATER in the order has no effect: agent 0 keeps its boundary mask
    for key in keys[:: max(1, len(keys) // 4)]:
        out.append(explicit(A, "chains", [_cell(A, *mid), _key_cell(A, mid, key), _key_cell(A, mid, keys[-1])], tags=("later",)))
    # every scene again in reverse order (stale empty-mask bits in the fault word: this step must clear them)
    for sc in list(out):
        out.append(explicit(A, "chains", sc.pos[::-1], tags=sc.tags + ("reversed",), fault0=STALE))
    return out


def block16(A):
    """Sixteen agents, one lattice cell apart in a 4 x 4 block on alternating levels: every agent but the first has moved neighbours."""
    d = derived(A)
    return np.array([_cell(A, 3 + k // 4, 4 + k % 4, (k + k // 4) % d.space_z) for k in range(16)])


def team16_scenes(A):
    out = [explicit(A, "team16", block16(A)), explicit(A, "team16", block16(A)[::-1]),
           explicit(A, "team16", np.array([_cell(A, 0, 0, 0)] * 16))]        # all sixteen in one corner cell
    for k, ep in enumerate(EPISODES):
        out.append(Scene("choice", block16(A)[:: 1 if k % 2 else -1], POLICY_UNIFORM, t=(0, derived(A).budget)[k % 2], ep=ep))
    return out


def empty_mask_scenes(A):
    """Everything blocked: fault bit i, mask row all zero, move = first boundary-valid action.  fault[e] starts at the work-list overflow
    bit plus stale bits: the former is kept, the latter are replaced.  (9 actions cannot get there: the restore rule.)"""
    d = derived(A)
    top = d.space_z - 1
    if A == 4:
        ways = [approach(A, _cell(A, 1, 0, 1)), approach(A, _cell(A, 0, 1, 0))]
        pos, lead = [w[0] for w in ways] + [_cell(A, 0, 0, 2)], {q: w[1] for q, w in enumerate(ways)}
    elif A == 6:
        ways = [approach(A, _cell(A, 1, 0, 2)), approach(A, _cell(A, 0, 1, 0)), approach(A, _cell(A, 0, 0, 1))]
        pos, lead = [w[0] for w in ways] + [_cell(A, 0, 0, 1)], {q: w[1] for q, w in enumerate(ways)}
    elif A == 27:
        ways = [approach(A, _cell(A, 0, 1, top)), approach(A, _cell(A, 1, 0, top - 1)), approach(A, _cell(A, 1, 1, top)),
                approach(A, _cell(A, 0, 0, top - 1), pick=2)]
        fill = [_cell(A, 2 * k % 10, 6 + 2 * (k // 5), k % 3) for k in range(11)]   # eleven more, two cells apart, far from the corner
        pos, lead = [w[0] for w in ways] + fill + [_cell(A, 0, 0, top)], {q: w[1] for q, w in enumerate(ways)}
    else:
        return []
    base = explicit(A, "empty", pos, lead=lead, fault0=FAULT_WORK_OVERFLOW | STALE)
    i = base.N - 1
    onehot = np.zeros((base.N, A), dtype=np.float32)
    onehot[np.arange(base.N), base.actions] = 1.0          # (policies 2 / 3 then repeat the explicit scene's moves)
    return [base, Scene("empty", base.pos, POLICY_SAMPLE, probs=onehot, fault0=FAULT_WORK_OVERFLOW | STALE, ep=EPISODES[4], t=d.budget),
            Scene("empty", base.pos, POLICY_ARGMAX, probs=onehot, fault0=STALE | (1 << i)),
            Scene("empty", base.pos, POLICY_ARGMAX, probs=onehot, fault0=0, t=d.budget)]


@functools.lru_cache(maxsize=None)
def u_extremes():
    """(word >> 8, episode, agent, t) with the smallest and the largest u among 2^20 Philox action words: episodes 0 .. 2^18 - 1, agents 0
    and 1, t = 0 and the budget (the vectorised O.philox4x32)."""
    budget = derived(4).budget
    ep = np.arange(2 ** 18, dtype=np.int64)[:, None, None]
    agent = np.arange(2, dtype=np.int64)[None, :, None]
    t = np.array([0, budget], dtype=np.int64)[None, None, :]
    stream = (agent & 0xFF) | ((t & 0xFFFF) << 8) | (O.DOMAIN_ACTION << 24)
    word = O.philox4x32(0, ep, stream, 0, SEED & 0xFFFFFFFF, (SEED >> 32) & 0xFFFFFFFF)[0]
    assert word.size == 2 ** 20
    u = word >> np.uint32(8)
    out = []
    for flat in (int(u.argmin()), int(u.argmax())):
        e, a, k = np.unravel_index(flat, u.shape)
        assert O.philox_action_word(SEED, int(e), int(a), int(t[0, 0, k])) == int(word[e, a, k])   # (the scalar restatement agrees)
        out.append((int(u[e, a, k]), int(e), int(a), int(t[0, 0, k])))
    return tuple(out)


def _bases(A):
    """Start positions of two agents for the choice scenes: far apart, adjacent, in one column, at borders and in corners."""
    d = derived(A)
    mx, my, top = d.space_x - 1, d.space_y - 1, d.space_z - 1
    cells = [((2, 2, 1), (8, 7, 1)), ((5, 5, 1), (6, 5, 1)), ((5, 5, 0), (5, 5, 1)), ((0, 0, 0), (mx, my, top)), ((0, 4, top), (1, 4, top)),
             ((mx, 0, 0), (mx, 1, 0)), ((3, my, 1), (3, my, 1)), ((0, 0, top), (0, 1, top)), ((4, 0, 0), (4, 1, 1)), ((mx, my, 0), (mx - 1, my - 1, 1))]
    return [np.array([_cell(A, *a), _cell(A, *b)]) for a, b in cells]


def choice_scenes(A, explicit_scenes):
    """Policy 1 on the positions of the explicit scenes (so on masks of every popcount they reach); policies 2 and 3 on probabilities with
    zeros, ties, one-hot rows, unnormalised totals, all mass on masked actions, and the two extreme draws."""
    d = derived(A)
    rng = np.random.RandomState(1000 + A)
    out = []
    for k, sc in enumerate(explicit_scenes):
        if sc.family == "boundary" and sc.actions[0] != np.flatnonzero(_boundary(A, tuple(int(v) for v in sc.pos[0])))[0]:
            continue   # (one policy-1 scene per lattice point, not one per move)
        out.append(Scene("choice", sc.pos, POLICY_UNIFORM, t=(0, d.budget)[k % 2], ep=EPISODES[k % len(EPISODES)] + (k // 7 if k % 7 < 2 else 0),
                         fault0=sc.fault0))
    bases = _bases(A)
    bm = lambda pos: np.array([_boundary(A, tuple(int(v) for v in p)) for p in pos], dtype=np.float32)  # noqa: E731
    k = 0
    for pos in bases:
        valid = bm(pos)
        pats = {}
        pats["zeros"] = np.where(np.arange(A)[None, :] % 2 == 0, 0.0, rng.random_sample((2, A))).astype(np.float32)
        pats["zeros2"] = np.where(np.arange(A)[None, :] % 3 != 1, 0.0, np.ones((2, 1))).astype(np.float32)
        for q in range(3):   # one-hot on the q-th / last boundary-valid action (collision-masked or not: the oracle decides)
            oh = np.zeros((2, A), dtype=np.float32)
            for i in range(2):
                v = np.flatnonzero(valid[i])
                oh[i, v[(q * 2 + i) % len(v)] if q < 2 else v[-1]] = 1.0
            pats[f"onehot{q}"] = oh
        dirichlet = rng.dirichlet(np.ones(A), size=2).astype(np.float32)
        pats["dirichlet"] = dirichlet
        pats["tiny"] = (dirichlet * np.float32(1e-30)).astype(np.float32)      # totals of 1e-30 and 1e30: the draw scales with the total
        pats["huge"] = (dirichlet * np.float32(1e30)).astype(np.float32)
        pats["masked"] = (1.0 - valid).astype(np.float32)                       # all mass on boundary-masked actions (or none at all)
        pats["ties"] = (rng.randint(0, 3, size=(2, A)) * 0.25).astype(np.float32)
        top = pats["ties"].copy()                                               # the largest probability sits on a masked action
        top[valid == 0] = 0.75
        pats["masked_max"] = top
        for name, probs in pats.items():
            assert probs.min() >= 0 and np.isfinite(probs).all() and (probs[probs > 0] >= 1e-36).all()   # (no denormals)
            for policy in (POLICY_SAMPLE, POLICY_ARGMAX):
                if policy == POLICY_ARGMAX and not (probs[0] * valid[0]).any():
                    # argmax(probs * mask) is 0 when every valid action has probability 0, masked or not: the move may leave the lattice.
                    # Only the LAST agent of an env is put there (nothing is defined for agents that meet a neighbour outside the world).
                    probs = probs.copy()
                    probs[0, np.flatnonzero(valid[0])[0]] = 0.5
                out.append(Scene("choice", pos, policy, t=(0, d.budget)[k // 2 % 2], ep=EPISODES[k % len(EPISODES)], probs=probs, tags=(name,)))
                k += 1
    # the smallest and the largest u of 2^20 candidates, on uniform and on random weights, every action boundary-valid for both agents
    for u, ep, agent, t in u_extremes():
        pos = np.array([_cell(A, 2, 2, 1), _cell(A, 8, 7, 1)])
        for probs in (np.full((2, A), 1.0 / A, dtype=np.float32), rng.dirichlet(np.ones(A), size=2).astype(np.float32),
                      np.where(np.arange(A)[None, :] < A - 1, 1.0, 0.0).astype(np.float32) * np.ones((2, 1), dtype=np.float32)):
            out.append(Scene("choice", pos, POLICY_SAMPLE, t=t, ep=ep, probs=probs, tags=(("u", u, agent),)))
        out.append(Scene("choice", pos, POLICY_UNIFORM, t=t, ep=ep, tags=(("u", u, agent),)))
    # sixteen agents under policies 2 and 3 (agent indices up to 15 in the stream word)
    for k, ep in enumerate(EPISODES[:4]):
        probs = rng.dirichlet(np.ones(A), size=16).astype(np.float32)
        out.append(Scene("choice", block16(A), POLICY_SAMPLE if k % 2 == 0 else POLICY_ARGMAX, t=(0, d.budget)[k // 2 % 2], ep=ep, probs=probs))
    return out


@functools.lru_cache(maxsize=None)
def scenes(A: int):
    """Every scene of the action set."""
    out = boundary_scenes(A) + pair_scenes(A) + chain_scenes(A) + team16_scenes(A) + empty_mask_scenes(A)
    out += choice_scenes(A, [sc for sc in out if sc.policy == POLICY_EXPLICIT])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def team_size_scenes(A: int):
    """The four-agent chain scenes with fewer agents flying: agents >= n_active do not move and raise no fault bit, however close they are."""
    out = []
    for k, sc in enumerate(s for s in chain_scenes(A) if s.N == 4):
        n = 1 + k % 4
        out.append(explicit(A, "teams", sc.pos, lead={i: int(sc.actions[i]) for i in range(n)}, n_active=n, fault0=STALE if k % 3 == 0 else 0))
        out.append(Scene("teams", sc.pos, POLICY_UNIFORM, t=derived(A).budget, ep=EPISODES[k % len(EPISODES)], n_active=n))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(A: int, which: str = "all"):
    """[(scene, mask, action, new positions, fault)] for ``scenes(A)`` (or ``team_size_scenes(A)``), evaluated once."""
    return tuple((sc,) + evaluate(A, sc) for sc in (scenes(A) if which == "all" else team_size_scenes(A)))


def groups(A: int, which: str = "all"):
    """{(N, policy, t): [index into expected(A, which)]}: the scenes that can share a launch (policy and t are launch arguments)."""
    out = {}
    for k, rec in enumerate(expected(A, which)):
        sc = rec[0]
        out.setdefault((sc.N, sc.policy, sc.t), []).append(k)
    return out


def batch_arrays(A: int, which, idx):
    """The device inputs and the expected outputs of the scenes ``idx`` as stacked arrays."""
    recs = [expected(A, which)[k] for k in idx]
    sc0 = recs[0][0]
    N = sc0.N
    out = dict(pos=np.stack([r[0].pos for r in recs]).astype(np.int32), episode=np.array([r[0].ep for r in recs], dtype=np.int64),
               fault0=np.array([r[0].fault0 for r in recs], dtype=np.int32), n_active=np.array([r[0].n for r in recs], dtype=np.int32),
               want_mask=np.stack([r[1] for r in recs]), want_action=np.stack([r[2] for r in recs]), want_pos=np.stack([r[3] for r in recs]),
               want_fault=np.array([r[4] for r in recs], dtype=np.int64).astype(np.int32), probs=None, actions=None)
    if sc0.policy == POLICY_EXPLICIT:
        out["actions"] = np.stack([r[0].actions for r in recs]).astype(np.int32)
    if sc0.policy in (POLICY_SAMPLE, POLICY_ARGMAX):
        out["probs"] = np.stack([r[0].probs for r in recs]).astype(np.float32)
    out["flying"] = np.arange(N)[None, :] < out["n_active"][:, None]
    return out
