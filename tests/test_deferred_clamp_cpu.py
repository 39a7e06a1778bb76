"""The deferred clamp's bookkeeping on the NumPy model (tests/deferred_clamp_ref.py): plans that defer their clamp-only ops and a
settle before every look must show exactly the maps of the plans that clip at once -- and both the maps of the reference's full-grid clip."""
import numpy as np
import pytest

from deferred_clamp_ref import LC, Literal, Planned, random_events


def run(events, model, defer_policy):
    """Plays `events` into `model`; `defer_policy(step_no, looked_since_last_plan)` -> whether the plan defers.  -> the maps at the looks."""
    seen, looked, k = [], True, 0
    for ev in events:
        if ev[0] == "look":
            model.settle()
            seen.append(model.L.copy())
            looked = True
        elif ev[0] == "sense":
            model.sense(ev[1], ev[2])
        else:
            model.plan_and_fuse(ev[1], defer=defer_policy(k, looked))
            looked = False
            k += 1
    return seen


def as_host(k, looked):      # VecEnv: a step that follows a look at the maps plans as ever
    return not looked


@pytest.mark.parametrize("seed", range(40))
def test_random_sequences_deferred_and_settled_equal_eager_and_literal(seed):
    rng = np.random.default_rng(seed)
    events = random_events(rng, steps=int(rng.integers(6, 30)))
    lit = run(events, Literal(), as_host)
    eager_model, defer_model = Planned(cap=None), Planned(cap=64)
    eager = run(events, eager_model, as_host)
    always = Planned(cap=64)
    deferred_always = run(events, always, lambda k, looked: True)
    deferred = run(events, defer_model, as_host)
    assert len(lit) == len(eager) == len(deferred) >= 1
    for a, b, c, d in zip(lit, eager, deferred, deferred_always):
        assert np.array_equal(a, b)          # the eager plans ARE the full-grid clip
        assert np.array_equal(b, c)
        assert np.array_equal(b, d)
    assert eager_model.flags() == defer_model.flags() == always.flags()
    assert always.fused_cells <= eager_model.fused_cells


def test_deferral_is_exercised_by_the_random_sequences():
    """Not vacuous: over the seeds above, deferring plans exist, their fusions touch fewer cells, and settles change cells."""
    fused_e = fused_d = settled = plans = 0
    for seed in range(40):
        rng = np.random.default_rng(seed)
        events = random_events(rng, steps=int(rng.integers(6, 30)))
        e, d = Planned(cap=None), Planned(cap=64)
        run(events, e, as_host)
        run(events, d, as_host)
        fused_e += e.fused_cells
        fused_d += d.fused_cells
        settled += d.settled_cells
        plans += d.plans_deferred
    assert plans > 100 and settled > 1000 and fused_d < 0.95 * fused_e


def test_gap_between_two_left_behind_footprints_is_clipped():
    """Two far-apart footprints left behind while the agent hears nobody: RECT_A is their hull, and an owed out-of-range cell lies in the
    hull's gap.  A settle that took the hull for legitimately unclamped would leave that cell out of range."""
    far = 30.0
    gap_fp, fp1, fp2 = (12, 18, 12, 18), (0, 5, 0, 5), (26, 31, 26, 31)
    msg = ((0, 4, 28, 32), 4.0)                        # a message that meets none of the above

    def events():
        return [("sense", gap_fp, far),               # out of range in the middle of the map, FLAG_S
                ("fuse", [msg]),                       # takes a message: the footprint is owed a clip (eager: clamp-only op)
                ("sense", fp1, far), ("fuse", []),     # hears nobody twice: the two footprints are left behind, unclamped
                ("sense", fp2, far), ("fuse", []),
                ("sense", (20, 24, 2, 6), 2.0),
                ("look",)]
    eager, d = Planned(cap=None), Planned(cap=16)
    want = run(events(), eager, lambda k, looked: False)[0]
    m = run(events(), d, lambda k, looked: True)
    # before the settle the cell was still out of range, inside the hull of what was left behind
    assert d.rect_a == (0, 31, 0, 31) and d.legit == [fp1, fp2]
    assert d.settled_cells == 36
    assert np.array_equal(m[0], want)
    assert abs(want[14, 14]) == np.float32(LC) and want[2, 2] == np.float32(far) and want[28, 28] == np.float32(far)
    # ... and the wrong settle (the hull as legit) is told apart by this scenario
    wrong = Planned(cap=16)
    wrong.legit_rects = lambda: [wrong.rect_a]
    assert not np.array_equal(run(events(), wrong, lambda k, looked: True)[0], want)


def test_legit_overflow_falls_back_to_the_eager_plan():
    """More footprints left behind than the list holds: the list is marked incomplete, the next plan that takes messages ignores
    `defer`, clips the hull (and whatever was owed) itself and starts a fresh list."""
    cap = 3
    ev = [("sense", (1, 4, 1, 4), 30.0)]
    for k in range(5):                                 # five left-behind footprints, a list of three
        ev += [("fuse", []), ("sense", (2 + 5 * k, 6 + 5 * k, 8, 12), 30.0)]
    ev += [("look",), ("fuse", [((20, 26, 20, 26), 30.0)]), ("sense", (0, 3, 28, 31), 30.0), ("look",),
           ("fuse", [((10, 14, 2, 6), 4.0)]), ("sense", (5, 9, 5, 9), 30.0), ("look",)]
    eager, d = Planned(cap=None), Planned(cap=cap)
    want = run(ev, eager, lambda k, looked: False)
    seen, looked, k, overflowed_at_plan = [], True, 0, None
    for e in ev:
        if e[0] == "look":
            d.settle()
            seen.append(d.L.copy())
        elif e[0] == "sense":
            d.sense(e[1], e[2])
        else:
            if e[1] and overflowed_at_plan is None:
                overflowed_at_plan = d.overflowed
                before = d.plans_deferred
                d.plan_and_fuse(e[1], defer=True)
                assert d.plans_deferred == before and not d.overflowed and d.legit == [] and d.owed is None   # the eager path was taken
                continue
            d.plan_and_fuse(e[1], defer=True)
    assert overflowed_at_plan is True
    assert d.plans_deferred == 1                        # the plan after the fallback defers again
    for a, b in zip(want, seen):
        assert np.array_equal(a, b)
    assert eager.flags() == d.flags()


@pytest.mark.parametrize("kind", ["end", "every4"])
def test_gpu_scenario_leaves_owed_cells_at_its_looks(kind):
    """The episodes tests/test_hip_deferred_clamp.py flies, with the oracle's geometry (footprints, who hears whom) and one log-odds
    step per look by altitude in place of the measurements: at the looks of its cases (a) and (b) the settles change cells in every
    env, the deferring fusions touch fewer cells, and the maps equal the eager model's."""
    import ipp_oracle as O
    from deferred_clamp_scenario import E, N, oracle_episodes, read_points, scenario_params
    d = O.Derived(scenario_params())
    T = d.budget + 1
    step = {5: 4.595, 10: 1.02, 15: 0.511}              # ln((1 - noise) / noise) of O.noise_of_altitude
    reads = read_points(kind, T)
    for e, run_ in enumerate(oracle_episodes((5, 6, 7))):
        dm = [Planned(n=d.gx, cap=d.budget + 2) for _ in range(N + 1)]
        em = [Planned(n=d.gx, cap=None) for _ in range(N + 1)]
        looked = True
        for t, rec in enumerate(run_["log"]):
            rects = [tuple(int(v) for v in r) for r in rec["rects"]]
            lm = [step[int(z)] for z in rec["positions"][:, 2]]
            if t == 0:
                for i in range(N):
                    dm[i].sense(rects[i], lm[i])
                    em[i].sense(rects[i], lm[i])
            for maps, defer in ((dm, not looked), (em, False)):
                for i in range(N):
                    maps[i].plan_and_fuse([(rects[j], lm[j]) for j in sorted(rec["received"][i]) if j != i], defer=defer)
                maps[N].plan_and_fuse([(rects[j], lm[j]) for j in range(N)], defer=defer)
            looked = False
            for i in range(N):
                r, z = tuple(int(v) for v in rec["next_rects"][i]), int(rec["next_positions"][i, 2])
                dm[i].sense(r, step[z])
                em[i].sense(r, step[z])
            if t in reads:
                for a, b in zip(dm, em):
                    a.settle()
                    assert np.array_equal(a.L, b.L)
                looked = True
        assert sum(m.settled_cells for m in dm) > 0, f"env {e}: nothing owed at the looks"
        assert sum(m.fused_cells for m in dm) < sum(m.fused_cells for m in em), f"env {e}: nothing deferred"


def test_episode_long_list_never_overflows_under_the_host_rule():
    """VecEnv's rule: the list holds budget + 2 rectangles; plans 1 .. budget + 1 since a reset may defer, from plan budget + 2 on the env
    settles first and plans as ever.  Sequences of 3 x budget steps in which the agent mostly hears nobody stay exact."""
    budget = 7
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        events = random_events(rng, steps=3 * budget, p_alone=0.8, p_look=0.1)
        eager, d = Planned(cap=None), Planned(cap=budget + 2)
        want = run(events, eager, as_host)

        def host(k, looked, d=d):
            if k + 1 > budget + 1:
                d.settle()
                return False
            return not looked
        got = run(events, d, host)
        for a, b in zip(want, got):
            assert np.array_equal(a, b)
        assert len(d.legit) <= budget + 2
