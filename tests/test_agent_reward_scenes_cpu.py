"""What the constructed scenes of tests/agent_reward_scenes.py reach, and why their bounds can be asked of the device (no GPU):
the restatement against the oracle's own DeepQ path, the float32 restatement against half of every bound, the agreement of the
float32 log-odds class weight with the reference's probability rule on every constructed cell (nothing excused), the census of the
scene sets, and the one-line changes to the host model of the device code that the expected values must be able to tell apart."""
import numpy as np
import pytest

import agent_reward_scenes as A
import ipp_oracle as O
from agent_reward_scenes import F32, R
from configs import make_params

ALL_SETS = ["values128", "values_nf", "free_48"] + ["geometry_" + n for n in A.GEOMETRY]


def test_restatement_equals_the_oracles_deepq_path():
    """sums_ref / rewards_of against agent_rewards(ep, rec) as test_hip_deepq.py::oracle_deepq_episode uses it, on a few flown steps at
    prior 0.5 and 0.3: K = the step's global map, the footprints and bits read back from the agents' maps2communicate."""
    from test_deepq_golden import agent_rewards
    seed, episode = 0x5EED0DEE, 13
    for over, steps in ((dict(experiment__missions__n_agents=3), 3), (dict(experiment__missions__n_agents=3, mapping__prior=0.3), 2)):
        params = make_params("small", **over)
        g = A.Grid("flown", params)
        holder = {}

        def correctness(i, s, shape):      # (the production randomness, as oracle_deepq_episode draws it)
            pos = holder["ep"].agents[i]["position"]
            _, fc = O.project_field_of_view(holder["ep"].d, pos)
            return O.philox_correctness(seed, episode, i, s, fc, holder["ep"].d.gy, O.noise_of_altitude(pos[2]))

        ep = O.OracleEpisode(params, episode, correctness,
                             lambda i, t, mask, obs: O.uniform_valid_action(O.philox_action_word(seed, episode, i, t), mask),
                             comm_draw=lambda i, j, t: O.philox_comm_draw(seed, episode, i, j, t), build_features=False, exact=True)
        holder["ep"] = ep
        for t in range(steps):
            rec = ep.step(t)
            want_r, want_s = agent_rewards(ep, rec)
            K = np.asarray(rec["global_map"], dtype=np.float64)
            with np.errstate(divide="ignore"):
                L = np.log(K) - np.log1p(-K)
            rects, bits, lm = [], [], []
            for i, pos in enumerate(rec["next_positions"]):
                yu, yd, xl, xr = r = g.d.footprint(pos)[1]
                k = (int(pos[2]) - g.d.min_altitude) // g.d.spacing
                m2c = np.asarray(ep.agents[i]["map2communicate"])
                tile = m2c[xl:xr, yu:yd]
                outside = np.ones(m2c.shape, dtype=bool)
                outside[xl:xr, yu:yd] = False
                assert np.isin(tile, g.d.meas_value[k]).all() and (m2c[outside] == 0.5).all()
                y = g.d.meas_value[k].astype(np.float64)
                # (this path hands bayes_update the float32 measurement values in a float64 map: their log-odds are formed in float64 here,
                #  1e-7 away from the float32 ones of mappings.py:113 that the device, Sim and every scene set use -- the formula is what is pinned)
                rects.append(r), bits.append((tile == g.d.meas_value[k][1]).astype(np.uint8)), lm.append(np.log(y / (1 - y)))
            S, _ = A.sums_ref(g, L, np.array(rects), bits, np.array(lm))
            np.testing.assert_allclose(S, want_s, rtol=1e-9, atol=1e-9)
            rel, ab = A.rewards_of(g, S[:, 0], S[:, 1])
            np.testing.assert_allclose(np.stack([rel, ab], axis=1), want_r, rtol=1e-9, atol=1e-9)


def test_vectorised_reference_is_the_oracles_reward_sums():
    """sums_ref (all agents of an env at once) against O.reward_sums, and the host model against reward_sums(..., dtype=float32) of
    test_hip_constructed_rects.py, on three agents of one scene of a geometry set at either prior."""
    for name in ("geometry_48", "geometry_48p"):
        ds = A.direct_set(name)
        g, e = ds.g, 1
        S, T = A.sums_ref(g, ds.K[e], ds.rects[e], ds.bits[e], ds.lm[e])
        Am = A.after_maps(g, ds.K[e], ds.rects[e], ds.bits[e], ds.lm[e])
        rec = A.lm_record(g, ds.lm[e])
        for i in (0, 3, ds.N - 1):
            want = O.reward_sums(g.o, R._sigmoid(ds.K[e].astype(np.float64)), R._sigmoid(Am[i]))
            np.testing.assert_allclose(S[i], want, rtol=1e-12, atol=1e-12)
            if not g.shift:
                assert R._some(ds.rects[e, i])
                yu, yd, xl, xr = ds.rects[e, i]
                a32 = ds.K[e].copy()
                sel = np.where(ds.bits[e][i] != 0, ds.lm[e, i, 1], ds.lm[e, i, 0]).astype(F32)
                a32[xl:xr, yu:yd] = np.clip(a32[xl:xr, yu:yd], -F32(g.lc), F32(g.lc)) + sel
                want32 = R.reward_sums(g, ds.K[e], a32, np.float32)
                got = A.model_agent(g, ds.K[e], ds.rects[e, i], ds.code[e, i], rec[i], A.weighted_entropy32(g, ds.K[e]))
                np.testing.assert_allclose(got, want32, rtol=1e-12, atol=1e-9)


def _half_bound(tag, got, ref, bound):
    ratio = np.abs(got - ref) / bound
    print(tag, "float32 restatement / bound: S1 %.4f, S2 %.4f" % (ratio[..., 0].max(), ratio[..., 1].max()))
    assert ratio.max() <= 0.5, (tag, np.unravel_index(int(ratio.argmax()), ratio.shape), float(ratio.max()))


@pytest.mark.parametrize("name", ALL_SETS)
def test_float32_restatement_keeps_half_of_every_bound_direct(name):
    """Per-cell float32 terms summed in float64 (the kernel's arithmetic; float64 terms on the SHIFT path) stay within HALF of the
    bound on (S1_i, S2_i - T) for every agent of every scene: no term n_weighted_cells x eps_cell is needed beside the bound."""
    ds = A.direct_set(name)
    ref = ds.ref
    got = ds.model(T=ref["T"])
    _half_bound(name, got, ref["S"], ds.bound(ref["S"]))
    # the restatement's own T, as the device's running T would be: inside half of S2's bound too
    assert (np.abs(ds.model_T - ref["T"]) <= 0.5 * (A.RTOL * np.abs(ref["T"]) + 1e-6)).all()


A1_GRIDS = sorted({grid for grid, _ in A.A1_FORMS})


@pytest.mark.parametrize("grid", A1_GRIDS)
def test_float32_restatement_keeps_half_of_every_bound_scene_sets(grid):
    """Every scene, every step, every agent of every A1 grid.  This is also what stands for the class weights of these sets: their maps
    come from Sim, where a value beside +-wt is improbable, not excluded -- but a cell on which the float32 rule and the reference's
    probability rule disagreed on w(a) would move S2 by 0.5 H(K) and S1 by 0.5 (H(K) - H(a)) with H(a) = 1 at the threshold: one of
    the two by 0.25 or more, which is more than half of the largest bound here, so half of the bound on every scene leaves no such
    cell in the restatement's maps."""
    g = A.geom(grid)
    for t, ((S, _), (S32, _)) in enumerate(zip(A.a1_reference(grid, False), A.a1_reference(grid, True))):
        atol = np.vectorize(lambda s2: R.sums_atol(g, s2))(S[..., 1])
        bound = A.RTOL * np.abs(S) + atol[..., None]
        assert 0.5 * bound.max() < 0.25      # (what the docstring says of a class-weight disagreement)
        _half_bound(f"{grid} step {t}", S32, S, bound)


@pytest.mark.parametrize("name", ALL_SETS)
def test_float32_weight_rule_agrees_with_the_reference_on_every_cell(name):
    """The device decides the class weight on float32 log-odds, the reference on probabilities with 0.499 / 0.501 and np.round: they
    agree on K in every cell of every map and on a in every cell the kernel walks, for every agent.  Cells excused: 0."""
    ds = A.direct_set(name)
    g = ds.g
    wt = g.d.logit_weight_thr
    rec = A.lm_record(g, ds.lm)
    excused = 0
    for e in range(ds.E):
        K32 = ds.K[e]
        excused += int((A.weight32(K32, wt) != A.ref_weight(K32.astype(np.float64))).sum())
        Am = A.after_maps(g, K32, ds.rects[e], ds.bits[e], ds.lm[e])
        for i in range(ds.N):
            yu, yd, xl, xr = ds.rects[e, i]
            kc = np.clip(K32.astype(np.float64), -np.float64(F32(g.lc)), np.float64(F32(g.lc)))
            sel = np.where(ds.bits[e][i] != 0, rec[e, i, 1], rec[e, i, 0]).astype(F32) if R._some(ds.rects[e, i]) else None
            if g.shift:
                a64 = kc - g.lp
                if sel is not None:
                    a64[xl:xr, yu:yd] = kc[xl:xr, yu:yd] + sel.astype(np.float64)
                excused += int((A.weight32(a64.astype(F32), wt) != A.ref_weight(Am[i])).sum())
            elif sel is not None:
                a32 = (np.clip(K32[xl:xr, yu:yd], -F32(g.lc), F32(g.lc)) + sel).astype(F32)
                excused += int((A.weight32(a32, wt) != A.ref_weight(Am[i][xl:xr, yu:yd])).sum())
    assert excused == 0


def test_threshold_neighbours_are_at_most_one_float32_apart():
    """The values around +-wt and +-wt - lm: the value itself and its direct float32 neighbours already satisfy the agreement above
    (recorded in profiles/r22/README.md: distance 1 ulp everywhere, no value had to step further out)."""
    for name in ("128", "nf42"):
        vals, steps = A.value_classes(name)
        assert all(k == (0 if side == "on" else 1) for _, side, k in steps), [s for s in steps if s[2] not in (0, 1)]
        g = A.grid(name)
        wt = F32(g.d.logit_weight_thr)
        assert vals["+wt"] == wt and vals["+wt+"] == np.nextafter(wt, F32(1)) and vals["-wt-"] == np.nextafter(-wt, F32(-1))


def _transitions(ds, ring=0):
    """{(w(K), w(a), |K| >= lc)} over the cells of the footprints (and of a ring around them) of a set, by the reference's rule."""
    g, out = ds.g, set()
    for e in range(ds.E):
        Am = A.after_maps(g, ds.K[e], ds.rects[e], ds.bits[e], ds.lm[e])
        wk = A.ref_weight(ds.K[e].astype(np.float64))
        for i in range(ds.N):
            yu, yd, xl, xr = ds.rects[e, i] + np.array([-ring, ring, -ring, ring])
            wa = A.ref_weight(Am[i][xl:xr, yu:yd])
            clip = np.abs(ds.K[e][xl:xr, yu:yd]) >= F32(g.lc)
            out |= set(zip(wk[xl:xr, yu:yd].ravel().tolist(), wa.ravel().tolist(), clip.ravel().tolist()))
    return out


def test_census_of_the_value_sets():
    """Every class of K inside the footprint under both bits of every altitude, and in the ring; all nine (w(K), w(a)) transitions
    ((0.5, 0.5) in the ring only: inside a footprint it would need |lm| <= 2 wt, and the weakest measurement has |lm| = 0.51);
    with H(K) at the clip the four that exist: w(K) = 0.5 needs |K| <= wt < lc, and a = +-lc + lm inside the middle band needs a
    measurement of log-odds -+lc, which no altitude has -- so (0, 0), (1, 1) and, under the noise-free +-inf, (1, 0), (0, 1)."""
    seen = set()
    for name in ("values128", "values_nf"):
        ds = A.direct_set(name)
        g = ds.g
        yu, yd, xl, xr = A.FOOT[g.grid]
        inside = np.zeros((g.gx, g.gy), dtype=bool)
        inside[xl:xr, yu:yd] = True
        levels = {tuple(row) for row in ds.lm[0].tolist()}
        assert len(levels) == len(g.lm)
        cover, ring = set(), set()
        for e in range(ds.E):
            lab = ds.label_of[e]
            ring |= set(lab[(lab >= 0) & ~inside].tolist())
            for i in range(ds.N):
                lvl = [k for k, row in enumerate(g.lm.tolist()) if row == ds.lm[e, i].tolist() or (np.isinf(row[0]) and np.isinf(ds.lm[e, i, 0]))][0]
                cover |= set(zip(lab[xl:xr, yu:yd].ravel().tolist(), [lvl] * ds.bits[e][i].size, ds.bits[e][i].ravel().tolist()))
        n = len(ds.labels)
        assert ring == set(range(n)), sorted(set(range(n)) - ring)
        assert cover == {(k, lvl, b) for k in range(n) for lvl in range(len(g.lm)) for b in (0, 1)}
        # clip classes among the footprint's cells
        Kf, lc = ds.K[:, xl:xr, yu:yd], F32(g.lc)
        for cls in (Kf == lc, Kf == -lc, (Kf > lc) & np.isfinite(Kf), (Kf < -lc) & np.isfinite(Kf), np.abs(Kf) < lc, Kf == np.nextafter(lc, F32(0))):
            assert cls.any()
        if name == "values_nf":
            assert (Kf == np.inf).any() and (Kf == -np.inf).any() and np.isinf(ds.lm).any()
            # K = +inf under a -inf measurement
            hit = False
            for e in range(ds.E):
                for i in range(ds.N):
                    sel = np.where(ds.bits[e][i] != 0, ds.lm[e, i, 1], ds.lm[e, i, 0])
                    hit |= bool(((ds.K[e, xl:xr, yu:yd] == np.inf) & (sel == -np.inf)).any())
            assert hit
        tr = _transitions(ds, A.RING)
        print(name, len(ds.labels), "classes;", sorted(tr))
        seen |= tr
        if name == "values128":
            assert {(a, b) for a, b, _ in tr} == {(a, b) for a in (0.0, 0.5, 1.0) for b in (0.0, 0.5, 1.0)}
    assert {(a, b) for a, b, c in seen if c} == {(0.0, 0.0), (1.0, 1.0), (1.0, 0.0), (0.0, 1.0)}


def test_census_of_the_geometry_sets():
    """Alignments, thin and border footprints, the largest footprint's item counts per instantiation, empty footprints and agents
    that do not fly."""
    items = {}
    for name, full in A.GEOMETRY.items():
        ds = A.direct_set("geometry_" + name)
        g = ds.g
        rects = [tuple(r) for r in ds.rects.reshape(-1, 4).tolist()]
        some = [r for r in rects if R._some(r)]
        if full:
            assert len({(r[0] % 4, r[1] % 4, r[2] % 4, r[3] % 4) for r in some}) == 256
            assert {(r[3] - r[2], r[1] - r[0]) for r in some} >= {(h, w) for h in (1, 2, 3) for w in (1, 2, 3)}
            if g.tiles_ok:
                assert len({(r[2] % 4, r[0] % 8) for r in some}) == 32
        assert any(r[0] == 0 for r in some) and any(r[2] == 0 for r in some)
        assert any(r[1] == g.gy - 1 for r in some) and any(r[3] == g.gx - 1 for r in some)
        assert sum(r[1] - r[0] == g.wmax and r[3] - r[2] == g.hmax for r in some) >= 5
        empty = {r for r in rects if not R._some(r)}      # (at every prior)
        assert any(r == (0, 0, 0, 0) for r in empty) and any(r[3] == r[2] and r[1] > r[0] for r in empty) and any(r[1] == r[0] and r[3] > r[2] for r in empty)
        teams = A.team_sizes(ds)
        assert teams.min() == 1 and teams.max() == ds.N and len(set(teams.tolist())) == ds.N
        assert ds.copies[0] == 0 and 0 < ds.copies[1] < ds.E - 1 and ds.copies[2] == ds.E - 1 and all(np.array_equal(ds.K[0], ds.K[k]) for k in ds.copies)
        assert not np.array_equal(ds.K[1], ds.K[2])
        for layout in (("rows", "tiles") if (name, "tiles") in [(n[len("geometry_"):], lay) for n, lay in A.DIRECT_SETS] else ("rows",)):
            key = A.instantiation(g, layout == "tiles")
            items.setdefault(key, []).extend(A.items_of(g, r, layout == "tiles") for r in rects)
    for grid, layout in A.A1_FORMS:      # the scene sets of test_hip_constructed_rects.py: every instantiation runs there too
        g = A.geom(grid)
        key = A.instantiation(g, layout == "tiles")
        items.setdefault(key, []).extend(A.items_of(g, r, layout == "tiles") for sc in R.make_scenes(grid) for r in sc["rects"][1:].reshape(-1, 4))
    top = {k: max(v) for k, v in items.items()}
    print(top)
    assert set(top) == {"k_agent_rewards<%d, %s, %s>" % k for k in ((4, "false", "true"), (4, "false", "false"), (4, "true", "false"),
                                                                     (1, "false", "false"), (1, "true", "false"))}
    # the item loop runs a second time beyond 1024 items and a third time beyond 2048
    for key in ("k_agent_rewards<4, false, false>", "k_agent_rewards<4, false, true>", "k_agent_rewards<4, true, false>"):
        assert any(1024 < n <= 2048 for n in items[key]) or key != "k_agent_rewards<4, false, false>", key
        assert any(n > 2048 for n in items[key]) and any(0 < n <= 1024 for n in items[key]), key
    assert any(n > 1024 for n in items["k_agent_rewards<1, true, false>"])
    # (one cell per lane at prior 0.5: the contract's largest footprint on a grid below 44 cells has at most 20 x 20 items)
    assert 0 < top["k_agent_rewards<1, false, false>"] <= 1024
    assert any(n == 0 for n in items["k_agent_rewards<4, false, false>"])       # an empty footprint: nothing is walked


def test_one_line_changes_to_the_device_code_alter_an_expected_result():
    """Each change to the host model of k_agent_rewards moves at least one agent's (S1, S2) beyond its bound on some set, while the
    unchanged model stays within half of it.  "row bound inclusive" (x < xb made x <= xb) is not among them: the extra row is outside
    the footprint, so both of its weights are 0 whatever is loaded -- it can alter no value (profiles/r22/README.md)."""
    sets = [A.direct_set(n) for n in ("values128", "values_nf", "geometry_48", "geometry_34", "geometry_48p")]
    found = {}
    for m in A.MUTATIONS:
        if m == "row bound inclusive":
            continue
        for ds in sets:
            ref = ds.ref
            bound = ds.bound(ref["S"])
            got = ds.model(mutate=m, T=ref["T"])
            with np.errstate(invalid="ignore"):
                ratio = np.abs(got - ref["S"]) / bound
            ratio = np.where(np.isnan(ratio), np.inf, ratio)
            if ratio.max() > 1.0:
                found.setdefault(m, []).append((ds.name, float(min(ratio.max(), 1e300))))
    print(found)
    assert set(found) == set(A.MUTATIONS) - {"row bound inclusive"}, sorted(set(A.MUTATIONS) - set(found))
