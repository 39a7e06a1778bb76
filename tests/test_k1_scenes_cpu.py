"""The census of tests/k1_scenes.py, asserted with the oracle alone: what the constructed scenes of K1 reach is a checked condition, not a
hope.  Also: each of three one-line changes of the device code, applied to the oracle's restatement, changes the expected result of at
least one scene -- so tests/test_hip_k1_constructed.py (bit-for-bit against the unchanged expectation) would fail on a device that had it."""
import numpy as np
import pytest

import ipp_oracle as O
import k1_scenes as K


def _census(A):
    d = K.derived(A)
    keys = K.rule_keys(A)
    hit = {key: [0, 0] for key in keys}          # [with an effect, without]
    c = dict(scenes=0, guard_blocked=0, restored=0, pre_only=0, post_only=0, later_adjacent=0, empty_masks=0, off_lattice=0,
             order_dependent=0, far_unmasked=0, per_family={}, per_policy={}, popcounts={p: set() for p in range(4)}, faults=0,
             overflow_kept=0, stale_replaced=0, sampled_fault=0, team_sizes=set())
    for sc, mask, act, pos, fault in K.expected(A):
        ev = []
        got = K.evaluate(A, sc, events=ev)
        assert all(np.array_equal(a, b) for a, b in zip(got, (mask, act, pos, fault)))
        c["scenes"] += 1
        c["per_family"][sc.family] = c["per_family"].get(sc.family, 0) + 1
        c["per_policy"][sc.policy] = c["per_policy"].get(sc.policy, 0) + 1
        c["team_sizes"].add(sc.N)
        for e in ev:
            if e["kind"] == "pair":
                if e["key"] is not None:
                    hit[e["key"]][0 if e["effect"] else 1] += 1
                c["guard_blocked"] += e["guard_blocked"]
                c["restored"] += e["restored"]
                c["pre_only"] += e["pre"] and not e["post"]
                c["post_only"] += e["post"] and not e["pre"]
            else:
                c["later_adjacent"] += e["later_adjacent"] and e["unmasked"]
                c["empty_masks"] += e["popcount"] == 0
                if e["popcount"]:
                    c["popcounts"][sc.policy].add(e["popcount"])
        c["faults"] += fault != 0
        c["overflow_kept"] += bool(sc.fault0 & K.FAULT_WORK_OVERFLOW) and bool(fault & K.FAULT_WORK_OVERFLOW)
        c["stale_replaced"] += bool(sc.fault0 & ~K.FAULT_WORK_OVERFLOW) and (fault & ~K.FAULT_WORK_OVERFLOW) != (sc.fault0 & ~K.FAULT_WORK_OVERFLOW)
        c["sampled_fault"] += sc.policy == K.POLICY_SAMPLE and fault != 0 and mask[[i for i in range(sc.N) if fault >> i & 1]].any()
        off = [i for i in range(sc.N) if not K.on_lattice(A, pos[i:i + 1])]
        if off:
            # only policy 3's "every valid action has probability 0" leaves the lattice, and only with the env's last agent
            assert sc.policy == K.POLICY_ARGMAX and off == [sc.N - 1], (sc.family, sc.tags, off)
            c["off_lattice"] += 1
        if sc.family == "pairs":
            (_, (ox, oy, oz)), = sc.tags
            if max(abs(ox), abs(oy)) == 2 or (A == 27 and abs(oz) == 2):   # distance 2 masks nothing
                assert np.array_equal(mask[1], O.action_mask(d, sc.pos[1]).astype(np.uint8)), sc.tags
                c["far_unmasked"] += 1
        if sc.family == "chains" and "reversed" not in sc.tags:
            rev = K.explicit(A, "chains", sc.pos[::-1])
            rmask = K.evaluate(A, rev)[0][::-1]
            c["order_dependent"] += not np.array_equal(rmask, mask)
    c["hit"] = hit
    return c


@pytest.mark.parametrize("A", K.ACTION_SETS)
def test_scene_census(A):
    c = _census(A)
    d = K.derived(A)
    assert (d.space_x, d.space_y, d.space_z) == (11, 11, 3)
    print(f"\nK1 scene census, {A} actions: {c['scenes']} scenes; per family {c['per_family']}; per policy {c['per_policy']}; "
          f"team sizes {sorted(c['team_sizes'])}")
    print(f"  collision rules {len(c['hit'])}: matches with an effect {sum(v[0] for v in c['hit'].values())} (min per rule "
          f"{min(v[0] for v in c['hit'].values())}), without {sum(v[1] for v in c['hit'].values())} (min per rule {min(v[1] for v in c['hit'].values())})")
    print(f"  6-action guard blocks {c['guard_blocked']}, 9-action restores {c['restored']}, empty masks {c['empty_masks']}, scenes with a fault "
          f"{c['faults']} (sampling faults on a non-empty mask {c['sampled_fault']}), overflow bit kept {c['overflow_kept']}, stale bits replaced "
          f"{c['stale_replaced']}")
    print(f"  neighbour adjacent only before its move {c['pre_only']}, only after {c['post_only']}, adjacent agent later in the order "
          f"{c['later_adjacent']}, order-dependent chain scenes {c['order_dependent']}, distance-2 pairs {c['far_unmasked']}, "
          f"off-lattice moves (policy 3, last agent) {c['off_lattice']}")
    print(f"  mask popcounts reached: explicit {sorted(c['popcounts'][0])}, policy 1 {sorted(c['popcounts'][1])}, policy 2 "
          f"{sorted(c['popcounts'][2])}, policy 3 {sorted(c['popcounts'][3])}; u extremes {[(u, ep, a, t) for u, ep, a, t in K.u_extremes()]}")
    # every key of O.collision_rule at least once with an effect and at least once without
    for key, (eff, none) in c["hit"].items():
        assert eff >= 1 and none >= 1, (A, key, eff, none)
    assert len(c["hit"]) == {4: 4, 6: 5, 9: 8, 27: 26}[A]
    if A == 6:
        assert c["guard_blocked"] >= 1
    else:
        assert c["guard_blocked"] == 0
    if A == 9:
        assert c["restored"] >= 1 and c["empty_masks"] == 0       # 9 actions never produce an empty mask
    else:
        assert c["restored"] == 0 and c["empty_masks"] >= 4
        assert c["overflow_kept"] >= 2 and c["sampled_fault"] >= 1
    assert c["stale_replaced"] >= 1
    assert c["order_dependent"] >= 1 and c["pre_only"] >= 1 and c["post_only"] >= 1 and c["later_adjacent"] >= 1
    assert c["far_unmasked"] >= 16 and c["off_lattice"] >= 1
    assert set(c["team_sizes"]) == set(K.TEAMS) and set(c["per_policy"]) == {0, 1, 2, 3}
    # policy 1 draws over masks of every popcount the scenes reach
    assert c["popcounts"][1] >= c["popcounts"][0] | c["popcounts"][2] | c["popcounts"][3], c["popcounts"]
    # every scene is in exactly one launch group, none is left out of a comparison
    groups = K.groups(A)
    assert sorted(k for idx in groups.values() for k in idx) == list(range(c["scenes"]))
    assert all(t in (0, d.budget) for _, _, t in groups)


def test_u_extremes_are_in_the_scenes():
    (umin, *lo), (umax, *hi) = K.u_extremes()
    # 2^20 draws of a 24-bit u: the smallest and the largest are expected within 2^4 of the ends; 2^8 would be a one-in-10^7 event
    assert umin < 2 ** 8 and umax >= 2 ** 24 - 2 ** 8, (umin, umax)
    for A in K.ACTION_SETS:
        for u, (ep, agent, t) in ((umin, lo), (umax, hi)):
            found = [sc for sc in K.scenes(A) if sc.policy == K.POLICY_SAMPLE and (sc.ep, sc.t) == (ep, t) and sc.N > agent]
            assert len(found) >= 3, (A, u)
            assert O.philox_action_word(K.SEED, ep, agent, t) >> 8 == u
    # the largest u picks the last action with positive weight, the smallest the first
    A = 6
    p = np.full(A, 1.0 / A, dtype=np.float32)
    assert O.sample_masked_action(umin << 8, p) == 0 and O.sample_masked_action((umax << 8) | 0xFF, p) == A - 1


def test_episode_ids_and_agent_indices_reach_every_counter_word():
    for A in K.ACTION_SETS:
        drawn = [sc for sc in K.scenes(A) if sc.policy in (K.POLICY_UNIFORM, K.POLICY_SAMPLE)]
        assert {sc.ep >> 32 != 0 for sc in drawn} == {False, True}
        assert any(sc.ep == 2 ** 32 - 1 for sc in drawn) and any(sc.ep == 2 ** 32 for sc in drawn)
        assert {sc.t for sc in drawn} == {0, K.derived(A).budget}
        assert any(sc.N == 16 for sc in drawn if sc.policy == K.POLICY_UNIFORM) and any(sc.N == 16 for sc in drawn if sc.policy == K.POLICY_SAMPLE)


def test_empty_mask_scenes_fault_the_cornered_agent():
    for A in (4, 6, 27):
        found = [rec for rec in K.expected(A) if rec[0].family == "empty"]
        assert len(found) == 4 and {rec[0].policy for rec in found} == {0, 2, 3}
        for sc, mask, act, pos, fault in found:
            i = sc.N - 1
            assert fault >> i & 1 and not mask[i].any(), (A, sc.policy)
            assert fault & K.FAULT_WORK_OVERFLOW == sc.fault0 & K.FAULT_WORK_OVERFLOW
            first = int(np.flatnonzero(O.action_mask(K.derived(A), sc.pos[i]))[0])       # move = first boundary-valid action
            assert act[i] == first and np.array_equal(pos[i], O.action_to_position(K.derived(A), sc.pos[i], first))


def test_team_size_scenes_leave_the_grounded_agents_alone():
    for A in K.ACTION_SETS:
        recs = K.expected(A, "teams")
        assert {rec[0].n for rec in recs} == {1, 2, 3, 4} and all(rec[0].N == 4 for rec in recs)
        changed = 0
        for sc, mask, act, pos, fault in recs:
            assert np.array_equal(pos[sc.n:], sc.pos[sc.n:]) and fault >> sc.n == 0
            full = K.evaluate(A, K.Scene(sc.family, sc.pos, sc.policy, t=sc.t, ep=sc.ep, actions=sc.actions, probs=sc.probs))
            changed += not np.array_equal(full[2][:sc.n], pos[:sc.n]) or not np.array_equal(full[0][:sc.n], mask[:sc.n])
        assert changed == 0     # the agents that fly do not see the others either way: they come later in the order


@pytest.mark.parametrize("mutant,sets", [("no_guard", (6,)), ("j_le_i", (6,)), ("col27_4_only", (27,))])
def test_one_line_mutants_change_an_expected_result(mutant, sets):
    """The device code with (a) the popc(m) > 1 guard dropped, (b) ``j <= i`` in the collision loop, (c) ``1u << 4`` alone for the 27-action
    same-column case, restated on the oracle: each changes mask, action or position of some scene, which the GPU test compares bit for bit."""
    for A in sets:
        differing = 0
        for sc, mask, act, pos, fault in K.expected(A):
            got = K.evaluate(A, sc, mutant=mutant)
            differing += not all(np.array_equal(a, b) for a, b in zip(got, (mask, act, pos, fault)))
        print(f"\nmutant {mutant}, {A} actions: {differing} of {len(K.expected(A))} scenes change")
        assert differing >= 1
