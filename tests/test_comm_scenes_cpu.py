"""What the constructed comm cases of tests/comm_scenes.py reach (no GPU): the host model of comm_pair gives the oracle's bytes on
every case, every relation of distance to range and of draw to failure rate occurs with and without effect, and each one-line change
to the model flips at least one expected byte."""
import numpy as np

import comm_scenes as C


def test_host_model_of_comm_pair_gives_the_oracles_bytes():
    for c in C.cases():
        assert np.array_equal(C.model(c), c.expected), c.name
        if c.n_active is not None:      # the whole team, as ippm_comm_matrix sees it: more bytes are set
            assert c.expected_whole_team.sum() > c.expected.sum() and (c.expected_whole_team >= c.expected).all(), c.name
            for e in range(c.E):
                na = int(c.n_active[e])
                assert not c.expected[e, na:].any() and not c.expected[e, :, na:].any()


def test_census_of_the_comm_cases():
    cases = C.cases()
    rel = set()
    for c in cases:
        rel |= C.relations(c)
    print(len(cases), "cases,", sum(c.E for c in cases), "envs;", sorted(rel))
    # each relation with effect (the other condition holds: the relation decides the byte) and without (it fails anyway)
    assert rel >= {(kind, r, eff) for kind in ("range", "draw") for r in "<=>" for eff in (True, False)}, sorted(rel)
    names = [c.name for c in cases]
    # ranges: integer distances, square roots of non-squares, the float32 ranges on either side of their pair's distance
    f32 = C.case("range/float32/nearest")
    dist = np.sqrt(np.array([C._d2(o) for o in C.OFFSETS], dtype=np.float64))
    wide = f32.range32.astype(np.float64)
    assert (wide < dist).any() and (wide > dist).any() and (wide == dist).any()
    assert {int(n.split("/")[2]) for n in names if n.startswith("range/cfg/") and n.split("/")[2].isdigit()} >= {25, 625, 225, 50, 75, 125}
    for off in ((3, 4, 0), (0, 3, 4), (4, 0, 3), (0, -4, 3)):      # offsets at exactly 25.0 m
        assert C._d2(off) == 625 and off in C.OFFSETS
    at, below = C.case("range/cfg/625/at").expected, C.case("range/cfg/625/below").expected
    k34, k034 = C.OFFSETS.index((3, 4, 0)), C.OFFSETS.index((0, 3, 4))
    assert at[k34, 0, 1] == 1 and at[k034, 1, 0] == 1 and below[k34, 0, 1] == 0 and below[k034, 0, 1] == 0
    zero = C.case("range/cfg/zero").expected
    k0 = C.OFFSETS.index((0, 0, 0))
    assert zero[k0].all() and zero.sum() == 2 * len(C.OFFSETS) + 2       # range 0: the diagonal, and the co-located pair
    # draws: asymmetric matrices; co-located under a failing draw; the equal-draw pair of every Philox case passes, and fails one double up
    d = C.case("draws/edges")
    assert (d.draws != d.draws.transpose(0, 2, 1)).any() and (d.expected != d.expected.transpose(0, 2, 1)).any()
    assert d.expected[:, 0, 2].all() and d.expected[:, 2, 0].all() and not d.expected[:, 0, 3].any() and not d.expected[:, 3, 0].any()
    assert C.case("draws/moot").expected[:, :3, :3].all()
    for t in (0, 1, 255, 256, 65535):
        eq, ab = C.case(f"philox/t{t}/equal"), C.case(f"philox/t{t}/above")
        e, i, j = eq.star
        assert eq.draw(e, i, j) == eq.failure_rate and eq.expected[e, i, j] == 1 and ab.expected[e, i, j] == 0
        assert eq.draw(e, i, j) * 2.0 ** 32 == int(eq.draw(e, i, j) * 2.0 ** 32)
        assert int(eq.episode.max()) > 2 ** 32 > int(eq.episode.min()) and eq.n == 16
    assert {(c.n, c.E) for c in cases if c.name.startswith("team/n")} >= {(1, 65), (2, 65), (8, 65), (9, 65), (16, 65), (9, 1), (9, 63), (9, 64)}
    # the batched forms run every case but those whose cfg.comm_range no float32 equals: a single pair, every stage and every team among them
    batched = {c.name for c in cases if c.batched}
    assert len(batched) == 32 and all(c.range32 is None and float(np.float32(c.comm_range)) != c.comm_range for c in cases if not c.batched)
    assert {n for n in names if n.startswith(("philox/", "team/", "draws/", "range/float32/"))} <= batched
    assert {f"range/cfg/{d2}/at" for d2 in (25, 100, 225, 625, 900)} | {"range/cfg/zero", "range/cfg/100"} <= batched
    for n in (8, 9):
        c = C.case(f"team/sizes/n{n}")
        assert set(c.n_active.tolist()) == {0, 1, n - 1, n} and (c.pos[:, n - 1] == c.pos[:, 0]).all()


def test_one_line_changes_to_comm_pair_flip_an_expected_byte():
    flipped = {}
    for m in C.MUTATIONS:
        for c in C.cases():
            if c.name.startswith("team/n"):      # (the large Philox batches add nothing the philox/ cases do not have)
                continue
            n = int((C.model(c, m) != c.expected).sum())
            if n:
                flipped.setdefault(m, []).append((c.name, n))
    print({m: len(v) for m, v in flipped.items()})
    assert set(flipped) == set(C.MUTATIONS), sorted(set(C.MUTATIONS) - set(flipped))
    # the truncations are seen by the cases made for them: an episode id above 2^32, a stage above 255
    assert any(name.startswith("philox/") for name, _ in flipped["episode truncated to 32 bits"])
    assert {name.split("/")[1] for name, _ in flipped["stage truncated to 8 bits"]} == {"t256", "t65535"}
