"""CPU checks of the keyed minibatch permutation as tests/shuffle_ref.py restates it (the device kernel is held to the restatement bit for
bit by tests/test_hip_shuffle.py): it is a bijection, its keys matter, its statistics are those of uniform permutations with six rounds
(and visibly not with four), the mixed-team mapping is ``valid_transitions(W)[pi]``, and the switch's resolver."""
import numpy as np
import pytest

import shuffle_ref as S

SIZES = (1, 2, 3, 4, 5, 17, 63, 64, 65, 300, 4096, 4097, 61440)
ROUNDS = (0, 7, (1 << 32) + 5)
SEED = 0xC0FFEE1234567893


@pytest.mark.parametrize("n", SIZES)
def test_bijection(n):
    for rnd in ROUNDS:
        walks = []
        perm = S.permutation(n, SEED, rnd, 1, walks=walks)
        assert perm.dtype == np.int64 and perm.shape == (n,)
        assert np.array_equal(np.sort(perm), np.arange(n)), (n, rnd)
        assert 4 ** S.half_bits(n) >= n and (n < 3 or 4 ** S.half_bits(n) < 4 * n)
        print(f"n {n} round {rnd}: longest walk {int(walks[0].max())}, mean {walks[0].mean():.3f}")


def test_every_part_of_the_key_changes_the_permutation():
    n = 300
    base = S.permutation(n, SEED, 3, 0)
    assert np.array_equal(base, S.permutation(n, SEED, 3, 0))
    others = [S.permutation(n, SEED, 4, 0), S.permutation(n, SEED, 3, 1), S.permutation(n, SEED + 1, 3, 0),
              S.permutation(n, SEED ^ (1 << 40), 3, 0), S.permutation(n, SEED, 3 + (1 << 32), 0)]
    perms = [base] + others
    for i in range(len(perms)):
        for j in range(i):
            assert (perms[i] != perms[j]).mean() > 0.9, (i, j)


def _statistics(n, keys, rounds):
    perms = S.permutation(n, SEED, np.arange(keys, dtype=np.uint64), 0, rounds=rounds)         # [keys, n]
    assert (np.sort(perms, axis=1) == np.arange(n)).all()
    counts = np.zeros((n, n), dtype=np.int64)                                                   # [position, value]
    np.add.at(counts, (np.broadcast_to(np.arange(n), perms.shape).ravel(), perms.ravel()), 1)
    expected = keys / n
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    dof = (n - 1) ** 2
    successors = float((perms[:, 1:] == perms[:, :-1] + 1).sum(axis=1).mean())
    return chi2 / dof, dof, successors


@pytest.mark.parametrize("n", [60, 300])
def test_statistics_of_six_rounds(n):
    """Over 6000 keys: position-by-value chi^2 / dof within 1 +- 5 sqrt(2 / dof) (five standard deviations of a chi^2 variable over its
    degrees of freedom), and the mean number of pairs perm[i + 1] == perm[i] + 1 within 0.1 of the (n - 1) / n of uniform permutations
    (the count is nearly Poisson with that mean: a standard error of 0.013 over 6000 keys)."""
    ratio, dof, successors = _statistics(n, 6000, S.ROUNDS)
    print(f"n {n}: chi2/dof {ratio:.4f} (sigma {np.sqrt(2 / dof):.4f}), successor pairs {successors:.4f} (expected {(n - 1) / n:.4f})")
    assert abs(ratio - 1.0) <= 5 * np.sqrt(2 / dof)
    assert abs(successors - (n - 1) / n) <= 0.1


def test_four_rounds_fail_the_successor_statistic():
    """The check above is not vacuous: with four rounds and the 3-bit halves of n = 60 neighbours stay neighbours too often."""
    _, _, successors = _statistics(60, 6000, 4)
    print(f"4 rounds, n 60: successor pairs {successors:.4f} (expected {59 / 60:.4f})")
    assert abs(successors - 59 / 60) > 0.1


def test_team_mapping_is_the_flying_rows_indexed_by_the_permutation():
    teams, n_agents, blocks = [1, 2, 3, 6, 4, 5], 6, 3
    n_envs = len(teams)
    # valid_transitions: the nonzero positions of the flying mask expanded over the blocks, in [blocks, E, N] order
    flying = (np.arange(n_agents)[None, :] < np.asarray(teams)[:, None])
    rows = np.nonzero(np.broadcast_to(flying, (blocks, n_envs, n_agents)).reshape(-1))[0]
    n = blocks * sum(teams)
    assert rows.size == n
    for data_pass in range(3):
        perm = S.permutation(n, SEED, 11, data_pass)
        got = S.team_rows(perm, teams, n_agents)
        assert np.array_equal(got, rows[perm])
        assert np.array_equal(np.sort(got), rows)


def test_resolver(monkeypatch):
    from ippmarl import shuffle_native
    monkeypatch.delenv(shuffle_native.ENV_VAR, raising=False)
    assert shuffle_native.ENV_VAR == "IPPMARL_SHUFFLE"
    assert shuffle_native.resolve_mode() == "torch" and shuffle_native.resolve_mode("native") == "native"
    monkeypatch.setenv(shuffle_native.ENV_VAR, "native")
    assert shuffle_native.resolve_mode() == "native" and shuffle_native.resolve_mode("torch") == "torch"
    monkeypatch.setenv(shuffle_native.ENV_VAR, "")
    assert shuffle_native.resolve_mode() == "torch"
    for bad in ("hip", "Native", "1"):
        with pytest.raises(ValueError):
            shuffle_native.resolve_mode(bad)
    monkeypatch.setenv(shuffle_native.ENV_VAR, "philox")
    with pytest.raises(ValueError):
        shuffle_native.resolve_mode()
