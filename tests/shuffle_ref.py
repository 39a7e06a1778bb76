"""NumPy restatement of the minibatch permutation of include/ippmarl.h (ippm_minibatch_permutation), written on the oracle's Philox
(ipp_oracle.philox4x32): cycle-walking over a balanced Feistel network.

  k = bit length of n - 1 (0 for n = 1), h = max(1, ceil(k / 2)), mask = 2^h - 1; the domain is [0, 4^h).
  E(x): L = x >> h, R = x & mask; for r = 0 .. rounds - 1:
          f = Philox4x32-10(counter = (R, round & 0xFFFFFFFF, stream_word(agent = r, stage = data_pass, domain = 4), round >> 32),
                            key = (seed & 0xFFFFFFFF, seed >> 32)).word0 & mask;   (L, R) <- (R, L ^ f)
        E(x) = (L << h) | R
  pi(i) = the first of E(i), E(E(i)), ... that is < n.

``rounds`` is a parameter only so that the statistics test can show that fewer rounds than the library's six fail it."""
import numpy as np

import ipp_oracle as O

DOMAIN_SHUFFLE = 4
ROUNDS = 6           # IPPM_SHUFFLE_ROUNDS


def half_bits(n: int) -> int:
    k = int(n - 1).bit_length()
    return max(1, (k + 1) // 2)


def encrypt(x, h: int, seed: int, round: int, data_pass: int, rounds: int = ROUNDS):
    """E on an array of points of [0, 4^h)."""
    x = np.asarray(x, dtype=np.uint64)
    mask = np.uint64((1 << h) - 1)
    L, R = x >> np.uint64(h), x & mask
    # (``round``: an integer, or an array of them that broadcasts against x -- one key per row for the statistics)
    if isinstance(round, np.ndarray):
        round = round.astype(np.uint64)
        lo, hi = round & np.uint64(0xFFFFFFFF), round >> np.uint64(32)
    else:
        round &= 0xFFFFFFFFFFFFFFFF
        lo, hi = round & 0xFFFFFFFF, round >> 32
    for r in range(rounds):
        f = O.philox4x32(R, lo, O.philox_stream_word(r, data_pass, DOMAIN_SHUFFLE), hi,
                         seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0].astype(np.uint64) & mask
        L, R = R, L ^ f
    return (L << np.uint64(h)) | R


def permutation(n: int, seed: int, round: int, data_pass: int, rounds: int = ROUNDS, walks=None) -> np.ndarray:
    """pi as int64 [n] -- or, for ``round`` an array of K rounds, the K permutations as int64 [K, n].  ``walks`` (a list) receives the
    number of E applications of every i."""
    h = half_bits(n)
    many = isinstance(round, np.ndarray)
    shape = (len(round), n) if many else (n,)
    key = np.broadcast_to(round.reshape(-1, 1), shape) if many else None
    x = encrypt(np.broadcast_to(np.arange(n, dtype=np.uint64), shape), h, seed, key if many else round, data_pass, rounds)
    steps = np.ones(shape, dtype=np.int64)
    out = x >= np.uint64(n)
    while out.any():
        x[out] = encrypt(x[out], h, seed, key[out] if many else round, data_pass, rounds)
        steps[out] += 1
        out = x >= np.uint64(n)
    if walks is not None:
        walks.append(steps)
    return x.astype(np.int64)


def team_rows(perm: np.ndarray, team_sizes, n_agents: int) -> np.ndarray:
    """The mixed-team mapping of the header, rank by rank: block = q / F, s = q % F, e = the env with prefix[e] <= s < prefix[e + 1],
    a = s - prefix[e], row = (block * n_envs + e) * n_agents + a."""
    prefix = np.concatenate([[0], np.cumsum(np.asarray(team_sizes, dtype=np.int64))])
    F, n_envs = int(prefix[-1]), len(team_sizes)
    block, s = perm // F, perm % F
    e = np.searchsorted(prefix, s, side="right") - 1
    return (block * n_envs + e) * n_agents + (s - prefix[e])
