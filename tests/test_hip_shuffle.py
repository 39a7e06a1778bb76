"""GPU checks of ippm_minibatch_permutation (csrc/shuffle.hip) through the C-ABI: the indices are the NumPy restatement's
(tests/shuffle_ref.py) bit for bit, in the by-value and the device-counter form, with and without the mixed-team mapping; nothing but
idx[0 .. n) is written; a captured launch follows the device counter; every argument error is refused.  Every launch here writes into a
buffer prefilled with 0xFF between two 4096-byte guard bands that must stay untouched."""
import numpy as np
import pytest
import torch

import shuffle_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 2, 3, 4, 5, 17, 63, 64, 65, 300, 4096, 4097, 61440)
SEED = 0xC0FFEE1234567893          # high bits set
ROUND = (1 << 32) + 5
GUARD = 4096
TEAMS, N_AGENTS, BLOCKS = [1, 2, 3, 6, 4, 5], 6, 3


def _lib():
    from ippmarl import _ffi
    return _ffi, _ffi.load_library()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


class Banded:
    """int64 [n] in the middle of a byte buffer filled with 0xFF, a guard band on either side."""

    def __init__(self, n):
        self.n = n
        self.raw = torch.full((2 * GUARD + 8 * n,), 0xFF, dtype=torch.uint8, device=DEV)
        self.ptr = self.raw.data_ptr() + GUARD
        assert self.ptr % 8 == 0

    def read(self):
        """The indices, after checking both bands."""
        raw = self.raw.cpu().numpy()
        assert (raw[:GUARD] == 0xFF).all() and (raw[GUARD + 8 * self.n:] == 0xFF).all(), "a guard band was written"
        return raw[GUARD:GUARD + 8 * self.n].copy().view(np.int64)

    def untouched(self):
        return bool((self.raw == 0xFF).all())


def _run(n, data_pass, round=ROUND, round_dev=None, prefix=None, n_envs=0, n_agents=0, seed=SEED):
    _ffi, lib = _lib()
    out = Banded(n)
    rc = lib.ippm_minibatch_permutation(seed, round, _ffi.ptr(round_dev), data_pass, n, _ffi.ptr(prefix), n_envs, n_agents, out.ptr,
                                        _stream())
    assert rc == 0, lib.ippm_last_error().decode()
    torch.cuda.synchronize()
    return out.read()


@pytest.mark.parametrize("n", SIZES)
def test_indices_are_the_restatement_bit_for_bit(n):
    for data_pass in range(5):
        got = _run(n, data_pass)
        want = S.permutation(n, SEED, ROUND, data_pass)
        assert got.dtype == want.dtype and np.array_equal(got, want), (n, data_pass, np.nonzero(got != want)[0][:8])
    assert np.array_equal(_run(n, 0, round=0), S.permutation(n, SEED, 0, 0))


@pytest.mark.parametrize("n", [5, 300, 4097])
def test_device_counter_form_equals_the_by_value_form(n):
    counter = torch.tensor([ROUND], dtype=torch.int64, device=DEV)
    for data_pass in (0, 3):
        by_value = _run(n, data_pass, round=ROUND)
        by_counter = _run(n, data_pass, round=123, round_dev=counter)        # (the by-value argument is ignored when the counter is given)
        assert np.array_equal(by_value, by_counter)
        assert not np.array_equal(by_value, _run(n, data_pass, round=123)) or n < 4


def test_team_prefix_maps_ranks_to_the_flying_rows():
    n_envs = len(TEAMS)
    n = BLOCKS * sum(TEAMS)
    prefix = torch.tensor(np.concatenate([[0], np.cumsum(TEAMS)]), dtype=torch.int32, device=DEV)
    flying = np.arange(N_AGENTS)[None, :] < np.asarray(TEAMS)[:, None]
    rows = np.nonzero(np.broadcast_to(flying, (BLOCKS, n_envs, N_AGENTS)).reshape(-1))[0]
    counter = torch.tensor([ROUND], dtype=torch.int64, device=DEV)
    for data_pass in range(3):
        perm = S.permutation(n, SEED, ROUND, data_pass)
        want = S.team_rows(perm, TEAMS, N_AGENTS)
        assert np.array_equal(want, rows[perm])
        assert np.array_equal(_run(n, data_pass, prefix=prefix, n_envs=n_envs, n_agents=N_AGENTS), want)
        assert np.array_equal(_run(n, data_pass, round=0, round_dev=counter, prefix=prefix, n_envs=n_envs, n_agents=N_AGENTS), want)
    # an env nobody flies in: its rows never appear
    teams = [2, 0, 3]
    prefix = torch.tensor([0, 2, 2, 5], dtype=torch.int32, device=DEV)
    got = _run(10, 1, prefix=prefix, n_envs=3, n_agents=4)
    assert np.array_equal(got, S.team_rows(S.permutation(10, SEED, ROUND, 1), teams, 4))
    assert not ((got // 4) % 3 == 1).any()
    # no flying agent at all: -1 everywhere, nothing else written
    assert (_run(6, 0, prefix=torch.zeros(3, dtype=torch.int32, device=DEV), n_envs=2, n_agents=3) == -1).all()


def test_same_bits_across_two_runs():
    for n in (300, 61440):
        a = [_run(n, dp) for dp in range(2)]
        b = [_run(n, dp) for dp in range(2)]
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not np.array_equal(a[0], a[1])


def test_captured_launch_follows_the_device_counter():
    _ffi, lib = _lib()
    n, data_pass = 300, 2
    counter = torch.tensor([ROUND], dtype=torch.int64, device=DEV)
    out = Banded(n)
    stream = torch.cuda.Stream(device=DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        rc = lib.ippm_minibatch_permutation(SEED, 0, _ffi.ptr(counter), data_pass, n, None, 0, 0, out.ptr,
                                            torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
        assert rc == 0, lib.ippm_last_error().decode()
    torch.cuda.synchronize()
    assert out.untouched()                     # a capture records, it does not run
    replayed = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        replayed.append(out.read())
        counter += 1
    eager = [_run(n, data_pass, round=ROUND + k) for k in range(3)]
    assert all(np.array_equal(r, e) for r, e in zip(replayed, eager))
    assert not np.array_equal(eager[0], eager[1]) and not np.array_equal(eager[1], eager[2])


def test_every_argument_error_is_refused_and_launches_nothing():
    _ffi, lib = _lib()
    out = Banded(64)
    counter = torch.zeros(2, dtype=torch.int64, device=DEV)
    prefix = torch.tensor([0, 2, 4, 0], dtype=torch.int32, device=DEV)
    ok = dict(seed=SEED, round=1, round_dev=None, data_pass=0, n=64, prefix=None, n_envs=0, n_agents=0, idx=out.ptr)
    bad = {
        "null idx": dict(idx=None),
        "n = 0": dict(n=0),
        "n < 0": dict(n=-3),
        "n = 2^31": dict(n=1 << 31),
        "data_pass < 0": dict(data_pass=-1),
        "data_pass = 65536": dict(data_pass=65536),
        "prefix without envs": dict(prefix=prefix.data_ptr(), n_envs=0, n_agents=2),
        "prefix without agents": dict(prefix=prefix.data_ptr(), n_envs=2, n_agents=0),
        "misaligned idx": dict(idx=out.ptr + 4),
        "misaligned round_dev": dict(round_dev=counter.data_ptr() + 4),
        "misaligned prefix": dict(prefix=prefix.data_ptr() + 2, n_envs=2, n_agents=2),
    }
    for what, change in bad.items():
        a = dict(ok, **change)
        rc = lib.ippm_minibatch_permutation(a["seed"], a["round"], a["round_dev"], a["data_pass"], a["n"], a["prefix"], a["n_envs"],
                                            a["n_agents"], a["idx"], _stream())
        assert rc == -1, what
        message = lib.ippm_last_error().decode()
        assert "ippm_minibatch_permutation" in message, (what, message)
    torch.cuda.synchronize()
    assert out.untouched()
    # the same arguments without a defect run
    rc = lib.ippm_minibatch_permutation(ok["seed"], ok["round"], None, 0, 64, None, 0, 0, out.ptr, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.read(), S.permutation(64, SEED, 1, 0))


def test_native_shuffle_object():
    """shuffle_native.NativeShuffle above the entry point: one row per data pass, the counter forms, the multiple-of-F check."""
    from ippmarl import _ffi, shuffle_native
    sh = shuffle_native.NativeShuffle(SEED, 3, 300, DEV)
    a = sh.permutation(1, 300, round=ROUND).cpu().numpy()
    assert np.array_equal(a, S.permutation(300, SEED, ROUND, 1))
    sh.set_round(ROUND)
    assert sh.round() == ROUND == sh.host_round
    assert np.array_equal(sh.permutation(2, 120).cpu().numpy(), S.permutation(120, SEED, ROUND, 2))
    sh.advance()
    assert sh.round() == ROUND + 1
    assert np.array_equal(sh.permutation(0, 300).cpu().numpy(), S.permutation(300, SEED, ROUND + 1, 0))
    for args in ((3, 300), (0, 301), (0, 0)):
        with pytest.raises(_ffi.IppmError):
            sh.permutation(*args)
    teams = shuffle_native.NativeShuffle(SEED, 1, BLOCKS * sum(TEAMS), DEV, torch.tensor(TEAMS), len(TEAMS), N_AGENTS)
    n = BLOCKS * sum(TEAMS)
    assert np.array_equal(teams.permutation(0, n, round=4).cpu().numpy(), S.team_rows(S.permutation(n, SEED, 4, 0), TEAMS, N_AGENTS))
    with pytest.raises(_ffi.IppmError):
        teams.permutation(0, n - 1, round=4)
