"""CPU checks of the terrain library's draw: the host mirror of the device draw (ippm_host_library_draw) against the NumPy restatement
(tests/terrain_library_ref.py), the ranges of every draw, the coverage of the (map, symmetry) pairs the GPU tests rely on, the error
returns, and the reference's own pack / crop on hand-made maps."""
import ctypes as C
import os

import numpy as np
import pytest

import terrain_library_ref as R

SEED = 0xC0FFEE1234567893
_rng = np.random.default_rng(20)
EPISODES = [0, 1, 2 ** 31 - 1] + [int(v) for v in _rng.integers(0, 2 ** 40, 500)]


@pytest.fixture(scope="module")
def ffi():
    from ippmarl import _ffi
    if not os.path.isfile(os.path.abspath(_ffi.LIB_PATH)):
        pytest.fail("libippmarl.so is not built: python __graft_entry__.py builds it")
    return _ffi


def _in_ranges(d, M, lgx, lgy, gx, gy, flags):
    m, x0, y0, sym = d
    wr, wc = (gy, gx) if sym & 4 else (gx, gy)
    allowed = (3 if flags & R.FLIP else 0) | (4 if flags & R.TRANSPOSE else 0)
    return 0 <= m < M and 0 <= x0 <= lgx - wr and 0 <= y0 <= lgy - wc and sym & ~allowed == 0


# (gx, gy, lgx, lgy): exactly the grid's size (every offset 0), one cell of slack either way, a rectangular grid in a square library
# that holds it turned, and plenty of room
WINDOWS = [(45, 45, 45, 45), (45, 45, 46, 46), (64, 48, 64, 64), (64, 48, 65, 65), (128, 128, 300, 517)]


@pytest.mark.parametrize("M", [1, 2, 3, 7, 1000])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_host_mirror_equals_the_reference(ffi, M, flags):
    for gx, gy, lgx, lgy in WINDOWS:
        for ep in EPISODES:
            want = R.draw(SEED, ep, M, lgx, lgy, gx, gy, flags)
            got = ffi.host_library_draw(SEED, ep, M, lgx, lgy, gx, gy, flags)
            assert got == want, (ep, M, flags, gx, gy, lgx, lgy)
            assert _in_ranges(got, M, lgx, lgy, gx, gy, flags), (got, ep)
            if lgx == gx and lgy == gy and gx == gy:
                assert got[1] == 0 and got[2] == 0
    # lgx == gx alone pins x0 of the untransposed windows
    for ep in EPISODES[:50]:
        got = ffi.host_library_draw(SEED, ep, M, 64, 100, 64, 48, flags & R.FLIP)
        assert got == R.draw(SEED, ep, M, 64, 100, 64, 48, flags & R.FLIP) and got[1] == 0 and 0 <= got[2] <= 52


def test_every_part_of_the_key_changes_the_draw():
    draws = lambda seed, first: [R.draw(seed, first + k, 1000, 300, 517, 128, 128, 3) for k in range(64)]  # noqa: E731
    base = draws(SEED, 0)
    assert base == draws(SEED, 0)
    for other in (draws(SEED + 1, 0), draws(SEED ^ (1 << 40), 0), draws(SEED, 1 << 32), draws(SEED, 64)):
        assert sum(a == b for a, b in zip(base, other)) == 0


def test_consecutive_episodes_cover_every_map_and_symmetry():
    """The GPU tests compare whole planes of a handful of envs and lean on the draws they meet; this is the condition on the inputs: over
    4096 consecutive episodes every (map, symmetry) pair of 3 maps under "d4" occurs (and, without augmentation, symmetry 0 alone)."""
    pairs = {(d[0], d[3]) for d in (R.draw(3, ep, 3, 300, 517, 128, 128, R.AUGMENT["d4"]) for ep in range(4096))}
    assert pairs == {(m, s) for m in range(3) for s in range(8)}
    assert {R.draw(3, ep, 3, 300, 517, 128, 128, 0)[3] for ep in range(256)} == {0}
    assert {R.draw(3, ep, 3, 300, 517, 128, 128, R.FLIP)[3] for ep in range(256)} == {0, 1, 2, 3}
    assert {R.draw(3, ep, 3, 300, 517, 128, 128, R.TRANSPOSE)[3] for ep in range(256)} == {0, 4}


@pytest.mark.parametrize("args,needle", [
    ((0, 64, 64, 45, 45, 0), "n_maps"),                # no map
    ((3, 44, 64, 45, 45, 0), "smaller than the grid"),
    ((3, 64, 44, 45, 45, 3), "smaller than the grid"),
    ((3, 64, 50, 64, 48, 2), "TRANSPOSE"),             # holds the grid, not the turned grid
    ((3, 64, 50, 64, 48, 3), "TRANSPOSE"),
    ((3, 64, 64, 45, 45, 4), "flag"),
])
def test_error_returns(ffi, args, needle):
    lib = ffi.load_library()
    out = (C.c_int32 * 4)(-7, -7, -7, -7)
    M, lgx, lgy, gx, gy, flags = args
    assert lib.ippm_host_library_draw(SEED, 5, M, lgx, lgy, gx, gy, flags, out) == -1
    assert needle in lib.ippm_last_error().decode()
    assert list(out) == [-7] * 4
    with pytest.raises(ffi.IppmError):
        ffi.host_library_draw(SEED, 5, M, lgx, lgy, gx, gy, flags)
    # the same library without the transpose is fine where only the turned grid does not fit
    if needle == "TRANSPOSE":
        assert lib.ippm_host_library_draw(SEED, 5, M, lgx, lgy, gx, gy, flags & 1, out) == 0


def test_library_bytes(ffi):
    lib = ffi.load_library()
    n = np.zeros(1, dtype=np.int64)
    for M, lgx, lgy in [(1, 1, 1), (3, 70, 67), (2, 300, 517), (64, 1024, 1024)]:
        assert lib.ippm_terrain_library_bytes(M, lgx, lgy, n.ctypes.data) == 0
        assert int(n[0]) == M * lgx * ((lgy + 31) // 32) * 4 == R.pack_library(np.zeros((M, lgx, lgy), dtype=np.uint8)).size
    assert lib.ippm_terrain_library_bytes(0, 8, 8, n.ctypes.data) == -1
    assert lib.ippm_terrain_library_bytes(1, 1 << 16, 1 << 20, n.ctypes.data) == -1      # one map of 2^31 bytes or more


def test_reference_crop_on_a_hand_made_map():
    """The restatement itself, on a map whose cells say where they are: L[u][v] = 1 iff (3 u + 5 v) % 7 < 3."""
    u, v = np.meshgrid(np.arange(9), np.arange(11), indexing="ij")
    L = ((3 * u + 5 * v) % 7 < 3).astype(np.uint8)[None]
    gx, gy = 4, 6
    for sym in range(8):
        x0, y0 = 2, 3
        t = R.crop(L, (0, x0, y0, sym), gx, gy)
        win = L[0, x0:x0 + gy, y0:y0 + gx].T if sym & 4 else L[0, x0:x0 + gx, y0:y0 + gy]
        if sym & 1:
            win = win[::-1]
        if sym & 2:
            win = win[:, ::-1]
        assert np.array_equal(t, win), sym
    plane = R.truth_plane(L, (0, 2, 3, 0), gx, gy)
    assert plane.size == R.truth_bytes(gx, gy) == 4 and np.array_equal(np.unpackbits(plane, bitorder="little")[:24].reshape(4, 6), L[0, 2:6, 3:9])
    packed = R.pack_library(L).view(np.uint32).reshape(1, 9, 1)
    assert all(((int(packed[0, a, 0]) >> b) & 1) == L[0, a, b] for a in range(9) for b in range(11)) and not (packed >> 11).any()


def test_load_library_reads_npy_and_npz(tmp_path):
    from ippmarl.terrain import load_library
    maps = (_rng.random((3, 9, 11)) < 0.5)
    np.save(tmp_path / "maps.npy", maps)
    np.savez(tmp_path / "maps.npz", a=maps[0], b=maps[1:].astype(np.uint8) * 255)
    for name in ("maps.npy", "maps.npz"):
        got = load_library(str(tmp_path / name))
        assert got.dtype == np.uint8 and np.array_equal(got, maps.astype(np.uint8)), name
    with pytest.raises(ValueError):
        np.savez(tmp_path / "bad.npz", a=maps[0], b=maps[0, :5])
        load_library(str(tmp_path / "bad.npz"))
