"""NumPy restatement of the terrain library (include/ippmarl.h: the draw, the packed layout, the truth plane), built on the oracle's
Philox.  TEST INFRASTRUCTURE: the device kernels and the host mirror are held to it bit for bit."""
import numpy as np

import ipp_oracle as O

DOMAIN_LIBRARY = 5
FLIP, TRANSPOSE = 1, 2
AUGMENT = {"none": 0, "flips": FLIP, "d4": FLIP | TRANSPOSE}


def _mulhi(w, n):
    return (int(w) * int(n)) >> 32


def draw(seed, episode, M, lgx, lgy, gx, gy, flags):
    """(m, x0, y0, sym) of ``episode`` under ``seed`` for M maps of lgx x lgy cells and a gx x gy grid."""
    assert M >= 1 and lgx >= gx and lgy >= gy and (not flags & TRANSPOSE or (lgx >= gy and lgy >= gx))
    r = [int(v) for v in O.philox4x32(0, episode & 0xFFFFFFFF, O.philox_stream_word(0, 0, DOMAIN_LIBRARY), (episode >> 32) & 0xFFFFFFFF,
                                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)]
    sym = (r[3] & 3 if flags & FLIP else 0) | (((r[3] >> 2) & 1) << 2 if flags & TRANSPOSE else 0)
    m = _mulhi(r[0], M)
    wr, wc = (gy, gx) if sym & 4 else (gx, gy)
    return m, _mulhi(r[1], lgx - wr + 1), _mulhi(r[2], lgy - wc + 1), sym


def pack_library(maps):
    """uint8 bytes of the packed library: map m, row u at word (m * lgx + u) * lw, lw = ceil(lgy / 32); cell v = bit v & 31 of word v >> 5."""
    maps = (np.asarray(maps) != 0).astype(np.uint8)
    M, lgx, lgy = maps.shape
    lw = (lgy + 31) // 32
    padded = np.zeros((M, lgx, lw * 32), dtype=np.uint8)
    padded[:, :, :lgy] = maps
    return np.packbits(padded, axis=-1, bitorder="little").reshape(-1)     # (little-endian words: byte b of a row holds cells 8 b .. 8 b + 7)


def crop(maps, d, gx, gy):
    """The gx x gy truth of draw ``d``: truth(x, y) = L_m[u][v], cell by cell as the contract words it."""
    m, x0, y0, sym = d
    L = np.asarray(maps)[m] != 0
    x = np.arange(gx)[:, None]
    y = np.arange(gy)[None, :]
    xp = gx - 1 - x if sym & 1 else x
    yp = gy - 1 - y if sym & 2 else y
    u, v = (x0 + yp, y0 + xp) if sym & 4 else (x0 + xp, y0 + yp)
    u, v = np.broadcast_arrays(u, v)
    return L[u, v].astype(np.uint8)


def truth_bytes(gx, gy):
    return (gx * gy + (8 if gy % 4 else 0) + 31) // 32 * 4


def truth_plane(maps, d, gx, gy):
    """The env's packed plane: the row-major bit string of the crop, zero-padded to truth_bytes."""
    out = np.zeros(truth_bytes(gx, gy), dtype=np.uint8)
    bits = np.packbits(crop(maps, d, gx, gy).reshape(-1), bitorder="little")
    out[: bits.size] = bits
    return out
