"""Synthetic random-field terrain, generated on the GPU for a whole batch of episodes.

The reference synthesises a power-law Gaussian random field for every episode (white noise -> FFT -> sqrt(P(k)) ->
inverse FFT -> min/max normalise -> ``>= 0.5``; ``mapping/ground_truths.py:16-40`` with
``P(k) = k**-cluster_radius`` from ``mapping/simulations.py:34-40``) and then overwrites it with the half-plane split
it actually flies over.  ``VecEnv.reset(..., terrain="random_field")`` flies over that field instead: it is the
"synthetic random-field terrain" of the benchmark.  The device noise is Philox-keyed by (seed, episode, cell); it is
*not* NumPy's legacy normal stream, so for a given episode this field differs from the one the reference would have
discarded — tests that compare against the oracle hand the generated truth to both sides.

Device work (csrc/terrain.hip): power-of-two grids draw the half spectrum directly and invert it in two hand-written
LDS passes — rocFFT's batched 2-D real transforms were 4x slower on this shape — the second of them either run twice, for the
field's min / max and for its threshold bits, or (128 / 256 cells a side, 128 envs or more) once by one workgroup per env
that keeps the rows in registers, so that the field is never stored (``ippm_terrain_truth``;
``ippm_terrain_field`` + ``ippm_terrain_pack`` are the same arithmetic with the field written out); other grid sizes
(the default 493 x 493) use ``ippm_terrain_noise`` + rocFFT via torch.fft and ``ippm_terrain_pack``.

``terrain="library"`` (``LibraryTerrain``, at the end of this module) flies over the caller's own maps instead: crops of a device-resident
library, drawn per episode (csrc/terrain_library.hip).
"""
from typing import Optional

import numpy as np
import torch

from . import _ffi


def fft_index_row(n: int) -> np.ndarray:
    """Wave numbers in the order the reference enumerates them (ground_truths.py:9-13).  For odd n the list is one
    short, which leaves the last amplitude row/column at zero; that is kept."""
    half = n // 2
    return np.array(list(range(0, half + 1)) + [-i for i in reversed(range(1, half))], dtype=np.float64)


def amplitude_table(gx: int, gy: int, cluster_radius: float) -> np.ndarray:
    """sqrt(P(|k|)) with P(k) = k**-cluster_radius and P(0) = 0, float64 [gx, gy]."""
    kx, ky = fft_index_row(gx), fft_index_row(gy)
    k = np.sqrt(kx[:, None] ** 2 + ky[None, :] ** 2)
    amp = np.zeros((gx, gy))
    sub = np.zeros_like(k)
    sub[k > 0] = np.sqrt(k[k > 0] ** (-float(cluster_radius)))
    amp[: len(kx), : len(ky)] = sub
    return amp


class RandomFieldTerrain:
    def __init__(self, derived, ctx: "_ffi.Context", device: torch.device, cluster_radius: float, chunk_bytes: int = 1 << 30):
        self.d, self.ctx, self.device = derived, ctx, device
        gx, gy = derived.grid_x, derived.grid_y
        amp = amplitude_table(gx, gy, cluster_radius)
        self.real_fft = gx % 2 == 0 and gy % 2 == 0   # the odd-size quirk breaks the Hermitian symmetry of the table
        if self.real_fft:
            amp = amp[:, : gy // 2 + 1]
        self.amp = torch.from_numpy(np.ascontiguousarray(amp).astype(np.float32)).to(device)
        # the hand-written passes exist for 128 / 256 / 512 / 1024 cells a side (terrain_pow2_check in csrc/terrain.hip); every other
        # size, smaller powers of two included, draws the spectrum with ippm_terrain_noise and inverts it with rocFFT
        self.native = all(n in (128, 256, 512, 1024) for n in (gx, gy))
        self.chunk = max(1, chunk_bytes // (gx * gy * 4))
        self._noise: Optional[torch.Tensor] = None
        self._work: Optional[torch.Tensor] = None

    def generate(self, episode: torch.Tensor, truth: torch.Tensor, stream: int) -> None:
        """Writes the packed truth of ``episode[e]`` into ``truth[e]`` (both device tensors)."""
        gx, gy = self.d.grid_x, self.d.grid_y
        E = episode.numel()
        for lo in range(0, E, self.chunk):
            n = min(self.chunk, E - lo)
            ep, tr = episode[lo:lo + n], truth[lo:lo + n]
            if self.native:
                if self._work is None or self._work.shape[0] < n:
                    self._work = torch.empty(n, gy // 2 + 1, gx, 2, dtype=torch.float32, device=self.device)
                    self._keys = torch.zeros(4 * n + 4, dtype=torch.int32, device=self.device)
                # (the field itself is never stored: second pass once for its min / max, once more for the threshold bits, or its whole-field form;
                #  _keys = per env (min, max, and for IPPM_TERRAIN_ONE_LAUNCH=1: arrivals, fault word), then that form's ticket counter)
                self.ctx.call("ippm_terrain_truth", _ffi.ptr(ep), _ffi.ptr(self.amp), _ffi.ptr(self._work), _ffi.ptr(self._keys), _ffi.ptr(tr),
                              n, stream)
                continue
            if self._noise is None or self._noise.shape[0] < n:
                self._noise = torch.empty(n, gx, gy, dtype=torch.float32, device=self.device)
            noise = self._noise[:n]
            self.ctx.call("ippm_terrain_noise", _ffi.ptr(ep), _ffi.ptr(noise), n, stream)
            if self.real_fft:
                field = torch.fft.irfft2(torch.fft.rfft2(noise) * self.amp, s=(gx, gy))
            else:
                field = torch.fft.ifft2(torch.fft.fft2(noise) * self.amp).real
            field = field.contiguous()
            self.ctx.call("ippm_terrain_pack", _ffi.ptr(field), None, _ffi.ptr(tr), n, stream)


# ---- terrain library: episodes over caller-supplied ground-truth maps ------------------------------------------------------------------
AUGMENT_FLAGS = {"none": 0, "flips": _ffi.LIBRARY_FLIP, "d4": _ffi.LIBRARY_FLIP | _ffi.LIBRARY_TRANSPOSE}


def load_library(path: str) -> np.ndarray:
    """Maps of a ``.npy`` file (one ``[M, lgx, lgy]`` array, or one ``[lgx, lgy]`` map) or of an ``.npz`` archive (every array of it, in the
    archive's order, each one map or a stack of maps of one shape) as uint8 ``[M, lgx, lgy]``, nonzero = target class."""
    data = np.load(path, allow_pickle=False)
    if isinstance(data, np.ndarray):
        return _as_maps(data)
    with data:
        return _as_maps([data[k] for k in data.files])


def _as_maps(maps) -> np.ndarray:
    """uint8 [M, lgx, lgy] (1 = target class) of an array, a tensor or a list of equally shaped ones (2-D: one map, 3-D: a stack)."""
    if isinstance(maps, (list, tuple)):
        parts = [np.asarray(m.cpu() if isinstance(m, torch.Tensor) else m) for m in maps]
        if not parts:
            raise ValueError("terrain library: no maps")
        parts = [p[None] if p.ndim == 2 else p for p in parts]
        if any(p.ndim != 3 or p.shape[1:] != parts[0].shape[1:] for p in parts):
            raise ValueError("terrain library: the maps must be 2-D and of one shape")
        arr = np.concatenate(parts, axis=0)
    else:
        arr = np.asarray(maps.cpu() if isinstance(maps, torch.Tensor) else maps)
        if arr.ndim == 2:
            arr = arr[None]
    if arr.ndim != 3 or 0 in arr.shape:
        raise ValueError(f"terrain library: maps of shape [M, lgx, lgy] expected, not {arr.shape}")
    return np.ascontiguousarray(arr != 0).astype(np.uint8)


class LibraryTerrain:
    """Ground truth cut out of a library of binary maps (csrc/terrain_library.hip): at every reset env e gets map ``m``, the window at
    ``(x0, y0)`` and symmetry ``sym`` drawn from (philox_seed, episode[e]) -- the draw stated in include/ippmarl.h -- in one launch.
    ``maps``: ``[M, lgx, lgy]`` bool / uint8 array or tensor, or a list of equally shaped maps; uploaded and bit-packed once.
    ``augment``: "none" (crop only), "flips" (+ the two mirror images), "d4" (+ the transpose: all 8 symmetries of the square; the maps
    must then hold the turned grid too).  ``draws``: device int32 [E,4] = (m, x0, y0, sym) of the last ``generate``."""

    def __init__(self, derived, ctx: "_ffi.Context", device: torch.device, maps, augment: str = "d4"):
        if augment not in AUGMENT_FLAGS:
            raise ValueError(f"library_augment: 'none', 'flips' or 'd4', not {augment!r}")
        self.d, self.ctx, self.device = derived, ctx, device
        self.augment, self.flags = augment, AUGMENT_FLAGS[augment]
        cells = _as_maps(maps)
        self.n_maps, self.lgx, self.lgy = (int(v) for v in cells.shape)
        # the size requirements are the library's (ippm_host_library_draw runs the checks of the draw itself): an IppmError here, not at the first reset
        _ffi.host_library_draw(derived.philox_seed, 0, self.n_maps, self.lgx, self.lgy, derived.grid_x, derived.grid_y, self.flags)
        nbytes = np.zeros(1, dtype=np.int64)
        _ffi.check(ctx.lib.ippm_terrain_library_bytes(self.n_maps, self.lgx, self.lgy, nbytes.ctypes.data), "ippm_terrain_library_bytes")
        self.lib = torch.empty(int(nbytes[0]) // 4, dtype=torch.int32, device=device)
        dev_cells = torch.from_numpy(cells).to(device)
        stream = torch.cuda.current_stream(device)
        _ffi.check(ctx.lib.ippm_terrain_library_pack(_ffi.ptr(dev_cells), self.n_maps, self.lgx, self.lgy, _ffi.ptr(self.lib), stream.cuda_stream),
                   "ippm_terrain_library_pack")
        dev_cells.record_stream(stream)
        self.draws: Optional[torch.Tensor] = None

    def generate(self, episode: torch.Tensor, truth: torch.Tensor, stream: int) -> None:
        """Writes the packed truth of ``episode[e]`` into ``truth[e]`` (both device tensors) and the draws into ``draws``."""
        E = episode.numel()
        if self.draws is None or self.draws.shape[0] != E:
            self.draws = torch.zeros(E, 4, dtype=torch.int32, device=self.device)
        self.ctx.call("ippm_terrain_library_draw", _ffi.ptr(episode), _ffi.ptr(self.lib), self.n_maps, self.lgx, self.lgy, self.flags,
                      _ffi.ptr(self.draws), _ffi.ptr(truth), E, stream)
