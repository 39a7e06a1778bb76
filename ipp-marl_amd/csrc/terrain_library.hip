// Terrain library: every reset cuts each env's truth plane out of caller-supplied binary maps kept bit-packed on the device -- a map, a
// crop window of the grid's size and, optionally, one of the 8 symmetries of the square, drawn from (philox_seed, episode) alone.  The
// draw, the packed layout and the size requirements are the contract stated in include/ippmarl.h; tests/terrain_library_ref.py restates them.
//
// k_library_draw: a bit-granular gather.  An env's plane is the row-major bit string of its gx x gy cells; a workgroup owns the gy
// words of 32 output rows (32 gy bits: whole words whatever gy is), a lane one word at a time.  An output word may span several grid
// rows (gy need not be a multiple of 32): per row segment the lane fetches the 32 bits that start at the segment's first cell -- two
// words and a funnel shift -- masks them to the segment and shifts them into place; the word is stored whole, padding bits zero.
//   untransposed  the 32 bits come straight from the library row (reversed for a y-flip), through a bounds-checked buffer resource of the
//                 drawn map: the word behind a row's or the map's last one is never needed for a cell, and may be read.
//   transposed    an output row runs down a library column.  Lane j of a wavefront loads, from library row base + j, the 32 columns that
//                 are the workgroup's 32 output rows; ballot i over the wavefront is then 64 consecutive cells of output row i -- one load
//                 per 32 output bits, as in the other form.  The ballots go to LDS as 32 bit rows, and the words are assembled from there.
// No atomics, no scratch, vector stores only; the draw is recomputed by every lane (one Philox call) and made uniform with readfirstlane.
#include <algorithm>

#include "ippm_internal.h"
#include "ippm_tiles.h"

namespace {

struct LibDraw {
  int m, x0, y0, sym;
};

__host__ __device__ __forceinline__ uint32_t lib_mulhi(uint32_t w, uint32_t n) { return (uint32_t)(((uint64_t)w * n) >> 32); }

// THE DRAW (ippmarl.h); sizes already checked
__host__ __device__ __forceinline__ LibDraw library_draw(uint32_t k0, uint32_t k1, int64_t episode, int n_maps, int lgx, int lgy, int gx,
                                                         int gy, int flags) {
  const uint64_t ep = (uint64_t)episode;
  const Philox4 r = ippm_philox(0u, (uint32_t)ep, ippm_stream_word(0u, 0u, IPPM_DOMAIN_LIBRARY), (uint32_t)(ep >> 32), k0, k1);
  LibDraw d;
  d.sym = (int)(((flags & IPPM_LIBRARY_FLIP) ? (r.v[3] & 3u) : 0u) | ((flags & IPPM_LIBRARY_TRANSPOSE) ? (r.v[3] & 4u) : 0u));
  d.m = (int)lib_mulhi(r.v[0], (uint32_t)n_maps);
  const int wr = (d.sym & 4) ? gy : gx, wc = (d.sym & 4) ? gx : gy;
  d.x0 = (int)lib_mulhi(r.v[1], (uint32_t)(lgx - wr + 1));
  d.y0 = (int)lib_mulhi(r.v[2], (uint32_t)(lgy - wc + 1));
  return d;
}

struct LibArgs {
  const int64_t* episode;
  const uint32_t* lib;
  int32_t* draws;        // int32 [E,4] or null
  uint8_t* truth;
  uint32_t k0, k1;       // the seed's words
  int n_maps, lgx, lgy, lw;
  int gx, gy, flags;
  uint32_t words;        // 32-bit words of an env's plane (ippm_truth_bytes / 4)
  uint32_t parts;        // workgroups per env, each the gy words of 32 output rows
  int pitch;             // words per LDS bit row (transposed form)
};

__device__ __forceinline__ uint32_t lib_funnel(uint32_t lo, uint32_t hi, int s) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (s & 31)); }

// bits v .. v + 31 of row u of the map behind `rs` (lw words a row); words past the map read as 0
__device__ __forceinline__ uint32_t lib_fetch32(__amdgpu_buffer_rsrc_t rs, int u, int v, int lw) {
  const int off = (u * lw + (v >> 5)) * 4;
  const uint32_t lo = __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0), hi = __builtin_amdgcn_raw_buffer_load_b32(rs, off + 4, 0, 0);
  return lib_funnel(lo, hi, v);
}

// word w of the plane: fetch(x, y, n) returns, in its low n bits, cells (x, y) .. (x, y + n - 1) of the env's truth
template <class Fetch>
__device__ __forceinline__ uint32_t lib_assemble(uint32_t w, int gx, int gy, Fetch fetch) {
  const uint32_t lin = w * 32u;
  int x = (int)(lin / (uint32_t)gy), y = (int)(lin - (uint32_t)x * (uint32_t)gy);
  uint32_t out = 0;
  int filled = 0;
  while (filled < 32 && x < gx) {
    const int n = min(32 - filled, gy - y);
    uint32_t bits = fetch(x, y, n);
    if (n < 32) bits &= (1u << n) - 1u;
    out |= bits << filled;
    filled += n;
    y += n;
    if (y == gy) { y = 0; ++x; }
  }
  return out;
}

__global__ void __launch_bounds__(256) k_library_draw(const LibArgs a) {
  extern __shared__ uint32_t lds[];
  const uint32_t e = blockIdx.x / a.parts, part = blockIdx.x - e * a.parts;
  const int gx = a.gx, gy = a.gy, lw = a.lw, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const LibDraw d = library_draw(a.k0, a.k1, a.episode[e], a.n_maps, a.lgx, a.lgy, gx, gy, a.flags);
  // (every lane draws the same values: readfirstlane tells the compiler so -- the resource below must be built from scalars)
  const int m = __builtin_amdgcn_readfirstlane(d.m), x0 = __builtin_amdgcn_readfirstlane(d.x0), y0 = __builtin_amdgcn_readfirstlane(d.y0),
            sym = __builtin_amdgcn_readfirstlane(d.sym);
  if (a.draws && part == 0 && tid == 0) {
    int32_t* o = a.draws + (size_t)e * 4;
    o[0] = m; o[1] = x0; o[2] = y0; o[3] = sym;
  }
  const size_t map_words = (size_t)a.lgx * lw;
  const __amdgpu_buffer_rsrc_t rs = IPPM_RSRC(a.lib + (size_t)m * map_words, map_words * 4);
  const bool fx = sym & 1, fy = sym & 2;
  uint32_t* out = reinterpret_cast<uint32_t*>(a.truth + (size_t)e * a.words * 4);
  const uint32_t w_end = min((part + 1u) * (uint32_t)gy, a.words);
  if (!(sym & 4)) {
    for (uint32_t w = part * (uint32_t)gy + tid; w < w_end; w += 256u)
      out[w] = lib_assemble(w, gx, gy, [&](int x, int y, int n) -> uint32_t {
        const int u = x0 + (fx ? gx - 1 - x : x);
        if (!fy) return lib_fetch32(rs, u, y0 + y, lw);
        // cells y .. y + n - 1 are library columns y0 + gy - 1 - y downwards: fetch from the lowest, reverse
        return __builtin_bitreverse32(lib_fetch32(rs, u, y0 + gy - y - n, lw)) >> (32 - n);
      });
    return;
  }
  // transposed: output rows xb .. xb + 31 are 32 consecutive library columns, output column y is library row x0 + y'
  const int xb = (int)part * 32, P = a.pitch;
  if (xb < gx) {
    // first column fetched; in the last block of an x-flipped window it may lie up to 31 columns in front of the map: fetch from column 0
    // and shift (the bits shifted in belong to rows >= gx, which nobody reads)
    const int cs = fx ? y0 + gx - 1 - xb - 31 : y0 + xb;
    const int sh = cs < 0 ? -cs : 0, c0 = cs + sh;
    for (int k = wave; k * 64 < gy; k += 4) {
      const int y = k * 64 + lane;
      const int u = x0 + (fy ? gy - 1 - y : y);
      const int off = y < gy ? (u * lw + (c0 >> 5)) * 4 : IPPM_OOB;
      const uint32_t lo = __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0);
      const uint32_t hi = __builtin_amdgcn_raw_buffer_load_b32(rs, y < gy ? off + 4 : IPPM_OOB, 0, 0);
      uint32_t col = lib_funnel(lo, hi, c0) << sh;
      if (fx) col = __builtin_bitreverse32(col);       // bit i = output row xb + i
      uint64_t mine = 0;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        const uint64_t b = __ballot((col >> i) & 1u);  // cells y = 64 k .. 64 k + 63 of output row xb + i
        if ((lane & 31) == i) mine = b;
      }
      lds[(lane & 31) * P + 2 * k + (lane >> 5)] = (uint32_t)(mine >> (32 * (lane >> 5)));
    }
  }
  __syncthreads();
  for (uint32_t w = part * (uint32_t)gy + tid; w < w_end; w += 256u)
    out[w] = lib_assemble(w, gx, gy, [&](int x, int y, int n) -> uint32_t {
      const uint32_t* row = lds + (x - xb) * P + (y >> 5);
      return lib_funnel(row[0], row[1], y);
    });
}

// one wavefront per 64 cells of a library row: a coalesced byte load each, one ballot, two words
__global__ void __launch_bounds__(256) k_library_pack(const uint8_t* __restrict__ cells, uint32_t* __restrict__ lib, size_t rows, int lgy, int lw) {
  const int lane = threadIdx.x & 63, chunks = (lgy + 63) >> 6;
  const size_t items = rows * (size_t)chunks, stride = (size_t)gridDim.x * 4;
  for (size_t it = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += stride) {
    const size_t row = it / (size_t)chunks;
    const int c = (int)(it - row * (size_t)chunks), v = c * 64 + lane;
    const uint64_t bits = __ballot(v < lgy && cells[row * (size_t)lgy + v] != 0);
    if (lane < 2 && 2 * c + lane < lw) lib[row * (size_t)lw + 2 * c + lane] = (uint32_t)(bits >> (32 * lane));
  }
}

int library_sizes_ok(const std::string& who, int64_t n_maps, int64_t lgx, int64_t lgy) {
  if (n_maps < 1 || lgx < 1 || lgy < 1) { ippm_set_error(who + ": needs n_maps >= 1 and maps of at least one cell"); return -1; }
  if (lgx * ((lgy + 31) / 32) * 4 >= ((int64_t)1 << 31)) { ippm_set_error(who + ": a packed map must stay below 2^31 bytes"); return -1; }
  return 0;
}

int library_draw_ok(const std::string& who, int n_maps, int lgx, int lgy, int gx, int gy, int flags) {
  if (library_sizes_ok(who, n_maps, lgx, lgy)) return -1;
  if (flags & ~(IPPM_LIBRARY_FLIP | IPPM_LIBRARY_TRANSPOSE)) { ippm_set_error(who + ": unknown flag bits"); return -1; }
  if (gx < 1 || gy < 1) { ippm_set_error(who + ": the grid needs at least one cell"); return -1; }
  if (lgx < gx || lgy < gy) {
    ippm_set_error(who + ": the library's maps (" + std::to_string(lgx) + " x " + std::to_string(lgy) + ") are smaller than the grid (" +
                   std::to_string(gx) + " x " + std::to_string(gy) + ")");
    return -1;
  }
  if ((flags & IPPM_LIBRARY_TRANSPOSE) && (lgx < gy || lgy < gx)) {
    ippm_set_error(who + ": IPPM_LIBRARY_TRANSPOSE needs maps that also hold the turned grid (" + std::to_string(gy) + " x " + std::to_string(gx) + ")");
    return -1;
  }
  return 0;
}

}  // namespace

extern "C" int ippm_host_library_draw(uint64_t seed, int64_t episode, int32_t n_maps, int32_t lgx, int32_t lgy, int32_t gx, int32_t gy,
                                      int32_t flags, int32_t* out4) {
  const std::string who = "ippm_host_library_draw";
  if (!out4) { ippm_set_error(who + ": null argument (out4)"); return -1; }
  if (library_draw_ok(who, n_maps, lgx, lgy, gx, gy, flags)) return -1;
  const LibDraw d = library_draw((uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), episode, n_maps, lgx, lgy, gx, gy, flags);
  out4[0] = d.m; out4[1] = d.x0; out4[2] = d.y0; out4[3] = d.sym;
  return 0;
}

extern "C" int ippm_terrain_library_bytes(int32_t n_maps, int32_t lgx, int32_t lgy, int64_t* bytes) {
  const std::string who = "ippm_terrain_library_bytes";
  if (!bytes) { ippm_set_error(who + ": null argument (bytes)"); return -1; }
  if (library_sizes_ok(who, n_maps, lgx, lgy)) return -1;
  *bytes = (int64_t)n_maps * lgx * ((lgy + 31) / 32) * 4;
  return 0;
}

extern "C" int ippm_terrain_library_pack(const uint8_t* cells, int32_t n_maps, int32_t lgx, int32_t lgy, uint32_t* lib, void* stream) {
  const std::string who = "ippm_terrain_library_pack";
  if (!cells || !lib) { ippm_set_error(who + ": null argument"); return -1; }
  if (reinterpret_cast<uintptr_t>(lib) & 3) { ippm_set_error(who + ": lib must be 4-byte aligned"); return -1; }
  if (library_sizes_ok(who, n_maps, lgx, lgy)) return -1;
  const size_t rows = (size_t)n_maps * lgx, items = rows * (size_t)((lgy + 63) / 64);
  const unsigned grid = (unsigned)std::min<size_t>((items + 3) / 4, (size_t)1 << 20);
  hipLaunchKernelGGL(k_library_pack, dim3(grid), dim3(256), 0, S_(stream), cells, lib, rows, (int)lgy, (int)((lgy + 31) / 32));
  IPPM_LAUNCH_CHECK("ippm_terrain_library_pack");
  return 0;
}

extern "C" int ippm_terrain_library_draw(ippm_ctx* ctx, const int64_t* episode, const uint32_t* lib, int32_t n_maps, int32_t lgx, int32_t lgy,
                                         int32_t flags, int32_t* draws, uint8_t* truth, int32_t n_envs, void* stream) {
  const std::string who = "ippm_terrain_library_draw";
  if (!ctx || !episode || !lib || !truth) { ippm_set_error(who + ": null argument"); return -1; }
  if ((reinterpret_cast<uintptr_t>(lib) & 3) || (reinterpret_cast<uintptr_t>(truth) & 3) || (reinterpret_cast<uintptr_t>(draws) & 3)) {
    ippm_set_error(who + ": lib, truth and draws must be 4-byte aligned");
    return -1;
  }
  const int gx = ctx->cfg.grid_x, gy = ctx->cfg.grid_y;
  if (library_draw_ok(who, n_maps, lgx, lgy, gx, gy, flags)) return -1;
  if (n_envs < 1) { ippm_set_error(who + ": n_envs must be at least 1"); return -1; }
  const size_t words = ippm_truth_bytes(gx, gy) / 4;
  if (words >= ((size_t)1 << 26)) { ippm_set_error(who + ": the grid's truth plane must stay below 2^31 bits"); return -1; }
  const size_t parts = (words + (size_t)gy - 1) / (size_t)gy;
  if ((size_t)n_envs * parts >= ((size_t)1 << 31)) { ippm_set_error(who + ": n_envs * workgroups per env must stay below 2^31"); return -1; }
  // the transposed form stages 32 output rows as bit rows of ceil(gy / 64) ballots (+ the word a funnel shift reads behind the last) in LDS
  const int pitch = 2 * ((gy + 63) / 64) + 1;
  const size_t shmem = (flags & IPPM_LIBRARY_TRANSPOSE) ? (size_t)32 * pitch * 4 : 0;
  if (shmem > 65536) { ippm_set_error(who + ": IPPM_LIBRARY_TRANSPOSE needs grid_y <= 16320"); return -1; }
  const uint64_t seed = ctx->cfg.philox_seed;
  const LibArgs a = {episode, lib, draws, truth, (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), n_maps, lgx, lgy, (lgy + 31) / 32,
                     gx, gy, flags, (uint32_t)words, (uint32_t)parts, pitch};
  IPPM_LAUNCH_SH(ctx, IPPM_T_TERRAIN, k_library_draw, dim3((unsigned)((size_t)n_envs * parts)), dim3(256), shmem, S_(stream), a);
  IPPM_LAUNCH_CHECK("ippm_terrain_library_draw");
  return 0;
}
