// Scoring of belief maps against the ground truth (coma_test.py:84-97,150-196, IG_baseline.py:84-97, utils/utils.py:64-76): per map the
// entropy summed over the target cells and the target class's (tp, fp, fn) at the three log-odds thresholds (+delta, 0, -delta), from ONE
// streaming read of the maps (4 B + 1 bit per cell).  Deterministic by construction: a workgroup scores a fixed part of one map and stores
// its ten partial sums, a second small kernel adds a map's partials in part order -- no atomics, no ticket -- and the parts of a map depend on
// the grid alone, so that a map scores the same alone and in any batch, bit for bit.

#include "ippm_tiles.h"

#define SCORE_THREADS 256
#define SCORE_SLOTS 8                                     // 16-byte loads in flight per lane: 32 KiB per workgroup
#define SCORE_PART_GROUPS (SCORE_SLOTS * SCORE_THREADS)   // 4-cell groups of a part: 2048 = 8192 cells
#define SCORE_WORDS 10                                    // partial sums of a part: the entropy (double), then 3 x (tp, fp, fn) (int64)

// parts a map is scored in (by the grid only) -- its last part also takes the 1..3 tail cells of a map that is not a multiple of 4 cells
static inline int score_parts(const ippm_ctx* ctx) {
  const size_t groups = IPPM_MAP_PITCH(ctx->cfg.grid_x, ctx->cfg.grid_y) / 4;
  return (int)std::max<size_t>(1, (groups + SCORE_PART_GROUPS - 1) / SCORE_PART_GROUPS);
}

struct ScoreAcc {
  double h;        // entropy over the target cells
  int n[9];        // [threshold][tp, fp, fn]
};

// One group of four cells: `t` its truth bits, `valid` the cells that exist (0xF, less for a map's tail, 0 for a lane without work).
__device__ __forceinline__ void score_group(ScoreAcc& a, const CellVec<4>& v, uint32_t t, uint32_t valid, float lc, float delta) {
  uint32_t p[3] = {0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    p[0] |= v.v[j] > delta ? 1u << j : 0u;
    p[1] |= v.v[j] > 0.f ? 1u << j : 0u;
    p[2] |= v.v[j] > -delta ? 1u << j : 0u;
  }
  const uint32_t nt = valid & ~t;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.n[3 * k + 0] += __popc(p[k] & t);
    a.n[3 * k + 1] += __popc(p[k] & nt);
    a.n[3 * k + 2] += __popc(~p[k] & t);
  }
  if (t) {   // entropy only where the group holds a target cell: H(sigmoid(clamp(L))) in the series form (ippm_entropy_from_e)
    float h = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float b = fminf(fabsf(v.v[j]), lc);
      float rd;
      h += ippm_masked(ippm_bitmask(t, j), ippm_entropy_from_e(b, __expf(-b), rd));
    }
    a.h += (double)h;   // (float32 over a group's four cells, float64 from there on: as the tile fusion sums its reward terms)
  }
}

// Workgroup (part, map): lane-load q of the part is the 16-byte group part * 2048 + q * 256 + thread of the map's stored floats -- four cells
// of one row in either layout, at 4-byte alignment when a map is not a multiple of 4 cells (the second map of a 45 x 45 batch; gfx950 serves
// 16-byte accesses there).  All eight loads go out before the first use; loads of lanes without work point past the resource and return 0.
template <bool TL>
__global__ void __launch_bounds__(SCORE_THREADS)
k_score_maps(const float* __restrict__ maps, const uint8_t* __restrict__ truth, double* __restrict__ scratch, uint32_t cells, int gy, int parts,
             int maps_per_truth, uint32_t truth_bytes, float lc, float delta) {
  const int m = blockIdx.x / parts, part = blockIdx.x - m * parts;
  const __amdgpu_buffer_rsrc_t rs = IPPM_RSRC(maps + (size_t)m * cells, (size_t)cells * 4);
  const uint8_t* tr = truth + (size_t)(m / maps_per_truth) * truth_bytes;
  const uint32_t full = cells >> 2, g0 = (uint32_t)part * SCORE_PART_GROUPS + threadIdx.x;
  CellVec<4> v[SCORE_SLOTS];
  uint32_t t[SCORE_SLOTS];
#pragma unroll
  for (int q = 0; q < SCORE_SLOTS; ++q) {
    const uint32_t g = g0 + q * SCORE_THREADS;
    v[q] = buf_load_cells<4>(rs, g < full ? (int)(g * 16u) : IPPM_OOB);
  }
#pragma unroll
  for (int q = 0; q < SCORE_SLOTS; ++q) {
    const uint32_t g = g0 + q * SCORE_THREADS;
    // the cell number of the group's first float (gy & 0xFFFF and the 32-bit index: the tile layout's division then is a 32-bit one)
    const size_t lin = g < full ? ippm_stored_cell((size_t)(g * 4u), gy & 0xFFFF, TL) : 0;
    t[q] = g < full ? ippm_truth4(tr, lin, truth_bytes) : 0u;
  }
  ScoreAcc a;
  a.h = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) a.n[k] = 0;
#pragma unroll
  for (int q = 0; q < SCORE_SLOTS; ++q) score_group(a, v[q], t[q], g0 + q * SCORE_THREADS < full ? 0xFu : 0u, lc, delta);
  const uint32_t rem = cells & 3u;
  if (!TL && rem && part == parts - 1 && threadIdx.x == 0) {   // the map's last 1..3 cells, float by float
    CellVec<4> w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w.v[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (uint32_t)j < rem ? (int)((full * 4u + j) * 4u) : IPPM_OOB, 0, 0));
    const uint32_t valid = (1u << rem) - 1u;
    score_group(a, w, ippm_truth4(tr, (size_t)full * 4, truth_bytes) & valid, valid, lc, delta);
  }
  // wavefront sums (a butterfly: the same order whatever the data), then the four wavefronts in order
  __shared__ double s_h[SCORE_THREADS / 64];
  __shared__ int s_n[SCORE_THREADS / 64][9];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.h += __shfl_xor(a.h, o, 64);
#pragma unroll
    for (int k = 0; k < 9; ++k) a.n[k] += __shfl_xor(a.n[k], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_h[threadIdx.x >> 6] = a.h;
#pragma unroll
    for (int k = 0; k < 9; ++k) s_n[threadIdx.x >> 6][k] = a.n[k];
  }
  __syncthreads();
  double* out = scratch + (size_t)blockIdx.x * SCORE_WORDS;
  if (threadIdx.x == 0) out[0] = ((s_h[0] + s_h[1]) + s_h[2]) + s_h[3];
  else if (threadIdx.x < SCORE_WORDS) {
    const int k = threadIdx.x - 1;
    reinterpret_cast<long long*>(out)[threadIdx.x] = (long long)(s_n[0][k] + s_n[1][k] + s_n[2][k] + s_n[3][k]);
  }
}

// thread (map, word): the map's partials of that word, added in part order
__global__ void __launch_bounds__(256)
k_score_sum(const double* __restrict__ scratch, double* __restrict__ entropy, long long* __restrict__ counts, int parts, int n_maps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_maps * SCORE_WORDS) return;
  const int m = i / SCORE_WORDS, k = i - m * SCORE_WORDS;
  const double* p = scratch + (size_t)m * parts * SCORE_WORDS + k;
  if (k == 0) {
    double s = 0.0;
    for (int q = 0; q < parts; ++q) s += p[(size_t)q * SCORE_WORDS];
    entropy[m] = s;
  } else {
    long long s = 0;
    for (int q = 0; q < parts; ++q) s += reinterpret_cast<const long long*>(p)[(size_t)q * SCORE_WORDS];
    counts[(size_t)m * 9 + k - 1] = s;
  }
}

extern "C" int ippm_score_scratch(ippm_ctx* ctx, int32_t n_maps, int64_t* doubles) {
  if (!ctx || !doubles || n_maps < 0) { ippm_set_error("ippm_score_scratch: bad argument"); return -1; }
  *doubles = (int64_t)n_maps * score_parts(ctx) * SCORE_WORDS;
  return 0;
}

extern "C" int ippm_score_maps(ippm_ctx* ctx, const float* maps, const uint8_t* truth, int32_t maps_per_truth, float logodds_delta,
                               double* entropy, int64_t* counts, double* scratch, int32_t n_maps, void* stream) {
  if (!ctx || !maps || !truth || !entropy || !counts || !scratch) { ippm_set_error("ippm_score_maps: null argument"); return -1; }
  if (n_maps <= 0) return 0;
  const size_t cells = IPPM_MAP_PITCH(ctx->cfg.grid_x, ctx->cfg.grid_y);
  const int parts = score_parts(ctx);
  // (a lane addresses its map through a 32-bit byte offset; the launch is one-dimensional)
  if (cells * 4 > (size_t)IPPM_OOB) { ippm_set_error("ippm_score_maps: maps of 2 GB or more"); return -2; }
  if ((size_t)n_maps * parts > 0x7FFFFFFFu / SCORE_WORDS) { ippm_set_error("ippm_score_maps: too many maps for one launch"); return -2; }
  if (!(logodds_delta >= 0.f)) { ippm_set_error("ippm_score_maps: logodds_delta must not be negative"); return -2; }
  const dim3 grid((unsigned)(n_maps * parts)), block(SCORE_THREADS);
  const int mpt = maps_per_truth > 0 ? maps_per_truth : 1;
  const uint32_t tb = (uint32_t)ippm_truth_bytes(ctx->cfg.grid_x, ctx->cfg.grid_y);
  if (ctx->tl)
    hipLaunchKernelGGL(k_score_maps<true>, grid, block, 0, S_(stream), maps, truth, scratch, (uint32_t)cells, ctx->cfg.grid_y, parts, mpt, tb,
                       ctx->cfg.logit_clip, logodds_delta);
  else
    hipLaunchKernelGGL(k_score_maps<false>, grid, block, 0, S_(stream), maps, truth, scratch, (uint32_t)cells, ctx->cfg.grid_y, parts, mpt, tb,
                       ctx->cfg.logit_clip, logodds_delta);
  IPPM_LAUNCH_CHECK("score_maps");
  hipLaunchKernelGGL(k_score_sum, dim3(grid1((size_t)n_maps * SCORE_WORDS)), dim3(256), 0, S_(stream), scratch, entropy,
                     reinterpret_cast<long long*>(counts), parts, n_maps);
  IPPM_LAUNCH_CHECK("score_sum");
  return 0;
}
