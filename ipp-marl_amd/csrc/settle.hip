// ippm_settle_clamps (gfx950): pays the clips that plans made with IPPM_STEP_DEFER_CLAMPS left owed (DESIGN.md "deferred clamp").
//
// A plan that takes messages would put clamp-only ops ahead of its real ops: over region A (the last fusion's last-op rectangle, or
// the hull of the footprints left behind since) and over the agent's last footprint.  Their cells that no real op meets are loaded,
// clipped and stored by the fusion although nothing reads the clipped value before the map is looked at: every later op and K3 clip
// their input themselves, the reset discards the cells, and the reward terms of such a cell are exact zeros.  A deferring plan
// remembers those rectangles as ONE bounding box per map (the backlog's OWED) and this kernel clips, once, when the map is about to
// be read, every cell of the box that is not LEGITIMATELY unclamped at that moment:
//   - the last fusion's last-op rectangle (RECT_A while the LEGIT list is empty and FLAG_A is set),
//   - every rectangle of the LEGIT list (footprints K3 left behind while the agent heard nobody; RECT_A is then only their hull),
//   - the agent's current footprint when FLAG_S is set.
// Exact, cell by cell: a cell of the box that is neither owed nor legit is in range already (a clip changes nothing), an owed cell in
// a gap of a hull is clipped, a legit cell stays as it is (it is observable: the reference leaves a fusion's last outputs unclipped).
#include <algorithm>

#include "ippm_tiles.h"

#define IPPM_SETTLE_RECTS 64   // LEGIT entries + region A + the current footprint held in LDS (budget + 4 <= 64: checked at registration)

// One workgroup per map: the box's lane-loads (16 bytes: 4 grid-aligned cells of a row) are dealt out to the 256 threads in
// row-major order (TL: in the order of tile storage, rows of tiles x lane-loads, so that 8 consecutive lanes cover a line).
// Only lane-loads with a changed cell are stored.  Nobody else touches the map's backlog during the launch: thread 0 empties OWED.
template <bool MIS, bool TL>
__global__ void __launch_bounds__(256)
k_settle_clamps(float* __restrict__ local, float* __restrict__ global, const int32_t* __restrict__ ws, const int32_t* __restrict__ rect,
                int32_t* __restrict__ backlog, int bl_words, int n, int gx, int gy, float lc, unsigned long long* __restrict__ counters) {
  const int map_abs = blockIdx.x, e = map_abs / (n + 1), i = map_abs - e * (n + 1);
  int32_t* bl = backlog + (size_t)map_abs * bl_words;
  const int bx = bl[BL_OWED_X], by = bl[BL_OWED_Y];
  const int x0 = bx & 0xFFFF, x1 = min((int)((unsigned)bx >> 16), gx), y0 = by & 0xFFFF, y1 = min((int)((unsigned)by >> 16), gy);
  if (x1 <= x0 || y1 <= y0) return;   // nothing owed (uniform)
  const int32_t* w = ws + (size_t)map_abs * IPPM_WS_WORDS;
  __shared__ int4 s_rect[IPPM_SETTLE_RECTS];
  __shared__ int s_n;
  const int nl = bl[BL_LEGIT_N];
  if (threadIdx.x == 0) {
    int k = 0;
    const int4* lr = reinterpret_cast<const int4*>(bl + BL_RECTS);
    for (int q = 0; q < min(max(nl, 0), IPPM_SETTLE_RECTS - 2); ++q) s_rect[k++] = lr[q];
    // an empty list: RECT_A is the fusion's own rectangle.  (An overflowed list, nl < 0, cannot be made exact: the hull stands in, and the
    // box stays owed -- the next plan of the map takes the undeferred path and clips it.  ippm_set_clamp_backlog says how callers avoid this.)
    if (nl <= 0 && w[WS_FLAG_A]) s_rect[k++] = make_int4(w[WS_RECT_A], w[WS_RECT_A + 1], w[WS_RECT_A + 2], w[WS_RECT_A + 3]);
    if (i < n && w[WS_FLAG_S]) s_rect[k++] = *reinterpret_cast<const int4*>(rect + (size_t)(e * n + i) * 4);
    s_n = k;
  }
  __syncthreads();
  const int nr = s_n;
  float* map = i == n ? global + (size_t)e * IPPM_MAP_PITCH(gx, gy) : local + (size_t)(e * n + i) * IPPM_MAP_PITCH(gx, gy);
  const __amdgpu_buffer_rsrc_t rmap = IPPM_RSRC(map, (size_t)gx * gy * 4);
  // the box in lane-loads: rows [r0, r0 + R) x lane-loads [g0, g0 + W) of a row (TL: rows of tiles, 8 lane-loads per tile)
  const int r0 = TL ? x0 >> 2 : x0, R = (TL ? (x1 + 3) >> 2 : x1) - r0;
  const int g0 = TL ? (y0 >> 3) << 3 : y0 >> 2, W = (TL ? ((y1 + 7) >> 3) << 3 : (y1 + 3) >> 2) - g0;
  const int total = R * W;
  unsigned changed = 0;
  for (int t = threadIdx.x; t < total; t += 256) {
    const int r = t / W, g = t - r * W;
    int row, col, off;
    if (TL) {
      const ippm_lane_load ll = ippm_tile_lane_load(r0 + r, g0 + g, gy);
      row = ll.row; col = ll.col; off = ll.off;
    } else {
      row = r0 + r; col = (g0 + g) * 4; off = (row * gy + col) * 4;
    }
    // cells col .. col + 3 of `row` that are owed a clip: inside the box, outside every legit rectangle
    unsigned owed = 0;
    if (row >= x0 && row < x1) {
      const int lo = min(max(y0 - col, 0), 4), hi = min(max(y1 - col, 0), 4);
      owed = ((1u << (hi - lo)) - 1u) << lo;
      for (int k = 0; k < nr; ++k) {
        const int4 q = s_rect[k];   // {yu, yd, xl, xr}
        if (row >= q.z && row < q.w) {
          const int a = min(max(q.x - col, 0), 4), b = min(max(q.y - col, 0), 4);
          owed &= ~(((1u << max(b - a, 0)) - 1u) << a);
        }
      }
    }
    if (owed == 0) continue;
    const CellVec<4> v = buf_load_cells<4>(rmap, off);
    CellVec<4> out;
    unsigned diff = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float cl = ippm_clampl(v.v[j], lc);
      const bool ch = ((owed >> j) & 1u) && __float_as_uint(cl) != __float_as_uint(v.v[j]);
      out.v[j] = ch ? cl : v.v[j];
      diff |= ch ? (1u << j) : 0u;
    }
    if (diff == 0) continue;
    changed += __popc(diff);
    // (MIS: a row's last group hangs over into the next row -- owed cells lie inside the row, the store goes out cell by cell there)
    buf_store_cells_tail<4, MIS>(rmap, off, col, gy, out);
  }
  if (threadIdx.x == 0 && nl >= 0) { bl[BL_OWED_X] = 0; bl[BL_OWED_Y] = 0; }
  const float cs = ippm_wave_sum((float)changed);   // (a box holds fewer than 2^24 cells)
  if (counters && (threadIdx.x & 63) == 0 && cs > 0.f)
    atomicAdd(&counters[((map_abs + (threadIdx.x >> 6)) & (IPPM_COUNTER_SLOTS - 1)) * 8 + 7], (unsigned long long)cs);
}

extern "C" int ippm_clamp_backlog_words(ippm_ctx* ctx, int32_t n_envs, int64_t* words) {
  if (!ctx || !words || n_envs < 0) { ippm_set_error("ippm_clamp_backlog_words: bad argument"); return -1; }
  *words = (int64_t)n_envs * (ctx->cfg.n_agents + 1) * ippm_backlog_words(ctx);
  return 0;
}

extern "C" int ippm_set_clamp_backlog(ippm_ctx* ctx, int32_t* backlog) {
  if (!ctx) { ippm_set_error("ippm_set_clamp_backlog: null context"); return -1; }
  if (backlog && (ctx->cfg.grid_x > 0x7FFF || ctx->cfg.grid_y > 0x7FFF)) { ippm_set_error("ippm_set_clamp_backlog: grid too large for a packed box"); return -1; }
  if (backlog && ippm_backlog_cap(ctx) + 2 > IPPM_SETTLE_RECTS) { ippm_set_error("ippm_set_clamp_backlog: budget above 60 steps"); return -2; }
  if (backlog && ctx->vec != 4) { ippm_set_error("ippm_set_clamp_backlog: needs the 16-byte layout (grid_y >= 44)"); return -2; }
  if (backlog && (reinterpret_cast<uintptr_t>(backlog) & 15)) { ippm_set_error("ippm_set_clamp_backlog: needs a 16-byte aligned buffer"); return -1; }
  ctx->backlog = backlog;
  return 0;
}

extern "C" int ippm_settle_clamps(ippm_ctx* ctx, float* local, float* global, const int32_t* ws, const int32_t* rect, int32_t* backlog,
                                  int32_t n_envs, void* stream) {
  if (!ctx || !local || !global || !ws || !rect || !backlog) { ippm_set_error("ippm_settle_clamps: null argument"); return -1; }
  if (backlog != ctx->backlog) { ippm_set_error("ippm_settle_clamps: not the backlog registered with ippm_set_clamp_backlog"); return -1; }
  if (n_envs <= 0) return 0;
  const ippm_config& c = ctx->cfg;
  const dim3 grid((unsigned)(n_envs * (c.n_agents + 1))), block(256);
#define IPPM_SETTLE_L(...) hipLaunchKernelGGL((k_settle_clamps<__VA_ARGS__>), grid, block, 0, S_(stream), local, global, ws, rect, backlog, \
                                              ippm_backlog_words(ctx), c.n_agents, c.grid_x, c.grid_y, c.logit_clip, ctx->dcounters)
  if (ctx->tl) IPPM_SETTLE_L(false, true);
  else if (c.grid_y & 3) IPPM_SETTLE_L(true, false);
  else IPPM_SETTLE_L(false, false);
#undef IPPM_SETTLE_L
  IPPM_LAUNCH_CHECK("settle_clamps");
  return 0;
}
