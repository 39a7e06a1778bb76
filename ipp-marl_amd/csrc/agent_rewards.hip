// DeepQ per-agent information-gain rewards (gfx950): for every agent i of an env, get_global_reward(K, K (+) m_i) of fusing ONLY
// agent i's fresh measurement into the step's global map K.
//
//   coma_wrapper.py:113-133 (mission type "DeepQ")   fuse_map(critic_map_knowledge, [maps2communicate[i]]) + get_global_reward
//   mappings.py:109-124                               the update: clip every cell of K, add the measurement's log-odds - logit(prior)
//   utils/reward.py:25-40,68-82, utils/state.py:53-121 S1, S2 and the "reward"-mode class weights of the AFTER map
//
// S1_i = sum w(K (+) m_i) (H(K) - H(K (+) m_i)) and S2_i = sum w(K (+) m_i) H(K) = T + sum (w(K (+) m_i) - w(K)) H(K), T = sum w(K) H(K)
// being the running weighted entropy the COMA reward keeps in sums[e][2].  With prior 0.5 a cell outside agent i's footprint keeps its
// weight and its (clipped) entropy, so only the footprint is walked; with any other prior every cell shifts by -logit(prior) and the
// whole grid is walked (the slow path, as in the fusion: float64 chain and entropies).  The per-cell arithmetic -- clip, entropy from
// log-odds, class weight, the reward expression -- is the COMA reward's own (ippm_internal.h), so the two rewards cannot drift apart.
//
// Shape: one workgroup per (env, agent), the footprint's 4-cell groups spread over its lanes with four 16-byte buffer loads in flight
// per lane (OOB offsets for lanes without a cell: loads return 0), reduced in the workgroup: no zero-fill launch, no cross-workgroup
// hand-off.  Under tile storage the lanes walk whole tiles: 8 consecutive lanes = the 2 groups x 4 rows of one 128-byte tile.
#include "ippm_tiles.h"

#define IPPM_AR_THREADS 256
#define IPPM_AR_UNR 4   // cell groups in flight per lane

template <int VEC, bool SHIFT, bool TL>
__global__ __launch_bounds__(IPPM_AR_THREADS) void k_agent_rewards(const ippm_config* __restrict__ c, const float* __restrict__ global,
                                                                   const uint8_t* __restrict__ code, const int32_t* __restrict__ rec,
                                                                   const double* __restrict__ sums, double* __restrict__ agent_sums,
                                                                   float* __restrict__ agent_reward, const int32_t* __restrict__ n_active) {
  const int n = c->n_agents;
  const int ei = blockIdx.x, e = ei / n, i = ei - e * n;
  if (n_active && i >= n_active[e]) {   // not flying in this env (ippm_set_team_sizes): 0
    if (threadIdx.x < 2) {
      agent_reward[(size_t)ei * 2 + threadIdx.x] = 0.f;
      if (agent_sums) agent_sums[(size_t)ei * 2 + threadIdx.x] = 0.0;
    }
    return;
  }
  const int32_t* r = rec + (size_t)ei * IPPM_SENSE_REC_WORDS;
  const int yu = r[0], yd = r[1], xl = r[2], xr = r[3];
  const float lm0 = __int_as_float(r[4]), lm1 = __int_as_float(r[5]);   // measurement log-odds - logit(prior)
  const int gx = c->grid_x, gy = c->grid_y, S = c->tile_stride;
  const int h = xr - xl, w = yd - yu;
  const bool fp = h > 0 && w > 0;
  const float lc = c->logit_clip, wt = c->logit_weight_thr;
  const double lp64 = c->logit_prior_f64;
  // the walk: the footprint (prior 0.5; nothing when it is empty: S1 = 0, S2 = T), the whole grid (SHIFT)
  const int xa = SHIFT ? 0 : (fp ? xl : 0), xb = SHIFT ? gx : (fp ? xr : 0);
  const int ya = SHIFT ? 0 : yu, yb = SHIFT ? gy : yd;
  const int y0 = ya & ~(VEC - 1);
  const int groups = xb > xa ? (yb - y0 + VEC - 1) / VEC : 0;
  const int x0 = TL ? (xa & ~3) : xa;
  const int rows = xb - x0;
  const int items = TL ? ((rows + 3) >> 2) * groups * 4 : rows * groups;
  const float inv_groups = __builtin_amdgcn_rcpf((float)max(groups, 1));
  const __amdgpu_buffer_rsrc_t rmap = IPPM_RSRC(global + (size_t)e * IPPM_MAP_PITCH(gx, gy), (size_t)gx * gy * 4);
  const size_t TB = ippm_tile_bytes(S, VEC);
  const __amdgpu_buffer_rsrc_t rcode = IPPM_RSRC(code + (size_t)ei * TB, TB);
  const int tile_y0 = yu & ~3;
  double a1 = 0.0, aD = 0.0;   // float64 lane sums of w(a) (H(b) - H(a)) and (w(a) - w(b)) H(b)
  for (int base = threadIdx.x; base < items; base += IPPM_AR_THREADS * IPPM_AR_UNR) {
    CellVec<VEC> v[IPPM_AR_UNR];
    uint32_t bits[IPPM_AR_UNR];
    int xs[IPPM_AR_UNR], ys[IPPM_AR_UNR];
    bool ok[IPPM_AR_UNR];
#pragma unroll
    for (int u = 0; u < IPPM_AR_UNR; ++u) {
      const int it = base + u * IPPM_AR_THREADS;
      int x, g;
      if (TL) {   // lane order (row quad, group, row in quad): 8 lanes = one whole tile
        const int rest = it >> 2, q = ippm_div_small(rest, inv_groups);
        g = rest - q * groups;
        x = x0 + 4 * q + (it & 3);
      } else {
        const int q = ippm_div_small(it, inv_groups);
        g = it - q * groups;
        x = x0 + q;
      }
      const int y = y0 + g * VEC;
      const bool valid = it < items && x >= xa && x < xb;
      xs[u] = x; ys[u] = y; ok[u] = valid;
      const int off = valid ? ippm_cell_index(x, y, gy, TL ? 1 : 0) * 4 : IPPM_OOB;
      v[u] = buf_load_cells<VEC>(rmap, off);
      // the group's measurement bits, for a group that meets the footprint
      const bool meets = valid && fp && (unsigned)(x - xl) < (unsigned)h && y + VEC > yu && y < yd;
      bits[u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rcode, meets ? (int)tile_index<VEC>(x - xl, y - tile_y0, S) : IPPM_OOB, 0, 0) &
                (VEC == 4 ? 0xFu : 1u);
    }
#pragma unroll
    for (int u = 0; u < IPPM_AR_UNR; ++u) {
      const int x = xs[u], y = ys[u];
      const bool rowin = ok[u] && fp && (unsigned)(x - xl) < (unsigned)h;
      if (SHIFT) {
        // every cell of the grid: a = clip(K) + (measurement - logit(prior)) inside the footprint, clip(K) - logit(prior) outside;
        // the chain in float64 and rounded once, as the fusion's SHIFT path stores it
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          if (!ok[u] || y + q >= gy) continue;
          const bool in = rowin && (unsigned)(y + q - yu) < (unsigned)w;
          const float b = v[u].v[q];
          const double kc = fmin(fmax((double)b, -(double)lc), (double)lc);
          const float a = (float)(kc + (in ? (double)(((bits[u] >> q) & 1u) ? lm1 : lm0) : -lp64));
          const float wa = ippm_weight_l(a, wt), wb = ippm_weight_l(b, wt);
          if (wa != 0.f || wb != 0.f) {
            const double hb = entropy_l_f64(b, lc), ha = entropy_l_f64(a, lc);
            a1 += (double)wa * (hb - ha);
            aD += (double)(wa - wb) * hb;
          }
        }
      } else {
        // the footprint's cells; cells of an edge group outside it contribute exact zeros (weights 0)
        float av[VEC], wa[VEC], wb[VEC], wsum = 0.f;
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
          const bool in = rowin && (unsigned)(y + q - yu) < (unsigned)w;
          av[q] = ippm_clampl(v[u].v[q], lc) + (((bits[u] >> q) & 1u) ? lm1 : lm0);
          wa[q] = in ? ippm_weight_l(av[q], wt) : 0.f;
          wb[q] = in ? ippm_weight_l(v[u].v[q], wt) : 0.f;
          wsum += wa[q] + wb[q];
        }
        // groups whose cells are believed free before and after (all weights 0) skip the entropies: wave-uniform on coherent terrain
        if (__any(wsum != 0.f)) {
          float r1 = 0.f, rD = 0.f;
#pragma unroll
          for (int q = 0; q < VEC; ++q) {
            const float hb = ippm_entropy_l(v[u].v[q], lc), ha = ippm_entropy_l(av[q], lc);
            r1 += wa[q] * (hb - ha);
            rD += (wa[q] - wb[q]) * hb;
          }
          a1 += (double)r1;
          aD += (double)rD;
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a1 += __shfl_xor(a1, o, 64); aD += __shfl_xor(aD, o, 64); }
  __shared__ double s_red[2][IPPM_AR_THREADS / 64];
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_red[0][wv] = a1; s_red[1][wv] = aD; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s1 = 0.0, d = 0.0;
#pragma unroll
    for (int k = 0; k < IPPM_AR_THREADS / 64; ++k) { s1 += s_red[0][k]; d += s_red[1][k]; }
    const double s2 = sums[(size_t)e * 8 + SUM_T] + d;
    ippm_reward_pair(c, s1, s2, agent_reward + (size_t)ei * 2);
    if (agent_sums) { agent_sums[(size_t)ei * 2] = s1; agent_sums[(size_t)ei * 2 + 1] = s2; }
  }
}

extern "C" int ippm_agent_rewards(ippm_ctx* ctx, const float* global, const uint8_t* code, const int32_t* rect, const double* sums,
                                  double* agent_sums, float* agent_reward, int32_t n_envs, void* stream) {
  if (!ctx || !global || !code || !rect || !sums || !agent_reward) { ippm_set_error("ippm_agent_rewards: null argument"); return -1; }
  if (n_envs <= 0) return 0;
  const ippm_config& c = ctx->cfg;
  const dim3 grid((unsigned)n_envs * (unsigned)c.n_agents), block(IPPM_AR_THREADS);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool shift = c.logit_prior != 0.f;   // (the fusion's choice of its SHIFT path)
#define IPPM_AR_L(V, SH, T) \
  IPPM_LAUNCH(ctx, IPPM_T_AGENT_REWARD, (k_agent_rewards<V, SH, T>), grid, block, st, ctx->dcfg, global, code, rect, sums, agent_sums, agent_reward, ctx->n_active)
  if (ctx->tl) {   // (tile storage implies 16-byte lane groups and prior 0.5: ippm_tile_storage_ok)
    IPPM_AR_L(4, false, true);
  } else if (ctx->vec == 4) {
    if (shift) IPPM_AR_L(4, true, false);
    else IPPM_AR_L(4, false, false);
  } else {
    if (shift) IPPM_AR_L(1, true, false);
    else IPPM_AR_L(1, false, false);
  }
#undef IPPM_AR_L
  IPPM_LAUNCH_CHECK("ippm_agent_rewards");
  return 0;
}
