// The per-round rollout log of the training mission (coma_mission.py:174-267; restated by ippmarl/metrics.py return_scalars and the count
// expressions of COMAMission.add_to_tensorboard): mean / population std / max / min of the absolute episode returns, the per-step relative
// rewards and the relative episode returns, one histogram of the actions flown and one of the altitude levels reached.  One small kernel per
// rollout step writes that step's share into a caller-owned blob; ONE closing kernel writes double out[12] and int64 counts[65].
//
// Contract ("Native rollout log").  A step call stores both reward columns of its (wave, step) slot as float32 and the
// slot's integer bins, one set of 65 per workgroup of RL_ROWS (env, agent) rows: a wavefront counts a bin by ballot, its lanes add their bins
// into LDS (integer atomics: exact in any order), the workgroup writes the 65 sums.  The closing kernel is one workgroup.  An episode's return
// is the float32 sum of its step rewards in step order, starting from the first one.  Every element is converted to double before it enters a
// statistic.  A thread owns L = max(2, ceil(episodes / 256) rounded up to even) consecutive episodes (wave-major, then env) and forms the
// moments (n, sum, M2) of its share of each series in two passes (the sum, then the squares around its own mean); the 256 shares are merged
// by Chan's formula in one fixed tree (neighbours first over the wavefront, the four wavefronts through LDS in order).  No floating-point
// atomics, no workgroup waits on another, every step call overwrites everything of its slot that is ever read: the result depends on the
// inputs and the sizes only.
//
// Blob (4-byte words), wave-major: slot (w, t) at (w * n_steps + t) * slot_words; a slot holds relative float [E], absolute float [E], then
// int32 [G][RL_BINS_PAD] bins, G = ceil(E * N / RL_ROWS); slot_words is rounded up to a multiple of 4.  The layout does not depend on n_waves:
// a closing call may reduce any prefix of the waves the blob was sized for.
#include <cmath>
#include <initializer_list>

#include "ippm_internal.h"

namespace {

constexpr int RL_ROWS = IPPM_ROLLOUT_ROWS;      // (env, agent) rows of one workgroup: 4 per thread
constexpr int RL_BINS = IPPM_ROLLOUT_COUNTS;    // 32 actions, 32 altitude levels, 1 "in no bin"
constexpr int RL_BINS_PAD = 68;
constexpr int RL_BAD = 64;

struct Mom { double n, s, m2; };

__device__ __forceinline__ Mom mom_merge(const Mom a, const Mom b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  const double n = a.n + b.n;
  const double delta = b.s / b.n - a.s / a.n;
  return Mom{n, a.s + b.s, a.m2 + b.m2 + delta * delta * (a.n * b.n / n)};
}

// min / max that keep a NaN once they have seen one (np.min / np.max)
__device__ __forceinline__ double nan_min(double a, double b) { return a != a ? a : (b != b || b < a) ? b : a; }
__device__ __forceinline__ double nan_max(double a, double b) { return a != a ? a : (b != b || b > a) ? b : a; }

// The fixed tree of the 256-thread workgroup (the one of csrc/metrics.hip): neighbours first, then the four wavefronts in order.
__device__ Mom block_mom(Mom m, double* lds, int tid) {
  for (int off = 1; off < 64; off <<= 1) {
    const Mom o{__shfl_down(m.n, off), __shfl_down(m.s, off), __shfl_down(m.m2, off)};
    m = mom_merge(m, o);
  }
  if ((tid & 63) == 0) { lds[3 * (tid >> 6)] = m.n; lds[3 * (tid >> 6) + 1] = m.s; lds[3 * (tid >> 6) + 2] = m.m2; }
  __syncthreads();
  Mom r{lds[0], lds[1], lds[2]};
  for (int w = 1; w < 4; ++w) r = mom_merge(r, Mom{lds[3 * w], lds[3 * w + 1], lds[3 * w + 2]});
  __syncthreads();
  return r;
}

template <bool MAX>
__device__ double block_ext(double v, double* lds, int tid) {
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_down(v, off);
    v = MAX ? nan_max(v, o) : nan_min(v, o);
  }
  if ((tid & 63) == 0) lds[tid >> 6] = v;
  __syncthreads();
  double r = lds[0];
  for (int w = 1; w < 4; ++w) r = MAX ? nan_max(r, lds[w]) : nan_min(r, lds[w]);
  __syncthreads();
  return r;
}

__host__ __device__ inline int64_t rl_groups(int64_t E, int64_t N) { return (E * N + RL_ROWS - 1) / RL_ROWS; }
__host__ __device__ inline int64_t rl_slot_words(int64_t E, int64_t N) { return (2 * E + rl_groups(E, N) * RL_BINS_PAD + 3) & ~(int64_t)3; }

// Workgroup g: rows [g RL_ROWS, (g + 1) RL_ROWS) of action / pos into its own 65 bins, and envs of the same index range into the two reward
// columns (E <= E N, so the grid that covers the rows covers the envs).
__global__ void __launch_bounds__(256)
k_rollout_log_step(float* slot, const float* reward, const float* agent_reward, const int32_t* action, const int32_t* pos,
                   const int32_t* n_active, int E, int N, int A, int min_alt, int spacing, int levels) {
  __shared__ int bins[RL_BINS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t rows = (int64_t)E * N;
  const int64_t base = (int64_t)blockIdx.x * RL_ROWS;
  if (tid < RL_BINS) bins[tid] = 0;
  __syncthreads();

  int mine = 0, bad = 0;      // lane b of a wavefront carries bin b of that wavefront; every lane carries its own "in no bin" entries
#pragma unroll
  for (int k = 0; k < RL_ROWS / 256; ++k) {
    const int64_t r0 = base + 256 * k + (tid & ~63);      // the wavefront's first row of this trip: wavefront-uniform
    if (r0 >= rows) break;
    const int64_t r = r0 + lane;
    int ba = -1, bz = -1;       // bins of this row's action and altitude; -1: the row does not fly (or is past the end)
    if (r < rows) {
      const int e = (int)(r / N), a = (int)(r - (int64_t)e * N);
      if (!n_active || a < n_active[e]) {
        const int act = action[r];
        ba = (act >= 0 && act < A) ? act : RL_BAD;
        const int64_t d = (int64_t)pos[3 * r + 2] - (int64_t)min_alt;
        const int64_t lv = d / spacing;
        bz = (d >= 0 && lv * spacing == d && lv < levels) ? 32 + (int)lv : RL_BAD;
        bad += (ba == RL_BAD) + (bz == RL_BAD);
      }
    }
    for (int b = 0; b < A; ++b) {
      const int c = __popcll(__ballot(ba == b));
      if (lane == b) mine += c;
    }
    for (int b = 0; b < levels; ++b) {
      const int c = __popcll(__ballot(bz == 32 + b));
      if (lane == 32 + b) mine += c;
    }
  }
  if (mine) atomicAdd(&bins[lane], mine);
  if (bad) atomicAdd(&bins[RL_BAD], bad);

  float* rel = slot;
  float* ab = slot + E;
#pragma unroll
  for (int k = 0; k < RL_ROWS / 256; ++k) {
    const int64_t e = base + 256 * k + tid;
    if (e < E) {
      const float* src = reward + 2 * e;
      if (agent_reward) {      // DeepQ: the row of the last agent that flies (clamped into the table: nothing out of range is read)
        int last = (n_active ? n_active[e] : N) - 1;
        last = last < 0 ? 0 : last >= N ? N - 1 : last;
        src = agent_reward + 2 * (e * N + last);
      }
      rel[e] = src[0];
      ab[e] = src[1];
    }
  }
  __syncthreads();
  if (tid < RL_BINS) reinterpret_cast<int*>(slot + 2 * (int64_t)E)[(int64_t)blockIdx.x * RL_BINS_PAD + tid] = bins[tid];
}

// One workgroup.  Series 0: absolute returns, 1: per-step relative rewards, 2: relative returns.
__global__ void __launch_bounds__(256)
k_rollout_log_finalize(const float* blob, int W, int T, int E, int N, double* out, int64_t* counts) {
  __shared__ double lds[12];
  const int tid = threadIdx.x;
  const int64_t words = rl_slot_words(E, N);
  const int64_t G = rl_groups(E, N);
  const int64_t n = (int64_t)W * E;
  int64_t L = (n + 255) / 256;
  L = L < 2 ? 2 : (L + 1) & ~(int64_t)1;
  const int64_t lo = tid * L < n ? tid * L : n;
  const int64_t hi = lo + L < n ? lo + L : n;
  const double cnt = (double)(hi - lo);

  double s[3] = {0.0, 0.0, 0.0}, m2[3] = {0.0, 0.0, 0.0}, mean[3] = {0.0, 0.0, 0.0};
  double mx[3] = {-INFINITY, -INFINITY, -INFINITY}, mn[3] = {INFINITY, INFINITY, INFINITY};
  for (int pass = 0; pass < 2; ++pass) {
    for (int64_t j = lo; j < hi; ++j) {
      const int64_t w = j / E, e = j - w * E;
      const float* p = blob + w * T * words + e;
      float ret = 0.f, aret = 0.f;
      for (int t = 0; t < T; ++t, p += words) {
        const float r = p[0], a = p[E];
        ret = t ? ret + r : r;
        aret = t ? aret + a : a;
        const double x = (double)r;
        if (pass == 0) { s[1] += x; mx[1] = nan_max(mx[1], x); mn[1] = nan_min(mn[1], x); }
        else { const double d = x - mean[1]; m2[1] += d * d; }
      }
      const double xa = (double)aret, xr = (double)ret;
      if (pass == 0) {
        s[0] += xa; mx[0] = nan_max(mx[0], xa); mn[0] = nan_min(mn[0], xa);
        s[2] += xr; mx[2] = nan_max(mx[2], xr); mn[2] = nan_min(mn[2], xr);
      } else {
        const double da = xa - mean[0], dr = xr - mean[2];
        m2[0] += da * da;
        m2[2] += dr * dr;
      }
    }
    if (pass == 0 && cnt > 0.0) { mean[0] = s[0] / cnt; mean[1] = s[1] / (cnt * T); mean[2] = s[2] / cnt; }
  }
  for (int q = 0; q < 3; ++q) {
    const Mom all = block_mom(Mom{q == 1 ? cnt * T : cnt, s[q], m2[q]}, lds, tid);
    const double hi_v = block_ext<true>(mx[q], lds, tid);
    const double lo_v = block_ext<false>(mn[q], lds, tid);
    if (tid == 0) {
      out[4 * q] = all.s / all.n;
      out[4 * q + 1] = sqrt(all.m2 / all.n);      // population std (np.std); one element: 0
      out[4 * q + 2] = hi_v;
      out[4 * q + 3] = lo_v;
    }
  }
  if (tid < RL_BINS) {
    int64_t c = 0;
    const int* p = reinterpret_cast<const int*>(blob) + 2 * (int64_t)E + tid;
    for (int64_t sl = 0; sl < (int64_t)W * T; ++sl)
      for (int64_t g = 0; g < G; ++g) c += p[sl * words + g * RL_BINS_PAD];
    counts[tid] = c;
  }
}

bool rl_shape_ok(const std::string& who, int32_t W, int32_t T, int32_t E, int32_t N) {
  if (W < 1 || W > 4096) { ippm_set_error(who + ": n_waves must be in [1, 4096]"); return false; }
  if (T < 1 || T > 4096) { ippm_set_error(who + ": n_steps must be in [1, 4096]"); return false; }
  if (E < 1 || E > (1 << 20)) { ippm_set_error(who + ": n_envs must be in [1, 2^20]"); return false; }
  if (N < 1 || N > 32) { ippm_set_error(who + ": n_agents must be in [1, 32]"); return false; }
  return true;
}

bool rl_aligned(const std::string& who, std::initializer_list<const void*> ptrs, uintptr_t mask, const char* what) {
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) & mask) { ippm_set_error(who + what); return false; }
  return true;
}

}  // namespace

extern "C" int ippm_rollout_log_bytes(int32_t n_waves, int32_t n_steps, int32_t n_envs, int32_t n_agents, int64_t* bytes) {
  const std::string who = "ippm_rollout_log_bytes";
  if (!bytes) { ippm_set_error(who + ": null argument"); return -1; }
  if (!rl_shape_ok(who, n_waves, n_steps, n_envs, n_agents)) return -1;
  *bytes = 4 * (int64_t)n_waves * n_steps * rl_slot_words(n_envs, n_agents);
  return 0;
}

extern "C" int ippm_rollout_log_step(void* log, int32_t wave, int32_t step, int32_t n_waves, int32_t n_steps, const float* reward,
                                     const float* agent_reward, const int32_t* action, const int32_t* pos, const int32_t* n_active,
                                     int32_t n_envs, int32_t n_agents, int32_t n_actions, int32_t min_altitude, int32_t spacing,
                                     int32_t n_levels, void* stream) {
  const std::string who = "ippm_rollout_log_step";
  if (!log || !reward || !action || !pos) { ippm_set_error(who + ": null argument"); return -1; }
  if (!rl_shape_ok(who, n_waves, n_steps, n_envs, n_agents)) return -1;
  if (wave < 0 || wave >= n_waves) { ippm_set_error(who + ": wave must be in [0, n_waves)"); return -1; }
  if (step < 0 || step >= n_steps) { ippm_set_error(who + ": step must be in [0, n_steps)"); return -1; }
  if (n_actions < 2 || n_actions > 32) { ippm_set_error(who + ": n_actions must be in [2, 32]"); return -1; }
  if (n_levels < 1 || n_levels > 32) { ippm_set_error(who + ": n_levels must be in [1, 32]"); return -1; }
  if (spacing < 1) { ippm_set_error(who + ": spacing must be at least 1"); return -1; }
  if (!rl_aligned(who, {log}, 15, ": the blob must be 16-byte aligned")) return -1;
  if (!rl_aligned(who, {reward, agent_reward, action, pos, n_active}, 3, ": the arrays must be 4-byte aligned")) return -1;
  float* slot = static_cast<float*>(log) + ((int64_t)wave * n_steps + step) * rl_slot_words(n_envs, n_agents);
  hipLaunchKernelGGL(k_rollout_log_step, dim3((unsigned)rl_groups(n_envs, n_agents)), dim3(256), 0, S_(stream), slot, reward, agent_reward,
                     action, pos, n_active, (int)n_envs, (int)n_agents, (int)n_actions, (int)min_altitude, (int)spacing, (int)n_levels);
  IPPM_LAUNCH_CHECK("ippm_rollout_log_step");
  return 0;
}

extern "C" int ippm_rollout_log_finalize(const void* log, int32_t n_waves, int32_t n_steps, int32_t n_envs, int32_t n_agents, double* out,
                                         int64_t* counts, void* stream) {
  const std::string who = "ippm_rollout_log_finalize";
  if (!log || !out || !counts) { ippm_set_error(who + ": null argument"); return -1; }
  if (!rl_shape_ok(who, n_waves, n_steps, n_envs, n_agents)) return -1;
  if (!rl_aligned(who, {log}, 15, ": the blob must be 16-byte aligned")) return -1;
  if (!rl_aligned(who, {out, counts}, 7, ": out and counts must be 8-byte aligned")) return -1;
  hipLaunchKernelGGL(k_rollout_log_finalize, dim3(1), dim3(256), 0, S_(stream), static_cast<const float*>(log), (int)n_waves, (int)n_steps,
                     (int)n_envs, (int)n_agents, out, counts);
  IPPM_LAUNCH_CHECK("ippm_rollout_log_finalize");
  return 0;
}
