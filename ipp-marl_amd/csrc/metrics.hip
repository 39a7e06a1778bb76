// The per-training-step diagnostics of the COMA round (coma_mission.py:208-424, critic/learner.py:100-190, actor/learner.py:36-200; restated
// by ippmarl/metrics.py): 32 scalars reduced on the device from the arrays a minibatch step has anyway, into a caller-owned blob of partial
// results, with one small kernel per call and ONE closing kernel that writes double out[32].
//
// Contract ("Native metrics").  Every input element is converted to double before anything is done with it; log and exp
// are the double ones.  A workgroup owns IPPM_METRICS_CHUNK rows of one minibatch ("slot"), one row per lane.  Within a chunk every quantity is
// a lane value (or a lane-local sum in index order) reduced by one fixed tree: __shfl_down over the wavefront, the four wavefront results
// through LDS, merged in wavefront order.  Moments travel as (n, sum, M2) -- the mean as its exact numerator -- and are merged by Chan's
// formula; a column's log-sum-exp travels as (max, sum exp(x - max)).  Partials go to the blob; k_metrics_finalize merges the chunks of a slot
// in chunk order, then the slots in slot order.  No atomics, no workgroup waits on another, every call overwrites all partials of its slot (or
// net), so a result depends on the inputs, batch, n_actions and n_minibatches only.
//
// Blob (doubles):  [2 nets][10 tensors][MT_GRAD_PARTS] gradient L1 partials, then per slot: MT_SLOT_HDR header doubles (critic loss, actor
// loss, mean square of hidden0, padding) and one MT_REC record per chunk (the MT_R_* offsets below).
#include <cmath>
#include <initializer_list>

#include "ippm_internal.h"

namespace {

constexpr int MT_CHUNK = IPPM_METRICS_CHUNK;
constexpr int MT_MAX_A = 32;
constexpr int MT_TENSORS = 10;
constexpr int MT_GRAD_PARTS = 64;                                // workgroups (and partials) per gradient tensor
constexpr int MT_GRAD_DOUBLES = 2 * MT_TENSORS * MT_GRAD_PARTS;
constexpr int MT_SLOT_HDR = 4;
constexpr int MT_R_TD = 0, MT_R_DISC = 3, MT_R_DEV = 6, MT_R_DIFF = 9, MT_R_QNEW = 12;   // moments: (n, sum, M2)
constexpr int MT_R_QCH = 15, MT_R_QMIN = 16;                                            // sum of q_chosen, min of q_new
constexpr int MT_R_ADV = 17;                                                            // moments
constexpr int MT_R_LOGC = 20, MT_R_ENT = 21, MT_R_KL = 22;                              // sums over the chunk's rows
constexpr int MT_R_COL = 24;                                                            // per column: max, sum exp, rows that chose it, their q
constexpr int MT_REC = MT_R_COL + 4 * MT_MAX_A;

struct Mom { double n, s, m2; };

__device__ __forceinline__ Mom mom_merge(const Mom a, const Mom b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  const double n = a.n + b.n;
  const double delta = b.s / b.n - a.s / a.n;
  return Mom{n, a.s + b.s, a.m2 + b.m2 + delta * delta * (a.n * b.n / n)};
}

__device__ __forceinline__ Mom mom_load(const double* p) { return Mom{p[0], p[1], p[2]}; }
__device__ __forceinline__ void mom_store(double* p, const Mom m) { p[0] = m.n; p[1] = m.s; p[2] = m.m2; }

// min that keeps a NaN once it has seen one (np.min / torch.min)
__device__ __forceinline__ double nan_min(double a, double b) { return a != a ? a : (b != b || b < a) ? b : a; }

// The fixed tree of a 256-thread workgroup: neighbours first (off = 1, 2, 4, ... 32), so every partial that reaches lane 0 covers an aligned
// block of 2 off consecutive lanes.  Lane 0 of a wavefront reads lane `off`, which at that step holds the merge of lanes off .. 2 off - 1;
// what the upper lanes compute on the way is never read.  Every thread returns the workgroup's result.
__device__ Mom block_mom(Mom m, double* lds, int tid) {
  for (int off = 1; off < 64; off <<= 1) {
    const Mom o{__shfl_down(m.n, off), __shfl_down(m.s, off), __shfl_down(m.m2, off)};
    m = mom_merge(m, o);
  }
  if ((tid & 63) == 0) mom_store(lds + 3 * (tid >> 6), m);
  __syncthreads();
  Mom r = mom_load(lds);
  for (int w = 1; w < 4; ++w) r = mom_merge(r, mom_load(lds + 3 * w));
  __syncthreads();
  return r;
}

__device__ double block_sum(double v, double* lds, int tid) {
  for (int off = 1; off < 64; off <<= 1) v += __shfl_down(v, off);
  if ((tid & 63) == 0) lds[tid >> 6] = v;
  __syncthreads();
  const double r = ((lds[0] + lds[1]) + lds[2]) + lds[3];
  __syncthreads();
  return r;
}

__device__ double block_min(double v, double* lds, int tid) {
  for (int off = 1; off < 64; off <<= 1) v = nan_min(v, __shfl_down(v, off));
  if ((tid & 63) == 0) lds[tid >> 6] = v;
  __syncthreads();
  const double r = nan_min(nan_min(nan_min(lds[0], lds[1]), lds[2]), lds[3]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 1; off < 64; off <<= 1) v += __shfl_down(v, off);
  return v;   // lane 0's is the sum
}

__global__ void __launch_bounds__(256)
k_metrics_critic(double* slot, const float* loss, const float* q_chosen, const float* td, const float* disc, const float* q_new,
                 const int32_t* action, int64_t B, int A) {
  __shared__ double lds[12];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * MT_CHUNK;
  const int64_t row = row0 + tid;
  const bool valid = row < B;
  double* rec = slot + MT_SLOT_HDR + (int64_t)blockIdx.x * MT_REC;

  double t = 0.0, d = 0.0, qc = 0.0;
  if (valid) { t = (double)td[row]; d = (double)disc[row]; qc = (double)q_chosen[row]; }
  const double one = valid ? 1.0 : 0.0;
  const Mom m_td = block_mom(Mom{one, t, 0.0}, lds, tid);
  const Mom m_disc = block_mom(Mom{one, d, 0.0}, lds, tid);
  const Mom m_dev = block_mom(Mom{one, valid ? fabs(d - qc) : 0.0, 0.0}, lds, tid);
  const Mom m_diff = block_mom(Mom{one, d - t, 0.0}, lds, tid);
  const double s_qc = block_sum(qc, lds, tid);

  // the row's A values of q_new: lane-local sum, then the squares around the lane's mean, both in column order
  Mom lane{0.0, 0.0, 0.0};
  double qmin = INFINITY;
  if (valid) {
    const float* q = q_new + row * A;
    double s = 0.0;
    for (int a = 0; a < A; ++a) { const double x = (double)q[a]; s += x; qmin = nan_min(qmin, x); }
    const double mean = s / (double)A;
    double m2 = 0.0;
    for (int a = 0; a < A; ++a) { const double e = (double)q[a] - mean; m2 += e * e; }
    lane = Mom{(double)A, s, m2};
  }
  const Mom m_q = block_mom(lane, lds, tid);
  qmin = block_min(qmin, lds, tid);

  // columns: wavefront w takes columns w, w + 4, ...; a lane takes rows lane, lane + 64, lane + 128, lane + 192 of the chunk in that order
  const int wave = tid >> 6, ln = tid & 63;
  for (int a = wave; a < A; a += 4) {
    double x[4];
    double mx = -INFINITY, cnt = 0.0, sq = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t r = row0 + ln + 64 * k;
      x[k] = -INFINITY;
      if (r < B) {
        x[k] = (double)q_new[r * A + a];
        mx = fmax(mx, x[k]);                 // (a NaN is skipped here and reaches the sum through exp(NaN - mx))
        const int act = action[r];
        if (act == a) { cnt += 1.0; sq += x[k]; }
        if (a == 0 && (act < 0 || act >= A)) sq += NAN;     // an action outside the table: NaN, nothing out of range is read
      }
    }
    for (int off = 1; off < 64; off <<= 1) mx = fmax(mx, __shfl_xor(mx, off));
    double se = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (row0 + ln + 64 * k < B) se += exp(x[k] - mx);
    se = wave_sum(se);
    cnt = wave_sum(cnt);
    sq = wave_sum(sq);
    if (ln == 0) {
      double* c = rec + MT_R_COL + 4 * a;
      c[0] = mx; c[1] = se; c[2] = cnt; c[3] = sq;
    }
  }

  if (tid == 0) {
    mom_store(rec + MT_R_TD, m_td);
    mom_store(rec + MT_R_DISC, m_disc);
    mom_store(rec + MT_R_DEV, m_dev);
    mom_store(rec + MT_R_DIFF, m_diff);
    mom_store(rec + MT_R_QNEW, m_q);
    rec[MT_R_QCH] = s_qc;
    rec[MT_R_QMIN] = qmin;
    if (blockIdx.x == 0) slot[0] = (double)loss[0];
  }
}

__global__ void __launch_bounds__(256)
k_metrics_actor(double* slot, const float* loss, const float* adv, const float* probs, const int32_t* action, const float* hidden0, int64_t B,
                int A) {
  __shared__ double lds[12];
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * MT_CHUNK + tid;
  const bool valid = row < B;
  double* rec = slot + MT_SLOT_HDR + (int64_t)blockIdx.x * MT_REC;
  double ad = 0.0, logc = 0.0, ent = 0.0;
  if (valid) {
    ad = (double)adv[row];
    const float* p = probs + row * A;
    const int act = action[row];
    logc = (act >= 0 && act < A) ? log((double)p[act]) : (double)NAN;
    for (int a = 0; a < A; ++a) { const double x = (double)p[a]; ent += x * log(x); }     // 0 log 0 is NaN, as the definition gives
  }
  const Mom m_adv = block_mom(Mom{valid ? 1.0 : 0.0, ad, 0.0}, lds, tid);
  const double s_logc = block_sum(logc, lds, tid);
  const double s_ent = block_sum(ent, lds, tid);
  double hh = 0.0;
  if (blockIdx.x == 0) {
    const double h = (double)hidden0[tid];
    hh = block_sum(h * h, lds, tid);
  }
  if (tid == 0) {
    mom_store(rec + MT_R_ADV, m_adv);
    rec[MT_R_LOGC] = s_logc;
    rec[MT_R_ENT] = s_ent;
    if (blockIdx.x == 0) { slot[1] = (double)loss[0]; slot[2] = hh / 256.0; }
  }
}

__global__ void __launch_bounds__(256)
k_metrics_actor_after(double* slot, const float* p_old, const float* p_after, int64_t B, int A) {
  __shared__ double lds[12];
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * MT_CHUNK + tid;
  double kl = 0.0;
  if (row < B) {
    const float* p = p_old + row * A;
    const float* q = p_after + row * A;
    for (int a = 0; a < A; ++a) { const double x = (double)p[a]; kl += x * (log(x) - (double)q[a]); }
  }
  kl = block_sum(kl, lds, tid);
  if (tid == 0) slot[MT_SLOT_HDR + (int64_t)blockIdx.x * MT_REC + MT_R_KL] = kl;
}

struct GradArgs {
  const float* g[MT_TENSORS];
  int64_t n[MT_TENSORS];
};

// workgroup (part, tensor): elements [part L, (part + 1) L) of the tensor, L = ceil(n / 64) rounded up to whole quads.  A lane sums the quads
// lane, lane + 256, ... element by element; a whole quad of a 16-byte aligned tensor arrives in one load, which changes no addition.
__global__ void __launch_bounds__(256) k_metrics_grad_l1(double* part_out, const GradArgs a) {
  __shared__ double lds[12];
  const int tid = threadIdx.x;
  const int ti = blockIdx.y;
  const float* g = a.g[ti];
  const int64_t n = a.n[ti];
  const int64_t L = ((n + MT_GRAD_PARTS - 1) / MT_GRAD_PARTS + 3) & ~(int64_t)3;
  const int64_t lo = (int64_t)blockIdx.x * L;
  const int64_t hi = lo + L < n ? lo + L : n;
  const bool vec = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
  double acc = 0.0;
  for (int64_t e = lo + 4 * (int64_t)tid; e < hi; e += 4 * 256) {
    if (vec && e + 4 <= hi) {
      const float4 v = *reinterpret_cast<const float4*>(g + e);
      acc += fabs((double)v.x); acc += fabs((double)v.y); acc += fabs((double)v.z); acc += fabs((double)v.w);
    } else {
      for (int i = 0; i < 4; ++i)
        if (e + i < hi) acc += fabs((double)g[e + i]);
    }
  }
  acc = block_sum(acc, lds, tid);
  if (tid == 0) part_out[ti * MT_GRAD_PARTS + blockIdx.x] = acc;
}

// One workgroup.  Threads 0..5: one moment set each; 6: the plain sums and the minimum; 8..27: one gradient tensor each; all: the
// (slot, column) pairs of the critic's batch-axis log-softmax.
__global__ void __launch_bounds__(256) k_metrics_finalize(const double* blob, int nb, int64_t B, int A, double* out) {
  __shared__ double lds[12];
  __shared__ double grad[2 * MT_TENSORS];
  __shared__ double ev[2];
  const int tid = threadIdx.x;
  const int64_t C = (B + MT_CHUNK - 1) / MT_CHUNK;
  const int64_t stride = MT_SLOT_HDR + C * MT_REC;
  const double* slots = blob + MT_GRAD_DOUBLES;
  const double rows = (double)nb * (double)B;

  if (tid < 6) {
    const int off = tid == 0 ? MT_R_TD : tid == 1 ? MT_R_DISC : tid == 2 ? MT_R_DEV : tid == 3 ? MT_R_DIFF : tid == 4 ? MT_R_QNEW : MT_R_ADV;
    Mom all{0.0, 0.0, 0.0};
    for (int s = 0; s < nb; ++s) {
      const double* rec = slots + s * stride + MT_SLOT_HDR + off;
      Mom m{0.0, 0.0, 0.0};
      for (int64_t c = 0; c < C; ++c) m = mom_merge(m, mom_load(rec + c * MT_REC));
      all = mom_merge(all, m);
    }
    const double mean = all.s / all.n;
    const double sd = sqrt(all.m2 / (all.n - 1.0));      // unbiased; one element: 0 / 0 = NaN, as torch
    if (tid == 0) { out[1] = mean; out[2] = sd; }
    if (tid == 1) { out[8] = mean; out[9] = sd; ev[1] = all.m2 / all.n; }
    if (tid == 2) { out[10] = mean; out[11] = sd; }
    if (tid == 3) ev[0] = all.m2 / all.n;
    if (tid == 4) { out[4] = mean; out[6] = sd; }
    if (tid == 5) { out[20] = mean; out[21] = sd; }
  } else if (tid == 6) {
    double lc = 0.0, la = 0.0, hid = 0.0, qch = 0.0, logc = 0.0, ent = 0.0, kl = 0.0, qmin = INFINITY;
    for (int s = 0; s < nb; ++s) {
      const double* hdr = slots + s * stride;
      lc += hdr[0]; la += hdr[1]; hid += hdr[2];
      double s_qch = 0.0, s_logc = 0.0, s_ent = 0.0, s_kl = 0.0;
      for (int64_t c = 0; c < C; ++c) {
        const double* rec = hdr + MT_SLOT_HDR + c * MT_REC;
        s_qch += rec[MT_R_QCH]; s_logc += rec[MT_R_LOGC]; s_ent += rec[MT_R_ENT]; s_kl += rec[MT_R_KL];
        qmin = nan_min(qmin, rec[MT_R_QMIN]);
      }
      qch += s_qch; logc += s_logc; ent += s_ent; kl += s_kl;
    }
    out[0] = lc / (double)nb;
    out[3] = qch / rows;
    out[5] = qmin;
    out[19] = la / (double)nb;
    out[22] = logc / rows;
    out[23] = -ent / rows;
    out[24] = kl / ((double)B * (double)A);      // summed over the minibatches, averaged over (sample, action)
    out[25] = hid / (double)nb;
  } else if (tid >= 8 && tid < 8 + 2 * MT_TENSORS) {
    const double* p = blob + (tid - 8) * MT_GRAD_PARTS;
    double s = 0.0;
    for (int i = 0; i < MT_GRAD_PARTS; ++i) s += p[i];
    grad[tid - 8] = s;
  }

  // log-softmax over the batch axis: sum_b q[b,a_b] - sum_a (rows that chose a) * logsumexp_b q[b,a]
  double lp = 0.0;
  for (int q = tid; q < nb * A; q += 256) {
    const int s = q / A, a = q - s * A;
    const double* col = slots + s * stride + MT_SLOT_HDR + MT_R_COL + 4 * a;
    double mx = col[0], se = col[1], cnt = col[2], sq = col[3];
    for (int64_t c = 1; c < C; ++c) {
      const double* o = col + c * MT_REC;
      const double M = fmax(mx, o[0]);
      se = se * exp(mx - M) + o[1] * exp(o[0] - M);
      mx = M;
      cnt += o[2];
      sq += o[3];
    }
    lp += cnt == 0.0 ? sq : sq - cnt * (mx + log(se));
  }
  lp = block_sum(lp, lds, tid);      // (its barriers also publish grad[] and ev[])
  if (tid == 0) {
    out[12] = lp / rows;
    // explained_variance_score with population variances and its zero rules
    const double num = ev[0], den = ev[1];
    out[7] = den == 0.0 ? (num == 0.0 ? 1.0 : 0.0) : 1.0 - num / den;
  }
  if (tid >= 32 && tid < 44) {
    const int k = (tid - 32) / 6, l = (tid - 32) % 6;      // net, layer of metrics.LAYERS (fc2, l == 4, has no gradient)
    const int li = l < 4 ? l : 4;
    out[13 + 13 * k + l] = l == 4 ? 0.0 : (grad[k * MT_TENSORS + 2 * li] + grad[k * MT_TENSORS + 2 * li + 1]) / 2.0;
  }
}

bool mt_shape_ok(const std::string& who, int32_t nb, int64_t batch, int32_t A) {
  if (nb < 1 || nb > 65536) { ippm_set_error(who + ": n_minibatches must be in [1, 65536]"); return false; }
  if (batch < 2 || batch > ((int64_t)1 << 24)) { ippm_set_error(who + ": batch must be in [2, 2^24]"); return false; }
  if (A < 2 || A > MT_MAX_A) { ippm_set_error(who + ": n_actions must be in [2, 32]"); return false; }
  return true;
}

bool mt_slot_ok(const std::string& who, const void* acc, int32_t slot, int32_t nb, int64_t batch, int32_t A) {
  if (!acc) { ippm_set_error(who + ": null argument"); return false; }
  if (!mt_shape_ok(who, nb, batch, A)) return false;
  if (slot < 0 || slot >= nb) { ippm_set_error(who + ": slot must be in [0, n_minibatches)"); return false; }
  if (reinterpret_cast<uintptr_t>(acc) & 15) { ippm_set_error(who + ": the blob must be 16-byte aligned"); return false; }
  return true;
}

bool mt_aligned4(const std::string& who, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs) {
    if (!p) { ippm_set_error(who + ": null argument"); return false; }
    if (reinterpret_cast<uintptr_t>(p) & 3) { ippm_set_error(who + ": the arrays must be 4-byte aligned"); return false; }
  }
  return true;
}

inline int64_t mt_chunks(int64_t batch) { return (batch + MT_CHUNK - 1) / MT_CHUNK; }

inline double* mt_slot(void* acc, int32_t slot, int64_t batch) {
  return static_cast<double*>(acc) + MT_GRAD_DOUBLES + (int64_t)slot * (MT_SLOT_HDR + mt_chunks(batch) * MT_REC);
}

}  // namespace

extern "C" int ippm_metrics_bytes(int32_t n_minibatches, int64_t batch, int32_t n_actions, int64_t* bytes) {
  const std::string who = "ippm_metrics_bytes";
  if (!bytes) { ippm_set_error(who + ": null argument"); return -1; }
  if (!mt_shape_ok(who, n_minibatches, batch, n_actions)) return -1;
  *bytes = 8 * (MT_GRAD_DOUBLES + (int64_t)n_minibatches * (MT_SLOT_HDR + mt_chunks(batch) * MT_REC));
  return 0;
}

extern "C" int ippm_metrics_critic(void* acc, int32_t slot, int32_t n_minibatches, const float* loss, const float* q_chosen, const float* td,
                                   const float* disc, const float* q_new, const int32_t* action, int64_t batch, int32_t n_actions,
                                   void* stream) {
  const std::string who = "ippm_metrics_critic";
  if (!mt_slot_ok(who, acc, slot, n_minibatches, batch, n_actions)) return -1;
  if (!mt_aligned4(who, {loss, q_chosen, td, disc, q_new, action})) return -1;
  hipLaunchKernelGGL(k_metrics_critic, dim3((unsigned)mt_chunks(batch)), dim3(256), 0, S_(stream), mt_slot(acc, slot, batch), loss, q_chosen,
                     td, disc, q_new, action, batch, (int)n_actions);
  IPPM_LAUNCH_CHECK("ippm_metrics_critic");
  return 0;
}

extern "C" int ippm_metrics_actor(void* acc, int32_t slot, int32_t n_minibatches, const float* loss, const float* adv, const float* probs,
                                  const int32_t* action, const float* hidden0, int64_t batch, int32_t n_actions, void* stream) {
  const std::string who = "ippm_metrics_actor";
  if (!mt_slot_ok(who, acc, slot, n_minibatches, batch, n_actions)) return -1;
  if (!mt_aligned4(who, {loss, adv, probs, action, hidden0})) return -1;
  hipLaunchKernelGGL(k_metrics_actor, dim3((unsigned)mt_chunks(batch)), dim3(256), 0, S_(stream), mt_slot(acc, slot, batch), loss, adv, probs,
                     action, hidden0, batch, (int)n_actions);
  IPPM_LAUNCH_CHECK("ippm_metrics_actor");
  return 0;
}

extern "C" int ippm_metrics_actor_after(void* acc, int32_t slot, int32_t n_minibatches, const float* probs_old, const float* probs_after,
                                        int64_t batch, int32_t n_actions, void* stream) {
  const std::string who = "ippm_metrics_actor_after";
  if (!mt_slot_ok(who, acc, slot, n_minibatches, batch, n_actions)) return -1;
  if (!mt_aligned4(who, {probs_old, probs_after})) return -1;
  hipLaunchKernelGGL(k_metrics_actor_after, dim3((unsigned)mt_chunks(batch)), dim3(256), 0, S_(stream), mt_slot(acc, slot, batch), probs_old,
                     probs_after, batch, (int)n_actions);
  IPPM_LAUNCH_CHECK("ippm_metrics_actor_after");
  return 0;
}

extern "C" int ippm_metrics_grad_l1(void* acc, int32_t net, float* const* grads, const int64_t* numel, int32_t n_tensors, void* stream) {
  const std::string who = "ippm_metrics_grad_l1";
  if (!acc || !grads || !numel) { ippm_set_error(who + ": null argument"); return -1; }
  if (net != 0 && net != 1) { ippm_set_error(who + ": net must be 0 (critic) or 1 (actor)"); return -1; }
  if (n_tensors != MT_TENSORS) { ippm_set_error(who + ": n_tensors must be 10 (the tensors of a network, in ippm_adam_step's order)"); return -1; }
  if (reinterpret_cast<uintptr_t>(acc) & 15) { ippm_set_error(who + ": the blob must be 16-byte aligned"); return -1; }
  GradArgs a;
  for (int i = 0; i < MT_TENSORS; ++i) {
    if (numel[i] < 1 || numel[i] > ((int64_t)1 << 36)) { ippm_set_error(who + ": every numel must be in [1, 2^36]"); return -1; }
    if (!mt_aligned4(who, {grads[i]})) return -1;
    a.g[i] = grads[i];
    a.n[i] = numel[i];
  }
  hipLaunchKernelGGL(k_metrics_grad_l1, dim3(MT_GRAD_PARTS, MT_TENSORS), dim3(256), 0, S_(stream),
                     static_cast<double*>(acc) + net * MT_TENSORS * MT_GRAD_PARTS, a);
  IPPM_LAUNCH_CHECK("ippm_metrics_grad_l1");
  return 0;
}

extern "C" int ippm_metrics_finalize(const void* acc, int32_t n_minibatches, int64_t batch, int32_t n_actions, double* out, void* stream) {
  const std::string who = "ippm_metrics_finalize";
  if (!acc || !out) { ippm_set_error(who + ": null argument"); return -1; }
  if (!mt_shape_ok(who, n_minibatches, batch, n_actions)) return -1;
  if (reinterpret_cast<uintptr_t>(acc) & 15) { ippm_set_error(who + ": the blob must be 16-byte aligned"); return -1; }
  if (reinterpret_cast<uintptr_t>(out) & 7) { ippm_set_error(who + ": out must be 8-byte aligned"); return -1; }
  hipLaunchKernelGGL(k_metrics_finalize, dim3(1), dim3(256), 0, S_(stream), static_cast<const double*>(acc), (int)n_minibatches, batch,
                     (int)n_actions, out);
  IPPM_LAUNCH_CHECK("ippm_metrics_finalize");
  return 0;
}
