// Native Adam (actor/learner.py:32, critic/learner.py:48: torch.optim.Adam(parameters, lr) with its defaults -- no weight decay, no amsgrad):
// ONE launch steps up to 16 float32 tensors, optionally clears their gradients and, for the ten tensors of a network, rewrites every byte of
// its bf16 inference pack (ippm_bf16_net.h's NetPack) from the new parameters.
//
// Arithmetic contract ("Native Adam"): the scalars of a step are formed in double from the powers kept in the state
// blob, b1p <- b1p * beta1, b2p <- b2p * beta2 (one multiplication each, no pow), step = float(lr / (1 - b1p)), rs = float(sqrt(1 - b2p)),
// w1 = float(1 - beta1), w2 = float(1 - beta2), B2 = float(beta2), E = float(eps); per element, every float32 operation is rounded on its own,
// in this order, nothing contracted into an FMA:
//     m <- m + w1 (g - m);   v <- B2 v + w2 (g g);   den = sqrtf(v) / rs + E;   p <- p - step (m / den)
//
// Work split: every tensor is cut into chunks of consecutive elements, one workgroup per chunk, the tensors' first workgroups travelling
// with the pointers in the kernel's by-value argument (no device-side table).  Without a pack a chunk is 4096 elements.  With a pack a
// chunk is what one workgroup can turn into whole pack rows: one output channel of a convolution (PyTorch's [O][C][kh][kw] row is read
// coalesced in parameter order, the new bf16 values are transposed to the pack's [tap][C] through LDS and leave in 16-byte stores), four
// rows of fc1 / fc3 (fc3's rows beyond n_actions are written as zeros), or a bias vector (float32, stored by the lane that stepped it).
//
// The counters (step number and the two powers) advance inside the same launch without any workgroup waiting on another: see k_adam_step.
#include <cmath>

#include "ippm_bf16_net.h"

namespace {

constexpr int AD_MAX = 16;              // tensors per launch
constexpr int AD_CHUNK = 4096;          // elements per workgroup of a tensor that feeds no pack row
constexpr int AD_LINEAR_CHUNK = 1024;   // ... and of fc1 / fc3 with a pack: four rows of 256
constexpr int AD_COUNTER_BYTES = 64;    // int64 t, double b1p, double b2p, uint32 ticket, padding (the header documents the layout)
constexpr int AD_TAP_LD = 256 + 8;      // LDS elements from one tap of a 4x4 row to the next: 16 bytes of padding keep 16 taps off one bank
constexpr int AD_LDS = 16 * AD_TAP_LD;

enum { AD_PLAIN = 0, AD_CONV1 = 1, AD_CONV4 = 2, AD_LINEAR = 3, AD_BIAS = 4 };

struct AdamTensor {
  float* p;
  float* g;
  int64_t n;        // elements
  int64_t m_off;    // float offset of m in the state blob; v follows at m_off + ((n + 3) & ~3)
  int64_t dst;      // byte offset of this tensor's part of the pack
  int32_t wg0;      // first workgroup (the prefix sum of the tensors before)
  int32_t chunk;    // elements per workgroup
  int32_t kind;
  int32_t dst_n;    // AD_BIAS: floats of the pack's block (fc3's bias is zero-padded to 32)
};

struct AdamArgs {
  AdamTensor t[AD_MAX];
  int32_t n_tensors;
  int32_t planes;
};

__host__ __device__ inline int64_t ad_span(int64_t n) { return (n + 3) & ~(int64_t)3; }

__global__ void __launch_bounds__(256) k_adam_init(uint32_t* state, int64_t words) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= words) return;
  // words 0-1: t = 0; 2-3 and 4-5: the doubles 1.0; 6: the ticket; everything else, the moments included, 0
  state[i] = (i == 3 || i == 5) ? 0x3FF00000u : 0u;
}

// The counters.  Every thread reads t, b1p and b2p before anything else.  A workgroup takes its ticket (an atomicAdd on a 32-bit word,
// device scope) after its last store and behind a barrier; the workgroup that draws the last ticket of the launch writes t + 1, the new powers
// and ticket 0.  No workgroup waits on another.  No workgroup can read a counter after it was advanced: the advance happens only after EVERY
// workgroup of the launch has taken its ticket; a workgroup's ticket is taken behind __syncthreads(), in front of which every wavefront has
// waited for all its outstanding memory operations (the barrier's workgroup-scope release), so the counter values had arrived in registers
// before its ticket was issued; and the next launch on the stream starts after this one has ended.  Nothing else crosses workgroups inside the
// launch (parameters, moments, gradients and pack bytes have one owner each and become visible at the end of the kernel), which is why
// there is no device-scope fence in front of the ticket: one per workgroup (presumably the cache write-back such a release implies) cost more
// than the step itself (118 us with the fence against 32 us without, a network's 2.2 M parameters with its pack: profiles/r15/).
__global__ void __launch_bounds__(256)
k_adam_step(const AdamArgs a, char* state, char* packed, double lr, double beta1, double beta2, double eps,
            int zero_grad, int n_actions) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) uint16_t lds[AD_LDS];
  const int64_t t_old = *reinterpret_cast<volatile int64_t*>(state);
  const double b1p = *reinterpret_cast<volatile double*>(state + 8) * beta1;
  const double b2p = *reinterpret_cast<volatile double*>(state + 16) * beta2;
  const float step = (float)(lr / (1.0 - b1p));
  const float rs = (float)sqrt(1.0 - b2p);
  const float w1 = (float)(1.0 - beta1), w2 = (float)(1.0 - beta2), B2 = (float)beta2, E = (float)eps;

  const int tid = threadIdx.x;
  const int wg = (int)blockIdx.x;
  int ti = 0;
  for (int i = 1; i < a.n_tensors; ++i)
    if (wg >= a.t[i].wg0) ti = i;
  const AdamTensor T = a.t[ti];
  const int kind = T.kind;
  const int64_t e0 = (int64_t)(wg - T.wg0) * T.chunk;
  float* m = reinterpret_cast<float*>(state) + T.m_off;
  float* v = m + ad_span(T.n);
  float* bias_out = kind == AD_BIAS ? reinterpret_cast<float*>(packed + T.dst) : nullptr;

  for (int j = tid; j < T.chunk; j += 256) {
    const int64_t e = e0 + j;
    uint16_t h = 0;          // (what a pack element beyond the tensor holds: fc3's rows past n_actions)
    if (e < T.n) {
      const float g = T.g[e];
      float mm = m[e], vv = v[e], pp = T.p[e];
      // (plain operators under the pragma above: the __f*_rn wrappers are inline functions of a header compiled with contraction
      //  allowed, and their operations keep that licence when they are inlined here)
      const float dm = g - mm;
      const float wm = w1 * dm;
      mm = mm + wm;
      const float gg = g * g;
      const float wv = w2 * gg;
      const float bv = B2 * vv;
      vv = bv + wv;
      const float sq = sqrtf(vv);
      const float qd = sq / rs;
      const float den = qd + E;
      const float md = mm / den;
      const float sm = step * md;
      pp = pp - sm;
      m[e] = mm;
      v[e] = vv;
      T.p[e] = pp;
      if (zero_grad) T.g[e] = 0.0f;
      if (kind == AD_BIAS) bias_out[e] = pp;
      h = ai_bf16(pp);
    } else if (kind == AD_BIAS && e < T.dst_n) {
      bias_out[e] = 0.0f;
    }
    // the pack's place of element j of this chunk
    if (kind == AD_CONV4) lds[(j & 15) * AD_TAP_LD + (j >> 4)] = h;                                  // [c][tap] -> [tap][c]
    else if (kind == AD_CONV1) { const int c = j / 25, tap = j - c * 25; lds[tap * a.planes + c] = h; }
    else if (kind == AD_LINEAR) lds[j] = h;
  }
  if (kind == AD_CONV1 || kind == AD_CONV4 || kind == AD_LINEAR) {
    // conv1's K columns from 25 * planes up to the padded K are zeros
    const int k_real = kind == AD_CONV1 ? T.chunk : 0;
    const int k_pad = kind == AD_CONV1 ? (T.chunk + 63) / 64 * 64 : 0;
    for (int j = k_real + tid; j < k_pad; j += 256) lds[j] = 0;
    __syncthreads();
    const int out_n = kind == AD_CONV1 ? k_pad : T.chunk;          // bf16 elements this workgroup owns in the pack
    uint4* dst = reinterpret_cast<uint4*>(packed + T.dst + (int64_t)(wg - T.wg0) * out_n * 2);
    for (int q = tid; q < out_n / 8; q += 256) {
      const int src = kind == AD_CONV4 ? (q >> 5) * AD_TAP_LD + (q & 31) * 8 : q * 8;
      dst[q] = *reinterpret_cast<const uint4*>(&lds[src]);
    }
  }

  __syncthreads();
  if (tid == 0) {
    unsigned* ticket = reinterpret_cast<unsigned*>(state + 24);
    if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
      *reinterpret_cast<volatile int64_t*>(state) = t_old + 1;
      *reinterpret_cast<volatile double*>(state + 8) = b1p;
      *reinterpret_cast<volatile double*>(state + 16) = b2p;
      atomicExch(ticket, 0u);
    }
  }
}

bool ad_tensors_ok(const char* who, const int64_t* numel, int32_t n_tensors) {
  if (!numel) { ippm_set_error(std::string(who) + ": null argument"); return false; }
  if (n_tensors < 1 || n_tensors > AD_MAX) { ippm_set_error(std::string(who) + ": n_tensors must be in [1, 16]"); return false; }
  for (int i = 0; i < n_tensors; ++i)
    if (numel[i] < 1 || numel[i] > ((int64_t)1 << 36)) { ippm_set_error(std::string(who) + ": every numel must be in [1, 2^36]"); return false; }
  return true;
}

int64_t ad_state_bytes(const int64_t* numel, int32_t n_tensors) {
  int64_t floats = 0;
  for (int i = 0; i < n_tensors; ++i) floats += 2 * ad_span(numel[i]);
  return AD_COUNTER_BYTES + floats * 4;
}

// the ten tensors of a network with `planes` input planes, in native_net._LAYERS order, and where each lands in NetPack<PLANES>
template <int PLANES>
bool ad_plan_pack(AdamArgs& a, const int64_t* numel, int32_t A) {
  using P = NetPack<PLANES>;
  const int64_t want[10] = {256 * P::K1_REAL, 256, 256 * 4096, 256, 256 * 4096, 256, 256 * 256, 256, (int64_t)A * 256, A};
  for (int i = 0; i < 10; ++i)
    if (numel[i] != want[i]) return false;
  const int64_t wdst[5] = {P::W1 * 2, P::W2 * 2, P::W3 * 2, P::W4 * 2, P::W5 * 2};
  const int32_t wkind[5] = {AD_CONV1, AD_CONV4, AD_CONV4, AD_LINEAR, AD_LINEAR};
  const int32_t wchunk[5] = {P::K1_REAL, 4096, 4096, AD_LINEAR_CHUNK, AD_LINEAR_CHUNK};
  const int32_t wgroups[5] = {256, 256, 256, 256 * 256 / AD_LINEAR_CHUNK, AI_NPAD * 256 / AD_LINEAR_CHUNK};
  int32_t wg = 0;
  for (int l = 0; l < 5; ++l) {
    AdamTensor& w = a.t[2 * l];
    w.dst = wdst[l]; w.kind = wkind[l]; w.chunk = wchunk[l]; w.wg0 = wg; w.dst_n = 0;
    wg += wgroups[l];
    AdamTensor& b = a.t[2 * l + 1];
    b.dst = P::BIAS_BYTES + (int64_t)l * 256 * 4; b.kind = AD_BIAS; b.chunk = 256; b.wg0 = wg; b.dst_n = l < 4 ? 256 : AI_NPAD;
    wg += 1;
  }
  a.planes = PLANES;
  return true;
}

}  // namespace

extern "C" int ippm_adam_state_bytes(const int64_t* numel, int32_t n_tensors, int64_t* bytes) {
  const char* who = "ippm_adam_state_bytes";
  if (!bytes) { ippm_set_error(std::string(who) + ": null argument"); return -1; }
  if (!ad_tensors_ok(who, numel, n_tensors)) return -1;
  *bytes = ad_state_bytes(numel, n_tensors);
  return 0;
}

extern "C" int ippm_adam_init(void* state, const int64_t* numel, int32_t n_tensors, void* stream) {
  const char* who = "ippm_adam_init";
  if (!state) { ippm_set_error(std::string(who) + ": null argument"); return -1; }
  if (!ad_tensors_ok(who, numel, n_tensors)) return -1;
  if (reinterpret_cast<uintptr_t>(state) & 15) { ippm_set_error(std::string(who) + ": state must be 16-byte aligned"); return -1; }
  const int64_t words = ad_state_bytes(numel, n_tensors) / 4;
  hipLaunchKernelGGL(k_adam_init, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, S_(stream), static_cast<uint32_t*>(state), words);
  IPPM_LAUNCH_CHECK(who);
  return 0;
}

extern "C" int ippm_adam_step(void* state, float* const* params, float* const* grads, const int64_t* numel, int32_t n_tensors, double lr,
                              double beta1, double beta2, double eps, int32_t flags, int32_t pack_planes, int32_t n_actions, void* packed,
                              void* stream) {
  const std::string who = "ippm_adam_step";
  if (!state || !params || !grads) { ippm_set_error(who + ": null argument"); return -1; }
  if (!ad_tensors_ok("ippm_adam_step", numel, n_tensors)) return -1;
  for (int i = 0; i < n_tensors; ++i)
    if (!params[i] || !grads[i]) { ippm_set_error(who + ": null argument (a parameter or gradient pointer)"); return -1; }
  if ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(packed)) & 15) {
    ippm_set_error(who + ": state and packed must be 16-byte aligned");
    return -1;
  }
  if (!(std::isfinite(lr) && lr >= 0.0)) { ippm_set_error(who + ": lr must be finite and not negative"); return -1; }
  if (!(std::isfinite(eps) && eps >= 0.0)) { ippm_set_error(who + ": eps must be finite and not negative"); return -1; }
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) { ippm_set_error(who + ": beta1 and beta2 must be in [0, 1)"); return -1; }
  if (flags & ~IPPM_ADAM_ZERO_GRAD) { ippm_set_error(who + ": unknown flags"); return -1; }
  if (pack_planes != 0 && pack_planes != IPPM_ACTOR_PLANES && pack_planes != IPPM_CRITIC_PLANES) {
    ippm_set_error(who + ": pack_planes must be 0, 7 or 12");
    return -1;
  }
  if ((packed != nullptr) != (pack_planes != 0)) { ippm_set_error(who + ": packed and pack_planes (7 or 12) go together"); return -1; }

  AdamArgs a = {};
  a.n_tensors = n_tensors;
  int64_t m_off = AD_COUNTER_BYTES / 4;
  for (int i = 0; i < n_tensors; ++i) {
    a.t[i].p = params[i];
    a.t[i].g = grads[i];
    a.t[i].n = numel[i];
    a.t[i].m_off = m_off;
    m_off += 2 * ad_span(numel[i]);
  }
  int64_t groups = 0;
  if (packed) {
    if (n_tensors != 10) { ippm_set_error(who + ": a pack needs the ten tensors of a network (n_tensors = 10)"); return -1; }
    if (!ai_actions_ok("ippm_adam_step", n_actions)) return -1;
    const bool ok = pack_planes == IPPM_ACTOR_PLANES ? ad_plan_pack<IPPM_ACTOR_PLANES>(a, numel, n_actions)
                                                     : ad_plan_pack<IPPM_CRITIC_PLANES>(a, numel, n_actions);
    if (!ok) { ippm_set_error(who + ": the sizes (numel) are not those of the network with these pack_planes and n_actions"); return -1; }
    groups = a.t[9].wg0 + 1;
  } else {
    for (int i = 0; i < n_tensors; ++i) {
      a.t[i].kind = AD_PLAIN;
      a.t[i].chunk = AD_CHUNK;
      a.t[i].wg0 = (int32_t)groups;
      groups += (numel[i] + AD_CHUNK - 1) / AD_CHUNK;      // (at most 16 * 2^24: ad_tensors_ok bounds every numel)
    }
  }
  hipLaunchKernelGGL(k_adam_step, dim3((unsigned)groups), dim3(256), 0, S_(stream), a, static_cast<char*>(state), static_cast<char*>(packed),
                     lr, beta1, beta2, eps, (int)(flags & IPPM_ADAM_ZERO_GRAD), (int)n_actions);
  IPPM_LAUNCH_CHECK("ippm_adam_step");
  return 0;
}
