// The learners' conv1 on the bf16 matrix cores, for the COMA update (actor/network.py:19-28, critic/network.py): the stride-1, unpadded
// 5x5 convolution from PLANES (7: actor, 12: critic) input planes of an 11x11 map to 256 channels of a 7x7 map -- forward (optionally with
// bias + ReLU at the store) and weight gradient -- over channels-last float32 tensors.  No input gradient: conv1's input is data.
// Numerical contract (as csrc/conv4x4_train.hip): every operand (x, w, gy) is rounded to bf16 (nearest even) on its
// way into LDS, products accumulate in float32 on mfma_f32_16x16x32_bf16, outputs are float32 and are not rounded again.  No float
// atomics; every output element has one owner and a fixed summation order.
//
// K = (ty, tx, c) -- tap-major, channel-minor -- is 25 * PLANES, zero-padded to a multiple of 64 (175 -> 192, 300 -> 320) as NetPack does
// for inference; the 5 taps of a kernel row and their channels are 5 * PLANES contiguous floats of the input and the next kernel row
// starts 11 * PLANES floats further on, so no im2col buffer exists.  The padded k are ZERO in LDS and are never read from memory.
//
// Forward: the implicit GEMM of k_actor_layer<true, PLANES> (ippm_bf16_net.h, on the tile of ippm_bf16_tile.h) with a float32 store.
// Weight gradient: gw[o][k] = sum over r = (b,oy,ox) of gy[r][o] * x[r + offset(k)].  The output is tiny (256 x K) and gy is the big
// operand (1 KiB per row), so a workgroup owns (chunk of IPPM_CONV5X5_WGRAD_CHUNK samples, 64 output channels, ALL of K): gy is read once,
// the small input four times.  Both tiles go into LDS transposed ([o][r], [k][r]); a wavefront owns 64 o x K/4 k.  The float32 partial
// sums of a chunk go to the scratch [chunk][k][o]; k_partial_sum<C5SumMap> adds them in chunk order and writes PyTorch's [256,PLANES,5,5].
#include "ippm_bf16_net.h"

namespace {

constexpr int C5_OUT = 256;                                 // output channels
constexpr int C5_OP = 49, C5_IP = 121;                      // output / input positions per sample
constexpr int C5_WG_O = 64;                                 // output channels per workgroup of the weight gradient

template <int PLANES>
struct C5 {
  static constexpr int K_REAL = NetPack<PLANES>::K1_REAL, K = NetPack<PLANES>::K1;
  static constexpr int ROW = 5 * PLANES, STRIDE = 11 * PLANES;
  static constexpr int64_t PACK_BYTES = (int64_t)C5_OUT * K * 2;       // bf16 [o][k] (a multiple of 16)
  static constexpr int64_t PARTIAL = (int64_t)C5_OUT * K;             // floats of one chunk's partial sums [k][o]
};

// offset, within a sample, of element k of an output position's patch relative to the position's first input element
template <int PLANES>
__device__ __forceinline__ int c5_koff(int k) {
  const int ty = k / C5<PLANES>::ROW;
  return ty * C5<PLANES>::STRIDE + (k - ty * C5<PLANES>::ROW);
}

// w float32 [256,PLANES,5,5] -> bf16 [o][k], the padded k zero
template <int PLANES>
__global__ void __launch_bounds__(256) k_conv5x5_pack(const float* __restrict__ w, uint16_t* __restrict__ packed) {
  using G = C5<PLANES>;
  const int i = blockIdx.x * 256 + threadIdx.x;             // < 256 * K (K is a multiple of 64: the grid is exact)
  const int o = i / G::K, k = i - o * G::K;
  float v = 0.f;
  if (k < G::K_REAL) { const int tap = k / PLANES, c = k - tap * PLANES; v = w[(o * PLANES + c) * 25 + tap]; }
  packed[i] = ai_bf16(v);
}

// ---- forward --------------------------------------------------------------------------------------------------------------------------
// y[m][n] = sum_k x[patch(m)][k] * W[n][k], m = (sample, oy, ox) of M rows; bias non-null: y = relu(y + bias[n]) with the arithmetic of
// k_bias_relu (learn.hip), NaN let through (ippm_relu).
// The K loop and the store are written out here: on lt_k_loop and lt_for_outputs the 7-plane forward measured 1.2 % slower
// (profiles/r20/README.md); the instruction stream of this form is the one measured before the tile header existed.
template <int PLANES>
__global__ void __launch_bounds__(256)
k_conv5x5(const float* __restrict__ in, const uint16_t* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out, int64_t M) {
  using G = C5<PLANES>;
  __shared__ __attribute__((aligned(16))) uint16_t As[LT_M * LT_LD];
  __shared__ __attribute__((aligned(16))) uint16_t Ws[LT_N * LT_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * LT_M;
  const int n0 = blockIdx.y * LT_N;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;

  // staging: thread -> chunk column (8 k) and 4 rows, 32 apart
  const int sc = tid & 7, sr = tid >> 3;
  int64_t a_base[4];
  bool a_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + sr + 32 * i;
    a_ok[i] = m < M;
    const int64_t b = a_ok[i] ? m / C5_OP : 0;
    const int p = a_ok[i] ? (int)(m - b * C5_OP) : 0;
    const int oy = p / 7, ox = p - oy * 7;
    a_base[i] = b * (C5_IP * PLANES) + (oy * 11 + ox) * PLANES;
  }
  const uint16_t* wrow = w + (int64_t)(n0 + sr) * G::K + sc * 8;

  u32x4 a_reg[4], w_reg[4];
  auto load = [&](int k0) __attribute__((always_inline)) {
    const int k = k0 + sc * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) w_reg[i] = *reinterpret_cast<const u32x4*>(wrow + 32 * i * G::K + k0);
    // every load is unconditional (a row or a k that does not exist reads the row's / the tensor's first element and is zeroed
    // afterwards), so that the 32 of them are in flight together
    int koff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) koff[j] = k + j < G::K_REAL ? c5_koff<PLANES>(k + j) : 0;
    float v[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = in[a_base[i] + koff[j]];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = (a_ok[i] && k + j < G::K_REAL) ? v[i][j] : 0.f;
      a_reg[i] = lt_cvt8(v[i]);
    }
  };
  auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<u32x4*>(&As[(sr + 32 * i) * LT_LD + sc * 8]) = a_reg[i];
      *reinterpret_cast<u32x4*>(&Ws[(sr + 32 * i) * LT_LD + sc * 8]) = w_reg[i];
    }
  };

  floatx4 acc[4][4];   // [n tile][m tile]
  lt_zero(acc);

  const int fr = lane & 15, fk = (lane >> 4) * 8;
  load(0);
#pragma unroll 1
  for (int k0 = 0; k0 < G::K; k0 += LT_K) {
    __syncthreads();          // the previous step's fragment reads are done
    stage();
    __syncthreads();
    if (k0 + LT_K < G::K) load(k0 + LT_K);   // (uniform over the workgroup)
    lt_mma_step(As, Ws, wm, wn, fr, fk, acc);
  }

  // D[n][m]: lane holds m = lane & 15 and n = (lane >> 4) * 4 + reg
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int64_t m = m0 + wm + mt * 16 + fr;
    if (m >= M) continue;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int n = n0 + wn + nt * 16 + (lane >> 4) * 4;
      float4 v = float4{acc[nt][mt][0], acc[nt][mt][1], acc[nt][mt][2], acc[nt][mt][3]};
      if (bias) {
        const float4 bv = *reinterpret_cast<const float4*>(bias + n);
        v.x = ippm_relu(v.x + bv.x); v.y = ippm_relu(v.y + bv.y); v.z = ippm_relu(v.z + bv.z); v.w = ippm_relu(v.w + bv.w);
      }
      *reinterpret_cast<float4*>(out + m * C5_OUT + n) = v;
    }
  }
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------------------
// blockIdx.x = chunk * 4 + (quarter of the output channels).  The K of this GEMM is r = (sample of the chunk, oy, ox) in steps of 64.
//   Xs [k][r]: thread -> k = (tid & 31) + 32 * i (lanes next to each other read floats next to each other) and the 8 consecutive r
//              (tid >> 5) * 8 ..; after the rounding the 8 r of a k are one 16-byte LDS store.
//   Gs [o][r]: thread -> 4 channels (tid & 15) * 4 .. (one float4 per row) of the 4 consecutive r (tid >> 4) * 4 ..; 8-byte LDS stores.
// A wavefront owns the 64 o of the workgroup and the K/4 k from wave * K/4 on: 4 x NT accumulator tiles (NT = 3 / 5).
template <int PLANES>
__global__ void __launch_bounds__(256)
k_conv5x5_wgrad(const float* __restrict__ gy, const float* __restrict__ x, float* __restrict__ partial, int64_t B) {
  using G = C5<PLANES>;
  constexpr int NI = G::K / 32;                             // k per thread of the staging
  constexpr int NT = G::K / 64;                             // 16-wide k tiles per wavefront
  __shared__ __attribute__((aligned(16))) uint16_t Xs[G::K * LT_LD];      // [k][r]
  __shared__ __attribute__((aligned(16))) uint16_t Gs[C5_WG_O * LT_LD];   // [o][r]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t chunk = blockIdx.x >> 2;
  const int o0 = (blockIdx.x & 3) * C5_WG_O;
  const int64_t b0 = chunk * IPPM_CONV5X5_WGRAD_CHUNK;
  const int ns = B - b0 < IPPM_CONV5X5_WGRAD_CHUNK ? (int)(B - b0) : IPPM_CONV5X5_WGRAD_CHUNK;
  const int R = ns * C5_OP;                                 // rows of this chunk
  const float* gy0 = gy + b0 * C5_OP * C5_OUT + o0;
  const float* x0 = x + b0 * (C5_IP * PLANES);

  const int xk = tid & 31, xrg = tid >> 5;                  // x: k = xk + 32 i, rows xrg*8 .. xrg*8+7 of the step
  const int gc = (tid & 15) * 4, grq = tid >> 4;            // gy: channels gc .. gc+3, rows grq*4 .. grq*4+3 of the step
  int koff[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) koff[i] = xk + 32 * i < G::K_REAL ? c5_koff<PLANES>(xk + 32 * i) : -1;

  u32x4 xr[NI];
  float4 gr[4];
  int g_ok = 0;                                             // how many of gr's rows exist
  auto load = [&](int s) __attribute__((always_inline)) {
    const int k0 = s * LT_K;
    {
      const int r0 = k0 + grq * 4;      // (a row past the chunk reads the chunk's first row and is zeroed at the rounding)
#pragma unroll
      for (int j = 0; j < 4; ++j) gr[j] = *reinterpret_cast<const float4*>(gy0 + (int64_t)(r0 + j < R ? r0 + j : 0) * C5_OUT + gc);
      g_ok = r0 < R ? (R - r0 < 4 ? R - r0 : 4) : 0;
    }
    {
      const int r0 = k0 + xrg * 8;
      int b = r0 / C5_OP, p = r0 - b * C5_OP, oy = p / 7, ox = p - oy * 7;
      // every load is unconditional (a row past the chunk or a padded k reads an element of the chunk's first sample and is zeroed
      // afterwards), so that the loads are in flight together
      int base[8];
      bool ok[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ok[j] = r0 + j < R;
        base[j] = ok[j] ? b * (C5_IP * PLANES) + (oy * 11 + ox) * PLANES : 0;
        if (++ox == 7) {
          ox = 0;
          if (++oy == 7) { oy = 0; ++b; }
        }
      }
      float v[NI][8];
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] = x0[base[j] + (koff[i] >= 0 ? koff[i] : 0)];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] = (koff[i] >= 0 && ok[j]) ? v[i][j] : 0.f;
        xr[i] = lt_cvt8(v[i]);
      }
    }
  };
  auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NI; ++i) *reinterpret_cast<u32x4*>(&Xs[(xk + 32 * i) * LT_LD + xrg * 8]) = xr[i];
    const float* gf = reinterpret_cast<const float*>(gr);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float h[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) h[j] = j < g_ok ? gf[j * 4 + q] : 0.f;
      *reinterpret_cast<uint2*>(&Gs[(gc + q) * LT_LD + grq * 4]) = make_uint2(lt_cvt2(h[0], h[1]), lt_cvt2(h[2], h[3]));
    }
  };

  floatx4 acc[4][NT];   // [o tile][k tile]
  lt_zero(acc);
  const int fr = lane & 15, fk = (lane >> 4) * 8;
  const int wk = wave * (NT * 16);                          // first k of this wavefront
  lt_k_loop<LT_GUARDED, LT_ROLLED>((R + LT_K - 1) / LT_K, load, stage, [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int kk = 0; kk < LT_K; kk += 32) {
      bf16x8 gf[4], xf[NT];
#pragma unroll
      for (int t = 0; t < 4; ++t) gf[t] = *reinterpret_cast<const bf16x8*>(&Gs[(t * 16 + fr) * LT_LD + kk + fk]);
#pragma unroll
      for (int t = 0; t < NT; ++t) xf[t] = *reinterpret_cast<const bf16x8*>(&Xs[(wk + t * 16 + fr) * LT_LD + kk + fk]);
#pragma unroll
      for (int ot = 0; ot < 4; ++ot)
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) acc[ot][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf[ot], xf[kt], acc[ot][kt], 0, 0, 0);
    }
  });

  // m is k, n is o; partial [chunk][k][o]
  float* pt = partial + chunk * G::PARTIAL;
  auto row = [&](int kl) __attribute__((always_inline)) { return pt + (wk + kl) * C5_OUT; };
  lt_for_outputs(acc, row, [&](float* prow, int ol, const float4& v) __attribute__((always_inline)) {
    *reinterpret_cast<float4*>(prow + (o0 + ol)) = v;
  });
}

// gw[o][c][tap] from element i = (k, o) of the partials [chunk][k][o], the real k only: the reads are coalesced over o
template <int PLANES>
struct C5SumMap {
  static constexpr int64_t STRIDE = C5<PLANES>::PARTIAL;
  static __device__ int out(int i) {
    const int o = i & 255, k = i >> 8, tap = k / PLANES, c = k - tap * PLANES;
    return (o * PLANES + c) * 25 + tap;
  }
};

// ---- host side -----------------------------------------------------------------------------------------------------------------------
bool c5_shape_ok(const char* who, int64_t batch, int32_t planes) {
  if (!lt_batch_ok(who, batch)) return false;
  if (planes != 7 && planes != 12) { ippm_set_error(std::string(who) + ": planes must be 7 or 12"); return false; }
  return true;
}

// the two passes: two tensors in, one out, the scratch; optional: bias, the one pointer that may be null
bool c5_pass_ok(const char* who, const void* a, const void* b, const void* out, const void* scratch, const void* optional, int64_t batch,
                int32_t planes) {
  return lt_args_ok(who, {a, b, out, scratch}, [&] { return c5_shape_ok(who, batch, planes); }, {scratch}, "scratch") &&
         lt_aligned_ok(who, {a, b, out, optional}, "the tensors");
}

template <int PLANES>
void c5_forward(const float* x, const float* w, const float* bias, int64_t batch, void* scratch, float* y, hipStream_t s) {
  using G = C5<PLANES>;
  uint16_t* pack = static_cast<uint16_t*>(scratch);
  hipLaunchKernelGGL(k_conv5x5_pack<PLANES>, dim3(C5_OUT * G::K / 256), dim3(256), 0, s, w, pack);
  const int64_t M = batch * C5_OP;
  hipLaunchKernelGGL(k_conv5x5<PLANES>, dim3((unsigned)((M + LT_M - 1) / LT_M), C5_OUT / LT_N), dim3(256), 0, s, x, pack, bias, y, M);
}

template <int PLANES>
void c5_grad_weight(const float* gy, const float* x, int64_t batch, void* scratch, float* gw, hipStream_t s) {
  using G = C5<PLANES>;
  float* partial = reinterpret_cast<float*>(static_cast<char*>(scratch) + G::PACK_BYTES);
  const int64_t chunks = lt_ceil_div(batch, IPPM_CONV5X5_WGRAD_CHUNK);
  hipLaunchKernelGGL(k_conv5x5_wgrad<PLANES>, dim3((unsigned)(chunks * (C5_OUT / C5_WG_O))), dim3(256), 0, s, gy, x, partial, batch);
  hipLaunchKernelGGL(k_partial_sum<C5SumMap<PLANES>>, dim3(G::K_REAL), dim3(256), 0, s, partial, chunks, gw);
}

}  // namespace

extern "C" int ippm_conv5x5_bf16_scratch_bytes(int64_t batch, int32_t planes, int64_t* bytes) {
  if (!bytes) { ippm_set_error("ippm_conv5x5_bf16_scratch_bytes: null argument"); return -1; }
  if (!c5_shape_ok("ippm_conv5x5_bf16_scratch_bytes", batch, planes)) return -1;
  const int64_t chunks = lt_ceil_div(batch, IPPM_CONV5X5_WGRAD_CHUNK);
  *bytes = planes == 7 ? C5<7>::PACK_BYTES + chunks * C5<7>::PARTIAL * 4 : C5<12>::PACK_BYTES + chunks * C5<12>::PARTIAL * 4;
  return 0;
}

extern "C" int ippm_conv5x5_bf16_forward(const float* x, const float* w, const float* bias, int64_t batch, int32_t planes, void* scratch,
                                         float* y, void* stream) {
  if (!c5_pass_ok("ippm_conv5x5_bf16_forward", x, w, y, scratch, bias, batch, planes)) return -1;
  if (planes == 7) c5_forward<7>(x, w, bias, batch, scratch, y, S_(stream));
  else c5_forward<12>(x, w, bias, batch, scratch, y, S_(stream));
  IPPM_LAUNCH_CHECK("conv5x5_bf16_forward");
  return 0;
}

extern "C" int ippm_conv5x5_bf16_grad_weight(const float* gy, const float* x, int64_t batch, int32_t planes, void* scratch, float* gw,
                                             void* stream) {
  if (!c5_pass_ok("ippm_conv5x5_bf16_grad_weight", gy, x, gw, scratch, nullptr, batch, planes)) return -1;
  if (planes == 7) c5_grad_weight<7>(gy, x, batch, scratch, gw, S_(stream));
  else c5_grad_weight<12>(gy, x, batch, scratch, gw, S_(stream));
  IPPM_LAUNCH_CHECK("conv5x5_bf16_grad_weight");
  return 0;
}
