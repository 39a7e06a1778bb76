// The bf16 matrix-core trunk shared by the native actor and critic forwards (actor_infer.hip, critic_infer.hip): conv 5x5 -> 4x4 -> 4x4
// (11 -> 7 -> 4 -> 1), fc1, and fc3's product.  The two networks differ in the planes of their input (7 / 12: a compile-time parameter
// of the first layer and of the pack) and in what their head does with fc3's output.  Numerical contract: the
// input and the weights of every layer are bf16 (round to nearest even), products accumulate in float32 on the matrix cores, the
// float32 bias is added to the accumulator, ReLU (NaN passes: ippm_relu), and the activation is rounded to bf16 once, at the store; fc3's
// output is float32.
//
// Every layer up to fc1 is ONE implicit-GEMM kernel, k_actor_layer: out[m][n] = relu(bias[n] + sum_k A[m][k] W[n][k]) with N = 256,
// m = (sample, out_y, out_x), k = (tap_y, tap_x, channel) -- tap-major, channel-minor, so the K of a row is read straight from the
// channels-last activation (no im2col buffer) and the 64 k of a tile never straddle a tap of a 256-channel layer.  conv3 (one output
// position over a 4x4x256 input) and fc1 (1x1 over 256 channels) are the same formula with other extents.  Deterministic: a row's K
// order is fixed, no atomics, no split-K -- a sample's outputs do not depend on the batch around it.
//
// Everything here sits in an unnamed namespace: each translation unit that includes the header owns its instantiations.
#pragma once
#include "ippm_bf16_tile.h"

namespace {

constexpr int AI_N = 256;          // output channels of every hidden layer
constexpr int AI_K2 = 4096;        // conv2 / conv3: 4*4*256
constexpr int AI_K4 = 256;         // fc1, fc3
constexpr int AI_NPAD = 32;        // fc3's N = n_actions, zero-padded to two 16-wide MFMA tiles
constexpr int AI_SLICE = 4096;     // samples per internal slice of the batch: bounds the scratch
constexpr int AI_NBIAS = 4 * AI_N + AI_NPAD;

// The packed blob of a network with PLANES input planes: element offsets of the bf16 weights, then the float32 biases (byte offset
// BIAS_BYTES).  conv1's K = 5*5*PLANES is zero-padded to a multiple of the layer kernel's K step: 175 -> 192, 300 -> 320.
template <int PLANES>
struct NetPack {
  static constexpr int K1_REAL = 25 * PLANES;
  static constexpr int K1 = (K1_REAL + 63) / 64 * 64;
  static constexpr int64_t W1 = 0;
  static constexpr int64_t W2 = W1 + (int64_t)AI_N * K1;
  static constexpr int64_t W3 = W2 + (int64_t)AI_N * AI_K2;
  static constexpr int64_t W4 = W3 + (int64_t)AI_N * AI_K2;
  static constexpr int64_t W5 = W4 + (int64_t)AI_N * AI_K4;
  static constexpr int64_t WEND = W5 + (int64_t)AI_NPAD * AI_K4;
  static constexpr int64_t BIAS_BYTES = WEND * 2;
  static constexpr int64_t PACK_BYTES = BIAS_BYTES + (int64_t)AI_NBIAS * 4;
};

// bf16 activations per sample in the scratch: conv1 [7,7,256], conv2 [4,4,256], conv3 [256], fc1 [256]
constexpr int64_t AI_ACT1 = 49 * AI_N, AI_ACT2 = 16 * AI_N, AI_ACT3 = AI_N, AI_ACT4 = AI_N;
constexpr int64_t AI_SCRATCH_PER_SAMPLE = (AI_ACT1 + AI_ACT2 + AI_ACT3 + AI_ACT4) * 2;

// ---- packing ---------------------------------------------------------------------------------------------------------------------
// PyTorch's [O,C,kh,kw] / [O,I] float32 -> [O][K] bf16 with k = (ty*kw + tx)*C + c; one thread per packed element.
template <int PLANES>
__global__ void __launch_bounds__(256)
k_net_pack(const float* __restrict__ c1w, const float* __restrict__ c1b, const float* __restrict__ c2w, const float* __restrict__ c2b,
           const float* __restrict__ c3w, const float* __restrict__ c3b, const float* __restrict__ f1w, const float* __restrict__ f1b,
           const float* __restrict__ f3w, const float* __restrict__ f3b, int A, uint16_t* __restrict__ packed) {
  using P = NetPack<PLANES>;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < P::W2) {
    const int o = (int)(i / P::K1), k = (int)(i % P::K1);
    float v = 0.f;
    if (k < P::K1_REAL) { const int tap = k / PLANES, c = k % PLANES; v = c1w[(o * PLANES + c) * 25 + tap]; }
    packed[i] = ai_bf16(v);
  } else if (i < P::W4) {
    const bool second = i < P::W3;
    const int64_t j = i - (second ? P::W2 : P::W3);
    const int o = (int)(j / AI_K2), k = (int)(j % AI_K2), tap = k >> 8, c = k & 255;
    packed[i] = ai_bf16((second ? c2w : c3w)[((int64_t)o * 256 + c) * 16 + tap]);
  } else if (i < P::W5) {
    packed[i] = ai_bf16(f1w[i - P::W4]);
  } else if (i < P::WEND) {
    const int64_t j = i - P::W5;
    packed[i] = (j / AI_K4) < A ? ai_bf16(f3w[j]) : (uint16_t)0;
  } else if (i < P::WEND + AI_NBIAS) {
    const int j = (int)(i - P::WEND);
    float* bias = reinterpret_cast<float*>(reinterpret_cast<char*>(packed) + P::BIAS_BYTES);
    const float* src = j < 256 ? c1b : j < 512 ? c2b : j < 768 ? c3b : f1b;
    bias[j] = j < 1024 ? src[j & 255] : (j - 1024 < A ? f3b[j - 1024] : 0.f);
  }
}

// ---- one hidden layer ------------------------------------------------------------------------------------------------------------
// One workgroup tile of ippm_bf16_tile.h per (128 rows, 128 output channels).
struct LayerGeom {
  int IW, C;       // input width (positions) and channels; an input sample is IH*IW*C elements
  int KW;          // kernel width; K = KH*KW*C
  int OW, OP;      // output width and positions per sample (OH*OW)
  int in_sample;   // elements per input sample
  int K;           // padded K, a multiple of 64
};

// FIRST: the layer reads the float32 network input [B,11,11,PLANES] (5x5 kernel) and rounds it to bf16 on the way into LDS; otherwise
// the bf16 activation of the layer before (PLANES is not used).
template <bool FIRST, int PLANES = 0>
__global__ void __launch_bounds__(256)
k_actor_layer(const void* __restrict__ in_, const uint16_t* __restrict__ w, const float* __restrict__ bias, uint16_t* __restrict__ out,
              int64_t M, LayerGeom g) {
  __shared__ __attribute__((aligned(16))) uint16_t As[LT_M * LT_LD];
  __shared__ __attribute__((aligned(16))) uint16_t Ws[LT_N * LT_LD];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * LT_M;
  const int n0 = blockIdx.y * LT_N;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;

  const int sc = tid & 7, sr = tid >> 3;
  int64_t a_base[4];
  bool a_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + sr + 32 * i;
    a_ok[i] = m < M;
    const int64_t b = a_ok[i] ? m / g.OP : 0;
    const int p = a_ok[i] ? (int)(m - b * g.OP) : 0;
    const int oy = p / g.OW, ox = p - oy * g.OW;
    a_base[i] = b * g.in_sample + (int64_t)(oy * g.IW + ox) * g.C;
  }
  const uint16_t* wrow = w + (int64_t)(n0 + sr) * g.K + sc * 8;

  u32x4 a_reg[4], w_reg[4];
  auto load = [&](int s) __attribute__((always_inline)) {
    const int k0 = s * LT_K, k = k0 + sc * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) w_reg[i] = *reinterpret_cast<const u32x4*>(wrow + (int64_t)32 * i * g.K + k0);
    if (FIRST) {
      // float32 input, PLANES channels: the 5 taps of a kernel row and their channels are 5 * PLANES contiguous floats of the input,
      // and the next kernel row starts 11 * PLANES floats further on
      constexpr int ROW = 5 * PLANES, STRIDE = 11 * PLANES, K_REAL = 25 * PLANES;
      const float* in = static_cast<const float*>(in_);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int kk = k + j, ty = kk / ROW, r = kk - ty * ROW;
          v[j] = (a_ok[i] && kk < K_REAL) ? in[a_base[i] + ty * STRIDE + r] : 0.f;
        }
        a_reg[i] = lt_round8(v);
      }
    } else {
      const uint16_t* in = static_cast<const uint16_t*>(in_);
      const int tap = k / g.C, c = k - tap * g.C, ty = tap / g.KW, tx = tap - ty * g.KW;
      const int off = (ty * g.IW + tx) * g.C + c;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        a_reg[i] = a_ok[i] ? *reinterpret_cast<const u32x4*>(in + a_base[i] + off) : u32x4{0u, 0u, 0u, 0u};
    }
  };
  auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      lt_stage_row(As, i, a_reg[i]);
      lt_stage_row(Ws, i, w_reg[i]);
    }
  };

  floatx4 acc[4][4];   // [n tile][m tile]
  lt_zero(acc);
  lt_k_loop<LT_RELOAD_LAST, LT_FREE>(g.K / LT_K, load, stage, As, Ws, wm, wn, acc);

  auto row = [&](int ml) __attribute__((always_inline)) {
    const int64_t m = m0 + wm + ml;
    return m < M ? out + m * AI_N : nullptr;
  };
  lt_for_outputs(acc, row, [&](uint16_t* orow, int nl, const float4& v) __attribute__((always_inline)) {
    const int n = n0 + wn + nl;
    const float4 bv = *reinterpret_cast<const float4*>(bias + n);
    uint2 o;   // the NaN-passing ReLU of every bf16 store (ippm_relu), then the rounding
    o.x = (uint32_t)ai_relu_bf16(v.x + bv.x) | ((uint32_t)ai_relu_bf16(v.y + bv.y) << 16);
    o.y = (uint32_t)ai_relu_bf16(v.z + bv.z) | ((uint32_t)ai_relu_bf16(v.w + bv.w) << 16);
    *reinterpret_cast<uint2*>(orow + n) = o;
  });
}

// ---- fc3 on the matrix cores: one wavefront per 16 samples -------------------------------------------------------------------------
// L[r][n] = bias[n] + sum_k h[b0 + r][k] w[n][k] for the 16 samples from b0 on (rows past B are computed from zeros) and the 32 padded
// outputs; the wavefront's lanes have all written L when this returns (a barrier is part of it).
__device__ __forceinline__ void ai_fc3_tile(const uint16_t* __restrict__ h, const uint16_t* __restrict__ w, const float* __restrict__ bias,
                                            int64_t b0, int64_t B, float (*L)[AI_NPAD + 1]) {
  const int lane = threadIdx.x, fr = lane & 15, fk = (lane >> 4) * 8;
  const int64_t m = b0 + fr;
  floatx4 acc[2] = {};
#pragma unroll
  for (int k = 0; k < AI_K4; k += 32) {
    uint4 a = make_uint4(0, 0, 0, 0);
    if (m < B) a = *reinterpret_cast<const uint4*>(h + m * AI_K4 + k + fk);
    const bf16x8 af = __builtin_bit_cast(bf16x8, a);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const bf16x8 wf = *reinterpret_cast<const bf16x8*>(w + (nt * 16 + fr) * AI_K4 + k + fk);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af, acc[nt], 0, 0, 0);
    }
  }
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = nt * 16 + (lane >> 4) * 4 + r;
      L[fr][n] = acc[nt][r] + bias[n];
    }
  __syncthreads();
}

inline bool ai_actions_ok(const char* who, int32_t A) {
  if (A < 1 || A > AI_NPAD) { ippm_set_error(std::string(who) + ": n_actions must be in [1, 32]"); return false; }
  return true;
}

// ---- host side: the argument rules and launches both networks' C entry points share ----------------------------------------------
template <int PLANES>
int ai_pack_bytes(const char* who, int32_t n_actions, int64_t* bytes) {
  if (!bytes) { ippm_set_error(std::string(who) + ": null argument"); return -1; }
  if (!ai_actions_ok(who, n_actions)) return -1;
  *bytes = NetPack<PLANES>::PACK_BYTES;
  return 0;
}

template <int PLANES>
int ai_pack(const char* who, const float* const* p, int32_t n_actions, void* packed, void* stream) {
  bool null = !packed;
  for (int i = 0; i < 10; ++i) null = null || !p[i];
  if (null) { ippm_set_error(std::string(who) + ": null argument"); return -1; }
  if (!ai_actions_ok(who, n_actions)) return -1;
  if (reinterpret_cast<uintptr_t>(packed) & 15) { ippm_set_error(std::string(who) + ": packed must be 16-byte aligned"); return -1; }
  const int64_t n = NetPack<PLANES>::WEND + AI_NBIAS;
  hipLaunchKernelGGL(k_net_pack<PLANES>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p[0], p[1],
                     p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], (int)n_actions, static_cast<uint16_t*>(packed));
  IPPM_LAUNCH_CHECK(who);
  return 0;
}

inline int ai_scratch_bytes(const char* who, int64_t batch, int64_t* bytes) {
  if (!bytes || batch < 1) { ippm_set_error(std::string(who) + ": needs batch >= 1 and an output"); return -1; }
  *bytes = (batch < AI_SLICE ? batch : (int64_t)AI_SLICE) * AI_SCRATCH_PER_SAMPLE;
  return 0;
}

inline bool ai_forward_args_ok(const char* who, const void* packed, const void* scratch, int64_t batch, int32_t n_actions) {
  if (batch < 1) { ippm_set_error(std::string(who) + ": needs batch >= 1"); return false; }
  if (!ai_actions_ok(who, n_actions)) return false;
  if ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(scratch)) & 15) {
    ippm_set_error(std::string(who) + ": packed and scratch must be 16-byte aligned");
    return false;
  }
  return true;
}

// The scratch of a slice of S samples, and the trunk of nb <= S samples of it: conv1 .. fc1 -> act4 bf16 [nb,256].
struct NetScratch {
  uint16_t *act1, *act2, *act3, *act4;
  NetScratch(void* scratch, int64_t S) {
    act1 = static_cast<uint16_t*>(scratch);
    act2 = act1 + S * AI_ACT1;
    act3 = act2 + S * AI_ACT2;
    act4 = act3 + S * AI_ACT3;
  }
};

template <int PLANES>
void ai_launch_trunk(const void* packed, const float* in, int64_t nb, const NetScratch& a, hipStream_t s) {
  using P = NetPack<PLANES>;
  const uint16_t* w = static_cast<const uint16_t*>(packed);
  const float* bias = reinterpret_cast<const float*>(static_cast<const char*>(packed) + P::BIAS_BYTES);
  //                      IW  C       KW OW OP  in_sample         K
  const LayerGeom g1 = {11, PLANES, 5, 7, 49, 11 * 11 * PLANES, P::K1};
  const LayerGeom g2 = {7, 256, 4, 4, 16, 49 * 256, AI_K2};
  const LayerGeom g3 = {4, 256, 4, 1, 1, 16 * 256, AI_K2};
  const LayerGeom g4 = {1, 256, 1, 1, 1, 256, AI_K4};
  auto blocks = [](int64_t M) { return dim3((unsigned)((M + LT_M - 1) / LT_M), AI_N / LT_N); };
  hipLaunchKernelGGL((k_actor_layer<true, PLANES>), blocks(nb * 49), dim3(256), 0, s, static_cast<const void*>(in), w + P::W1, bias, a.act1,
                     nb * 49, g1);
  hipLaunchKernelGGL((k_actor_layer<false>), blocks(nb * 16), dim3(256), 0, s, static_cast<const void*>(a.act1), w + P::W2, bias + 256, a.act2,
                     nb * 16, g2);
  hipLaunchKernelGGL((k_actor_layer<false>), blocks(nb), dim3(256), 0, s, static_cast<const void*>(a.act2), w + P::W3, bias + 512, a.act3, nb,
                     g3);
  hipLaunchKernelGGL((k_actor_layer<false>), blocks(nb), dim3(256), 0, s, static_cast<const void*>(a.act3), w + P::W4, bias + 768, a.act4, nb,
                     g4);
}

}  // namespace
