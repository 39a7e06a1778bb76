// The learners' conv2 on the bf16 matrix cores, for the COMA update (actor/network.py:19-28, critic/network.py): the stride-1, unpadded
// 4x4 convolution with 256 input and 256 output channels -- forward, input gradient and weight gradient -- over channels-last float32
// tensors.  Numerical contract: every operand (x, w, gy) is rounded to bf16 (nearest even) on its way into LDS,
// products accumulate in float32 on mfma_f32_16x16x32_bf16, outputs are float32 and are not rounded again.  No float atomics; every
// output element has one owner and a fixed summation order, so a result depends on the inputs and the batch size only.
//
// Forward and input gradient are ONE implicit-GEMM kernel (k_conv4x4) on the tile of the inference layers (ippm_bf16_tile.h: 128 rows x
// 128 channels, K steps of 64 through LDS, lt_k_loop): out[m][n] = sum over taps, channels of in[row(m) + tap offset][ch] * W[n][tap][ch].
//   forward         m = (sample, oy, ox), every tap, W = [o][tap][c].
//   input gradient  a gather: gx[b,iy,ix,c] = sum over the taps (ty,tx) with (iy-ty, ix-tx) inside the output, and over o, of
//                   gy[b,iy-ty,ix-tx,o] * w[o,c,ty,tx].  Rows are position-major: the 128 rows of a tile are 128 samples at ONE input
//                   position, so the K loop runs over that position's valid taps only (256 of the 49 x 16 (position, tap) pairs of the
//                   7x7 geometry); W = [c][tap][o].
// Weight gradient: gw[o,c,ty,tx] = sum over r = (b,oy,ox) of gy[r][o] * x[r + tap][c].  The reduction runs over the ROW index of both
// operands, so both tiles go into LDS transposed ([channel][r]; the 16-byte fragment reads stay as they are).  The batch is cut into
// chunks of IPPM_CONV4X4_WGRAD_CHUNK samples; a workgroup owns one (chunk, tap, 128 c, 128 o) tile and writes its float32 partial sums
// to the scratch; k_partial_sum<C4SumMap> adds the partials in chunk order and writes PyTorch's [O,C,4,4] layout.
#include "ippm_bf16_net.h"

namespace {

constexpr int C4_CH = 256;                                  // input and output channels
constexpr int64_t C4_W = (int64_t)C4_CH * AI_K2;            // elements of one weight pack / of one chunk's partial sums
constexpr int64_t C4_PACKS_BYTES = 2 * C4_W * 2;            // [o][tap][c] for the forward, then [c][tap][o] for the input gradient

struct C4Geom { int ih, iw, oh, ow; };

// w float32 [O,C,4,4] -> bf16 [row][tap][col]; TRANSPOSED: row = c, col = o (the input gradient's pack), else row = o, col = c
template <bool TRANSPOSED>
__global__ void __launch_bounds__(256) k_conv4x4_pack(const float* __restrict__ w, uint16_t* __restrict__ packed) {
  const int i = blockIdx.x * 256 + threadIdx.x;             // < C4_W
  const int row = i >> 12, tap = (i >> 8) & 15, col = i & 255;
  const int o = TRANSPOSED ? col : row, c = TRANSPOSED ? row : col;
  packed[i] = ai_bf16(w[(o * C4_CH + c) * 16 + tap]);
}

// ---- forward / input gradient ------------------------------------------------------------------------------------------------------
// BWD false: in = x [B,ih,iw,256], out = y [B,oh,ow,256], grid.x = tiles of 128 of the B*oh*ow rows.
// BWD true:  in = gy [B,oh,ow,256], out = gx [B,ih,iw,256], grid.x = (tile of 128 samples) * ih*iw + input position.
// The K loop and the store are written out here: on lt_k_loop and lt_for_outputs the input gradient measured 1 to 3 % slower
// (profiles/r20/README.md); the instruction stream of this form is the one measured before the tile header existed.
template <bool BWD>
__global__ void __launch_bounds__(256)
k_conv4x4(const float* __restrict__ in, const uint16_t* __restrict__ w, float* __restrict__ out, int64_t B, C4Geom g) {
  __shared__ __attribute__((aligned(16))) uint16_t As[LT_M * LT_LD];
  __shared__ __attribute__((aligned(16))) uint16_t Ws[LT_N * LT_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.y * LT_N;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int OP = g.oh * g.ow, IP = g.ih * g.iw;

  // rows of the tile: [m0, m0 + 128) of M rows; BWD: the rows are samples, all at input position (iy, ix)
  int iy = 0, ix = 0;
  int64_t m0, M;
  uint32_t taps = 0xFFFFu;                                  // bit ty*4+tx: the tap takes part
  if (BWD) {
    const int pos = (int)(blockIdx.x % (unsigned)IP);
    m0 = (int64_t)(blockIdx.x / (unsigned)IP) * LT_M;
    M = B;
    iy = pos / g.iw;
    ix = pos - iy * g.iw;
    taps = 0;
    for (int t = 0; t < 16; ++t) {
      const int oy = iy - (t >> 2), ox = ix - (t & 3);
      if (oy >= 0 && oy < g.oh && ox >= 0 && ox < g.ow) taps |= 1u << t;
    }
  } else {
    m0 = (int64_t)blockIdx.x * LT_M;
    M = B * OP;
  }

  // staging: thread -> chunk column (8 k) and 4 rows, 32 apart
  const int sc = tid & 7, sr = tid >> 3;
  int64_t a_base[4];
  bool a_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + sr + 32 * i;
    a_ok[i] = m < M;
    if (BWD) {
      a_base[i] = (a_ok[i] ? m : 0) * OP * C4_CH + sc * 8;
    } else {
      const int64_t b = a_ok[i] ? m / OP : 0;
      const int p = a_ok[i] ? (int)(m - b * OP) : 0;
      const int oy = p / g.ow, ox = p - oy * g.ow;
      a_base[i] = (b * IP + oy * g.iw + ox) * C4_CH + sc * 8;
    }
  }
  const uint16_t* wrow = w + (int64_t)(n0 + sr) * AI_K2 + sc * 8;

  float4 a_lo[4], a_hi[4];
  u32x4 w_reg[4];
  auto load = [&](int tap, int sub) __attribute__((always_inline)) {
    const int ty = tap >> 2, tx = tap & 3;
    const int a_off = (BWD ? (iy - ty) * g.ow + (ix - tx) : ty * g.iw + tx) * C4_CH + sub * LT_K;
    const int w_off = tap * C4_CH + sub * LT_K;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w_reg[i] = *reinterpret_cast<const u32x4*>(wrow + (int64_t)32 * i * AI_K2 + w_off);
      a_lo[i] = a_hi[i] = float4{0.f, 0.f, 0.f, 0.f};
      if (a_ok[i]) {
        a_lo[i] = *reinterpret_cast<const float4*>(in + a_base[i] + a_off);
        a_hi[i] = *reinterpret_cast<const float4*>(in + a_base[i] + a_off + 4);
      }
    }
  };
  auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<u32x4*>(&As[(sr + 32 * i) * LT_LD + sc * 8]) = lt_round8({a_lo[i].x, a_lo[i].y, a_lo[i].z, a_lo[i].w, a_hi[i].x, a_hi[i].y, a_hi[i].z, a_hi[i].w});
      *reinterpret_cast<u32x4*>(&Ws[(sr + 32 * i) * LT_LD + sc * 8]) = w_reg[i];
    }
  };

  floatx4 acc[4][4];   // [n tile][m tile]
  lt_zero(acc);

  const int fr = lane & 15, fk = (lane >> 4) * 8;
  const int nsteps = __popc(taps) * (C4_CH / LT_K);         // (every position has a tap inside: nsteps >= 4)
  int tap = __ffs((int)taps) - 1, sub = 0;
  load(tap, sub);
  for (int s = 0; s < nsteps; ++s) {
    __syncthreads();          // the previous step's fragment reads are done
    stage();
    __syncthreads();
    if (s + 1 < nsteps) {     // (uniform over the workgroup)
      if (++sub == C4_CH / LT_K) {
        sub = 0;
        taps &= taps - 1;
        tap = __ffs((int)taps) - 1;
      }
      load(tap, sub);
    }
    lt_mma_step(As, Ws, wm, wn, fr, fk, acc);
  }

  // D[n][m]: lane holds m = lane & 15 and n = (lane >> 4) * 4 + reg
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int64_t m = m0 + wm + mt * 16 + fr;
    if (m >= M) continue;
    float* row = out + (BWD ? m * IP + (iy * g.iw + ix) : m) * C4_CH;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int n = n0 + wn + nt * 16 + (lane >> 4) * 4;
      *reinterpret_cast<float4*>(row + n) = float4{acc[nt][mt][0], acc[nt][mt][1], acc[nt][mt][2], acc[nt][mt][3]};
    }
  }
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------------------
// blockIdx.x = chunk * 64 + tile, tile = tap * 4 + (c half) * 2 + (o half).  The K of this GEMM is r = (sample of the chunk, oy, ox) in
// steps of 64.  Staging: thread -> 4 channels (one float4 per row) of 8 consecutive r; after the rounding the 8 r of a channel are one
// 16-byte LDS store, and the 8 lanes that share a channel row write 128 contiguous bytes of it.
__global__ void __launch_bounds__(256)
k_conv4x4_wgrad(const float* __restrict__ gy, const float* __restrict__ x, float* __restrict__ partial, int64_t B, C4Geom g) {
  __shared__ __attribute__((aligned(16))) uint16_t Xs[LT_M * LT_LD];   // [c][r]
  __shared__ __attribute__((aligned(16))) uint16_t Gs[LT_N * LT_LD];   // [o][r]
  const int tid = threadIdx.x, wave = tid >> 6;
  const int64_t chunk = blockIdx.x >> 6;
  const int tile = blockIdx.x & 63, tap = tile >> 2, c0 = ((tile >> 1) & 1) * LT_M, o0 = (tile & 1) * LT_N;
  const int ty = tap >> 2, tx = tap & 3;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int OP = g.oh * g.ow;
  const int64_t b0 = chunk * IPPM_CONV4X4_WGRAD_CHUNK;
  const int ns = B - b0 < IPPM_CONV4X4_WGRAD_CHUNK ? (int)(B - b0) : IPPM_CONV4X4_WGRAD_CHUNK;
  const int R = ns * OP;                                    // rows of this chunk (<= 256 * 64)
  const float* gy0 = gy + b0 * OP * C4_CH + o0;
  const float* x0 = x + (b0 * g.ih * g.iw + ty * g.iw + tx) * C4_CH + c0;

  const int rg = tid & 7, c4 = (tid >> 3) * 4;              // rows rg*8 .. rg*8+7 of the step, channels c4 .. c4+3 of the tile
  float4 xr[8], gr[8];
  auto load = [&](int s) __attribute__((always_inline)) {
    const int r0 = s * LT_K + rg * 8;
    int b = r0 / OP, p = r0 - b * OP, oy = p / g.ow, ox = p - oy * g.ow;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xr[j] = gr[j] = float4{0.f, 0.f, 0.f, 0.f};
      if (r0 + j < R) {
        gr[j] = *reinterpret_cast<const float4*>(gy0 + (int64_t)(r0 + j) * C4_CH + c4);
        xr[j] = *reinterpret_cast<const float4*>(x0 + ((int64_t)(b * g.ih + oy) * g.iw + ox) * C4_CH + c4);
      }
      if (++ox == g.ow) {
        ox = 0;
        if (++oy == g.oh) { oy = 0; ++b; }
      }
    }
  };
  auto stage = [&]() __attribute__((always_inline)) {
    const float* xf = reinterpret_cast<const float*>(xr);
    const float* gf = reinterpret_cast<const float*>(gr);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float hx[8], hg[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { hx[j] = xf[j * 4 + q]; hg[j] = gf[j * 4 + q]; }
      *reinterpret_cast<u32x4*>(&Xs[(c4 + q) * LT_LD + rg * 8]) = lt_round8(hx);
      *reinterpret_cast<u32x4*>(&Gs[(c4 + q) * LT_LD + rg * 8]) = lt_round8(hg);
    }
  };

  floatx4 acc[4][4];   // [o tile][c tile]
  lt_zero(acc);
  lt_k_loop<LT_GUARDED, LT_FREE>((R + LT_K - 1) / LT_K, load, stage, Xs, Gs, wm, wn, acc);

  // m is c, n is o; partial [chunk][tap][c][o]
  float* pt = partial + (chunk * 16 + tap) * (int64_t)(C4_CH * C4_CH);
  auto row = [&](int ml) __attribute__((always_inline)) { return pt + (c0 + wm + ml) * C4_CH; };
  lt_for_outputs(acc, row, [&](float* prow, int nl, const float4& v) __attribute__((always_inline)) {
    *reinterpret_cast<float4*>(prow + (o0 + wn + nl)) = v;
  });
}

// gw[o][c][tap] from element i = (tap, c, o) of the partials [chunk][tap][c][o]: the reads are coalesced over o
struct C4SumMap {
  static constexpr int64_t STRIDE = C4_W;
  static __device__ int out(int i) { return ((i & 255) * C4_CH + ((i >> 8) & 255)) * 16 + (i >> 16); }
};

// ---- host side -----------------------------------------------------------------------------------------------------------------------
bool c4_shape_ok(const char* who, int64_t batch, int32_t ih, int32_t iw) {
  if (!lt_batch_ok(who, batch)) return false;
  if (ih < 4 || ih > 11 || iw < 4 || iw > 11) { ippm_set_error(std::string(who) + ": ih and iw must be in [4, 11]"); return false; }
  return true;
}

// the three passes: two tensors in, one out, the scratch
bool c4_pass_ok(const char* who, const void* a, const void* b, const void* out, const void* scratch, int64_t batch, int32_t ih, int32_t iw) {
  return lt_args_ok(who, {a, b, out, scratch}, [&] { return c4_shape_ok(who, batch, ih, iw); }, {scratch}, "scratch") &&
         lt_aligned_ok(who, {a, b, out}, "the tensors");
}

}  // namespace

extern "C" int ippm_conv4x4_bf16_scratch_bytes(int64_t batch, int32_t ih, int32_t iw, int64_t* bytes) {
  if (!bytes) { ippm_set_error("ippm_conv4x4_bf16_scratch_bytes: null argument"); return -1; }
  if (!c4_shape_ok("ippm_conv4x4_bf16_scratch_bytes", batch, ih, iw)) return -1;
  *bytes = C4_PACKS_BYTES + lt_ceil_div(batch, IPPM_CONV4X4_WGRAD_CHUNK) * C4_W * 4;
  return 0;
}

extern "C" int ippm_conv4x4_bf16_forward(const float* x, const float* w, int64_t batch, int32_t ih, int32_t iw, void* scratch, float* y,
                                         void* stream) {
  if (!c4_pass_ok("ippm_conv4x4_bf16_forward", x, w, y, scratch, batch, ih, iw)) return -1;
  hipStream_t s = S_(stream);
  const C4Geom g = {ih, iw, ih - 3, iw - 3};
  uint16_t* pack = static_cast<uint16_t*>(scratch);
  hipLaunchKernelGGL(k_conv4x4_pack<false>, dim3((unsigned)(C4_W / 256)), dim3(256), 0, s, w, pack);
  const int64_t M = batch * g.oh * g.ow;
  hipLaunchKernelGGL(k_conv4x4<false>, dim3((unsigned)((M + LT_M - 1) / LT_M), C4_CH / LT_N), dim3(256), 0, s, x, pack, y, batch, g);
  IPPM_LAUNCH_CHECK("conv4x4_bf16_forward");
  return 0;
}

extern "C" int ippm_conv4x4_bf16_grad_input(const float* gy, const float* w, int64_t batch, int32_t ih, int32_t iw, void* scratch, float* gx,
                                            void* stream) {
  if (!c4_pass_ok("ippm_conv4x4_bf16_grad_input", gy, w, gx, scratch, batch, ih, iw)) return -1;
  hipStream_t s = S_(stream);
  const C4Geom g = {ih, iw, ih - 3, iw - 3};
  uint16_t* pack = static_cast<uint16_t*>(scratch) + C4_W;
  hipLaunchKernelGGL(k_conv4x4_pack<true>, dim3((unsigned)(C4_W / 256)), dim3(256), 0, s, w, pack);
  const int64_t tiles = (batch + LT_M - 1) / LT_M * (ih * iw);
  hipLaunchKernelGGL(k_conv4x4<true>, dim3((unsigned)tiles, C4_CH / LT_N), dim3(256), 0, s, gy, pack, gx, batch, g);
  IPPM_LAUNCH_CHECK("conv4x4_bf16_grad_input");
  return 0;
}

extern "C" int ippm_conv4x4_bf16_grad_weight(const float* gy, const float* x, int64_t batch, int32_t ih, int32_t iw, void* scratch, float* gw,
                                             void* stream) {
  if (!c4_pass_ok("ippm_conv4x4_bf16_grad_weight", gy, x, gw, scratch, batch, ih, iw)) return -1;
  hipStream_t s = S_(stream);
  const C4Geom g = {ih, iw, ih - 3, iw - 3};
  float* partial = reinterpret_cast<float*>(static_cast<char*>(scratch) + C4_PACKS_BYTES);
  const int64_t chunks = lt_ceil_div(batch, IPPM_CONV4X4_WGRAD_CHUNK);
  hipLaunchKernelGGL(k_conv4x4_wgrad, dim3((unsigned)(chunks * 64)), dim3(256), 0, s, gy, x, partial, batch, g);
  hipLaunchKernelGGL(k_partial_sum<C4SumMap>, dim3((unsigned)(C4_W / 256)), dim3(256), 0, s, partial, chunks, gw);
  IPPM_LAUNCH_CHECK("conv4x4_bf16_grad_weight");
  return 0;
}
