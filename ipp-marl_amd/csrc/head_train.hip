// The heads of the COMA update (actor/network.py:81-88, critic/network.py:42-47; actor/learner.py:52-97, critic/learner.py:76-92): everything
// behind conv3 in a learner's forward-with-gradient pass -- fc1, ReLU, fc3, the loss and the gradients back to conv3's output h [B,256] --
// over float32 tensors in PyTorch's layouts (fc1_w [256,256], fc3_w [A,256]).
// Numerical contract (as csrc/conv4x4_train.hip): both operands of the six products (z1 = h W1^T, logits = a1 W3^T,
// ga1 = dlogits W3, gh = gz1 W1, gW1 = gz1^T h, gW3 = dlogits^T a1) are rounded to bf16 (nearest even) on their way into LDS or into a
// fragment, products accumulate in float32 on mfma_f32_16x16x32_bf16, outputs are float32 and are not rounded again.  Everything else --
// bias adds, the NaN-passing ReLU of k_bias_relu (ippm_relu), gz1 = ga1 [a1 > 0], the bias gradients, the losses' per-row arithmetic -- is float32 on
// unrounded values (the one sum over the batch that makes a loss is carried in double and rounded once).
// No float atomics; every output element has one owner and a fixed summation order.  Sums over the batch (gW1, gb1, gW3, gb3, the loss)
// are per-chunk partial sums (IPPM_HEAD_WGRAD_CHUNK samples) in the scratch, added in chunk order by a second kernel.
//
// Row kernels (k_head_rows, k_head_gz1) own HT_M = 64 rows and all 256 columns: one workgroup, four wavefronts of 64 x 64 (the tile of ippm_bf16_tile.h).
// The weights arrive as float32 and are rounded while they are staged -- no pack kernel: these passes are launch-bound at the reference's
// 60-sample minibatch, where the staging of the 256 KiB of fc1's weight IS the kernel's duration whatever the row tile, and a tile of 64
// rows is the smallest that does not multiply that staging at the large batches.
// Every load is unconditional on a clamped address (a row, a column or an action that does not exist reads the tensor's first and is
// zeroed afterwards).
#include "ippm_bf16_net.h"

namespace {

constexpr int HD = AI_N;                                    // width of h, a1 and fc1
constexpr int HT_M = 64;                                    // rows per workgroup of the row kernels
constexpr int HC = IPPM_HEAD_WGRAD_CHUNK;                   // samples per partial sum
static_assert(HC == LT_K && HC == HT_M, "a chunk is one K step of the weight-gradient GEMM and one row tile");
constexpr int A1_LD = HD + 8;                               // LDS row of the bf16 a1 tile
constexpr int D_LD = AI_NPAD + 8;                           // LDS row of the (action-padded) tiles of k_head_gz1
// floats of one chunk's partial sums: gW1 [k][o], gW3 [k][a padded], gb1, gb3
constexpr int64_t HP_W1 = 0, HP_W3 = HP_W1 + (int64_t)HD * HD, HP_B1 = HP_W3 + (int64_t)HD * AI_NPAD, HP_B3 = HP_B1 + HD;
constexpr int64_t HP_FLOATS = HP_B3 + AI_NPAD;

// lt_for_tiles' answer about a row of these kernels: none is skipped (rows past the batch still go into the a1 tile in LDS)
struct HdRow {
  int ml;
  __device__ explicit operator bool() const { return true; }
};
__device__ __forceinline__ HdRow hd_every_row(int ml) { return HdRow{ml}; }

// the scratch: the loss's partial sums double [chunks] (padded to 16 bytes), gz1 [B,256], the weight gradients' partial sums
// [chunks][HP_FLOATS]
struct HeadScratch {
  double* loss;
  float *gz1, *partial;
  static int64_t loss_doubles(int64_t batch) { return (lt_ceil_div(batch, HC) + 1) / 2 * 2; }
  static int64_t bytes(int64_t batch) { return loss_doubles(batch) * 8 + (batch * HD + lt_ceil_div(batch, HC) * HP_FLOATS) * 4; }
  HeadScratch(void* scratch, int64_t batch) {
    loss = static_cast<double*>(scratch);
    gz1 = reinterpret_cast<float*>(loss + loss_doubles(batch));
    partial = gz1 + batch * HD;
  }
};

// ---- rows x 256 <- rows x 256 times a 256 x 256 weight ---------------------------------------------------------------------------------
// FORWARD: a1[m][n] = relu(b1[n] + sum_k x[m][k] W1[n][k]), then logits[m][a] = b3[a] + sum_n a1[m][n] W3[a][n] from the bf16 a1 tile in LDS
//          (fc3's weight rows straight from memory into the fragments: one wavefront per 16 rows, as ai_fc3_tile).
// else:    out[m][n] = sum_k x[m][k] W1[k][n] -- the input gradient gh = gz1 W1: the weight tile goes into LDS transposed.
template <bool FORWARD>
__global__ void __launch_bounds__(256)
k_head_rows(const float* __restrict__ x, const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w3,
            const float* __restrict__ b3, float* __restrict__ out, float* __restrict__ logits, int64_t B, int A) {
  __shared__ __attribute__((aligned(16))) uint16_t As[HT_M * LT_LD];
  __shared__ __attribute__((aligned(16))) uint16_t Ws[HD * LT_LD];          // (the forward's bf16 a1 tile [64][A1_LD] afterwards)
  static_assert(HT_M * A1_LD <= HD * LT_LD, "the a1 tile fits into the weight tile");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * HT_M;
  const int sc = tid & 7, sr = tid >> 3;

  u32x4 a_reg[2], w_reg[8];
  auto load = [&](int s) __attribute__((always_inline)) {
    const int k0 = s * LT_K;
    float4 xv[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t m = m0 + sr + 32 * i;
      const float4* p = reinterpret_cast<const float4*>(x + (m < B ? m : 0) * HD + k0 + sc * 8);
      xv[i][0] = p[0]; xv[i][1] = p[1];
    }
    if (FORWARD) {
      float4 wv[8][2];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float4* p = reinterpret_cast<const float4*>(w1 + (sr + 32 * i) * HD + k0 + sc * 8);
        wv[i][0] = p[0]; wv[i][1] = p[1];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float v[8] = {wv[i][0].x, wv[i][0].y, wv[i][0].z, wv[i][0].w, wv[i][1].x, wv[i][1].y, wv[i][1].z, wv[i][1].w};
        w_reg[i] = lt_cvt8(v);
      }
    } else {
      // Ws[n = tid][k - k0]: 8 consecutive k of one n are 8 rows of W1; lanes next to each other read floats next to each other
      float wv[8][8];
#pragma unroll
      for (int g = 0; g < 8; ++g)
#pragma unroll
        for (int j = 0; j < 8; ++j) wv[g][j] = w1[(k0 + g * 8 + j) * HD + tid];
#pragma unroll
      for (int g = 0; g < 8; ++g) w_reg[g] = lt_cvt8(wv[g]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bool ok = m0 + sr + 32 * i < B;
      float v[8] = {xv[i][0].x, xv[i][0].y, xv[i][0].z, xv[i][0].w, xv[i][1].x, xv[i][1].y, xv[i][1].z, xv[i][1].w};
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = ok ? v[j] : 0.f;
      a_reg[i] = lt_cvt8(v);
    }
  };
  auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 2; ++i) lt_stage_row(As, i, a_reg[i]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (FORWARD) lt_stage_row(Ws, i, w_reg[i]);
      else *reinterpret_cast<u32x4*>(&Ws[tid * LT_LD + i * 8]) = w_reg[i];
    }
  };

  floatx4 acc[4][4];   // [n tile][m tile]
  lt_zero(acc);
  const int wn = wave * 64;
  lt_k_loop<LT_GUARDED, LT_ROLLED>(HD / LT_K, load, stage, As, Ws, 0, wn, acc);

  uint16_t* A1s = Ws;
  if (FORWARD) __syncthreads();            // every wavefront is done with the weight tile
  lt_for_outputs(acc, hd_every_row, [&](HdRow r, int nl, float4 v) __attribute__((always_inline)) {
    const int ml = r.ml;
    const int64_t m = m0 + ml;
    const int n = wn + nl;
    if (FORWARD) {
      const float4 bv = *reinterpret_cast<const float4*>(b1 + n);
      v.x = ippm_relu(v.x + bv.x); v.y = ippm_relu(v.y + bv.y); v.z = ippm_relu(v.z + bv.z); v.w = ippm_relu(v.w + bv.w);
      *reinterpret_cast<uint2*>(&A1s[ml * A1_LD + n]) = make_uint2(lt_cvt2(v.x, v.y), lt_cvt2(v.z, v.w));
    }
    if (m < B) *reinterpret_cast<float4*>(out + m * HD + n) = v;
  });
  if (!FORWARD) return;
  __syncthreads();

  // fc3: this wavefront's 16 rows x the 32 padded actions
  floatx4 acc3[2] = {};
  const int fr = lane & 15, fk = (lane >> 4) * 8, ml = wave * 16 + fr;
#pragma unroll
  for (int k = 0; k < HD; k += 32) {
    const bf16x8 af = *reinterpret_cast<const bf16x8*>(&A1s[ml * A1_LD + k + fk]);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int a = nt * 16 + fr;
      const float4* p = reinterpret_cast<const float4*>(w3 + (a < A ? a : 0) * HD + k + fk);
      const float4 lo = p[0], hi = p[1];
      float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = a < A ? v[j] : 0.f;
      acc3[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, lt_cvt8(v)), af, acc3[nt], 0, 0, 0);
    }
  }
  const int64_t m = m0 + ml;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = nt * 16 + (lane >> 4) * 4 + r;
      const float bias = b3[a < A ? a : 0];
      if (m < B && a < A) logits[m * A + a] = acc3[nt][r] + bias;
    }
}

// ---- gz1 = (dlogits * scale) W3 [a1 > 0]: 64 rows x 256 columns, K = the 32 padded actions (one MFMA K step) ---------------------------
__global__ void __launch_bounds__(256)
k_head_gz1(const float* __restrict__ dlogits, const float* __restrict__ scale_dev, const float* __restrict__ w3, const float* __restrict__ a1,
           float* __restrict__ gz1, int64_t B, int A) {
  __shared__ __attribute__((aligned(16))) uint16_t Wt[HD * D_LD];            // [n][a] = W3[a][n]
  __shared__ __attribute__((aligned(16))) uint16_t Ds[HT_M * D_LD];          // [m][a]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * HT_M;
  const float scale = scale_dev ? *scale_dev : 1.f;
  {
    float v[AI_NPAD];
#pragma unroll
    for (int a = 0; a < AI_NPAD; ++a) v[a] = w3[(a < A ? a : 0) * HD + tid];
#pragma unroll
    for (int a = 0; a < AI_NPAD; ++a) v[a] = a < A ? v[a] : 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float q[8] = {v[g * 8], v[g * 8 + 1], v[g * 8 + 2], v[g * 8 + 3], v[g * 8 + 4], v[g * 8 + 5], v[g * 8 + 6], v[g * 8 + 7]};
      *reinterpret_cast<u32x4*>(&Wt[tid * D_LD + g * 8]) = lt_cvt8(q);
    }
    const int ml = tid >> 2, a8 = (tid & 3) * 8;
    const int64_t m = m0 + ml;
    float d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = dlogits[(m < B ? m : 0) * A + (a8 + j < A ? a8 + j : 0)];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = (m < B && a8 + j < A) ? d[j] * scale : 0.f;
    *reinterpret_cast<u32x4*>(&Ds[ml * D_LD + a8]) = lt_cvt8(d);
  }
  __syncthreads();
  const int fr = lane & 15, fk = (lane >> 4) * 8, wn = wave * 64;
  bf16x8 af[4], wf[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    af[t] = *reinterpret_cast<const bf16x8*>(&Ds[(t * 16 + fr) * D_LD + fk]);
    wf[t] = *reinterpret_cast<const bf16x8*>(&Wt[(wn + t * 16 + fr) * D_LD + fk]);
  }
  auto tile = [&](int nt, int mt) __attribute__((always_inline)) {   // K is one MFMA: a tile is made when its outputs are asked for
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], af[mt], floatx4{}, 0, 0, 0);
  };
  lt_for_tiles<4>(tile, hd_every_row, [&](HdRow r, int nl, const float4& g) __attribute__((always_inline)) {
    const int64_t m = m0 + r.ml;
    const int n = wn + nl;
    const float4 a = *reinterpret_cast<const float4*>(a1 + (m < B ? m : 0) * HD + n);
    // the mask is a FACTOR, as the definition has it (gz1 = ga1 [a1 > 0]): a non-finite ga1 behind a closed ReLU gives NaN, not 0
    const float4 o = float4{g.x * (a.x > 0.f ? 1.f : 0.f), g.y * (a.y > 0.f ? 1.f : 0.f), g.z * (a.z > 0.f ? 1.f : 0.f),
                            g.w * (a.w > 0.f ? 1.f : 0.f)};
    if (m < B) *reinterpret_cast<float4*>(gz1 + m * HD + n) = o;
  });
}

// ---- the weight and bias gradients of a chunk -----------------------------------------------------------------------------------------
// blockIdx.x = chunk * 5 + q.  q < 4: gW1[o][k] (the 64 o from q * 64 on, all k) = sum over the chunk's rows r of gz1[r][o] h[r][k], and
// gb1[o] = sum_r gz1[r][o]; q = 4: gW3[a][k] = sum_r d[r][a] a1[r][k] and gb3[a] = sum_r d[r][a], d = dlogits * scale, over the 32 padded
// actions (the G tile's rows 32..63 are zeros).  The K of this GEMM is r: ONE step of 64.  Both tiles go into LDS transposed:
//   Gs [o][r]: thread -> column tid & 63, the 16 rows (tid >> 6) * 16 ..; their float32 sum, in row order, is the thread's share of the
//              bias gradient (four shares per column, added in order).
//   Xs [k][r]: thread -> k = tid, all 64 rows.
// A wavefront owns the 64 o and the 64 k from wave * 64 on.  Partial sums go to the scratch [chunk][HP_FLOATS].
__global__ void __launch_bounds__(256)
k_head_wgrad(const float* __restrict__ gz1, const float* __restrict__ dlogits, const float* __restrict__ scale_dev, const float* __restrict__ h,
             const float* __restrict__ a1, float* __restrict__ partial, int64_t B, int A) {
  __shared__ __attribute__((aligned(16))) uint16_t Xs[HD * LT_LD];           // [k][r]
  __shared__ __attribute__((aligned(16))) uint16_t Gs[64 * LT_LD];           // [o][r]
  __shared__ float part[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t chunk = blockIdx.x / 5;
  const int q = (int)(blockIdx.x - chunk * 5);
  const bool third = q == 4;                                                 // (uniform over the workgroup)
  const int64_t b0 = chunk * HC;
  const int ns = B - b0 < HC ? (int)(B - b0) : HC;
  const float* gsrc = third ? dlogits : gz1 + q * 64;
  const float* xsrc = third ? a1 : h;
  const int ld = third ? A : HD, ncols = third ? A : 64;
  const float scale = (third && scale_dev) ? *scale_dev : 1.f;
  {
    const int c = tid & 63, rg = tid >> 6;
    const bool c_ok = c < ncols;
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int r = rg * 16 + j;
      v[j] = gsrc[(b0 + (r < ns ? r : 0)) * ld + (c_ok ? c : 0)];
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      v[j] = (c_ok && rg * 16 + j < ns) ? v[j] * scale : 0.f;
      s += v[j];
    }
    part[rg][c] = s;
    const float lo[8] = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]}, hi[8] = {v[8], v[9], v[10], v[11], v[12], v[13], v[14], v[15]};
    *reinterpret_cast<u32x4*>(&Gs[c * LT_LD + rg * 16]) = lt_cvt8(lo);
    *reinterpret_cast<u32x4*>(&Gs[c * LT_LD + rg * 16 + 8]) = lt_cvt8(hi);
  }
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    float v[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const int r = half * 32 + j;
      v[j] = xsrc[(b0 + (r < ns ? r : 0)) * HD + tid];
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float w[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) w[j] = half * 32 + g * 8 + j < ns ? v[g * 8 + j] : 0.f;
      *reinterpret_cast<u32x4*>(&Xs[tid * LT_LD + half * 32 + g * 8]) = lt_cvt8(w);
    }
  }
  __syncthreads();

  floatx4 acc[4][4];   // [o tile][k tile]
  lt_zero(acc);
  const int wk = wave * 64;
  lt_mma_step(Xs, Gs, wk, 0, lane & 15, (lane >> 4) * 8, acc);

  // m is k, n is o (gW3: the action)
  float* pt = partial + chunk * HP_FLOATS;
  lt_for_outputs(acc, hd_every_row, [&](HdRow r, int o, const float4& v) __attribute__((always_inline)) {
    const int k = wk + r.ml;
    if (!third) *reinterpret_cast<float4*>(pt + HP_W1 + k * HD + q * 64 + o) = v;
    else if (o < AI_NPAD) *reinterpret_cast<float4*>(pt + HP_W3 + k * AI_NPAD + o) = v;
  });
  if (tid < (third ? AI_NPAD : 64)) {
    const float s = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    pt[third ? HP_B3 + tid : HP_B1 + q * 64 + tid] = s;
  }
}

// the partial sums [chunk][HP_FLOATS] added in chunk order; one thread per element, each written to its place in PyTorch's layouts
__global__ void __launch_bounds__(256)
k_head_wgrad_sum(const float* __restrict__ partial, int64_t chunks, int A, float* __restrict__ gw1, float* __restrict__ gb1,
                 float* __restrict__ gw3, float* __restrict__ gb3) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HP_FLOATS) return;
  float s = 0.f;
  for (int64_t ch = 0; ch < chunks; ++ch) s += partial[ch * HP_FLOATS + i];
  if (i < HP_W3) gw1[(i & 255) * HD + (i >> 8)] = s;
  else if (i < HP_B1) {
    const int j = i - (int)HP_W3, k = j >> 5, a = j & 31;
    if (a < A) gw3[a * HD + k] = s;
  } else if (i < HP_B3) gb1[i - HP_B1] = s;
  else if (i - HP_B3 < A) gb3[i - HP_B3] = s;
}

// ---- the losses -------------------------------------------------------------------------------------------------------------------------
// The loss is ONE float32 number summed over the whole batch: its per-row terms are widened to double, added in a fixed order (row order
// within a chunk, then chunk order) and rounded to float32 once, so the sum's own rounding never shows in it.  The critic's term is the
// exact square of the exact difference of the two float32 operands; the actor's is the float32 product adv log p w.
// critic/learner.py:76-92: one thread per row of a chunk.  An action outside [0, A) gives NaN (q_chosen, the loss) and reads nothing out
// of range.
__global__ void __launch_bounds__(HC)
k_critic_loss(const float* __restrict__ q, const int32_t* __restrict__ action, const float* __restrict__ td, int64_t B, int A,
              double* __restrict__ part, float* __restrict__ q_chosen, float* __restrict__ dq) {
  __shared__ double sq[HC];
  const int r = threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x * HC + r, bc = b < B ? b : 0;
  const int a = action[bc];
  const bool a_ok = a >= 0 && a < A;
  const float qv = q[bc * A + (a_ok ? a : 0)];
  const float qc = a_ok ? qv : __builtin_nanf("");
  const float tdv = td[bc];
  const float d = qc - tdv;
  const double dd = (double)qc - (double)tdv;
  sq[r] = b < B ? dd * dd : 0.0;
  if (b < B) {
    q_chosen[b] = qc;
    const float g = 2.f * d / (float)B;
    for (int j = 0; j < A; ++j) dq[b * A + j] = (j == a || !a_ok) ? g : 0.f;
  }
  __syncthreads();
  if (r == 0) {
    double s = 0.0;
    for (int j = 0; j < HC; ++j) s += sq[j];
    part[blockIdx.x] = s;
  }
}

// actor/learner.py:52-97: one 32-lane half-wave per row, lane = action; a workgroup's eight half-waves walk the chunk's rows.
// softmax with k_actor_head's max subtraction, p = (1 - eps) s + eps / A, adv = K7's row on (p, q, mask, action), w = sum(mask) / A,
// the row's term adv log p[c] w, and dlogits[a] = -(adv w / B) (1 - eps) s[c] ([a == c] - s[a]) / p[c].  An action outside [0, A) gives NaN.
__global__ void __launch_bounds__(256)
k_actor_loss(const float* __restrict__ logits, const float* __restrict__ q, const uint8_t* __restrict__ mask, const int32_t* __restrict__ action,
             int64_t B, int A, float eps, const float* __restrict__ eps_dev, double* __restrict__ part, float* __restrict__ adv,
             float* __restrict__ probs, float* __restrict__ dlogits) {
  __shared__ float term[HC];
  const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5;
  const bool on = lane < A;
  const int la = on ? lane : 0;
  const float e = eps_dev ? *eps_dev : eps;
#pragma unroll 1
  for (int r = hw; r < HC; r += 8) {
    const int64_t b = (int64_t)blockIdx.x * HC + r, bc = b < B ? b : 0;
    const float lv = logits[bc * A + la], qr = q[bc * A + la], mr = (float)mask[bc * A + la];
    const int c = action[bc];
    const bool c_ok = c >= 0 && c < A;
    const int cc = c_ok ? c : 0;
    const float l = on ? lv : -INFINITY, qv = on ? qr : 0.f, m = on ? mr : 0.f;
    float mx = l;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 32));
    const float ex = on ? expf(l - mx) : 0.f;
    float sum = ex, msum = m;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) { sum += __shfl_xor(sum, o, 32); msum += __shfl_xor(msum, o, 32); }
    const float s = ex / sum;
    const float p = (1.f - e) * s + e / (float)A;
    float pn;
    const float base = ippm_coma_baseline(on, on ? p : 0.f, qv, m, pn);
    const float qc = __shfl(qv, cc, 32), sc = __shfl(s, cc, 32), pc = __shfl(p, cc, 32);
    const float ad = c_ok ? qc - base : __builtin_nanf("");
    const float w = msum / (float)A;
    const float coef = -(ad * w / (float)B) * (1.f - e) * sc / pc;
    if (b < B && on) {
      dlogits[b * A + lane] = coef * ((lane == cc ? 1.f : 0.f) - s);
      if (probs) probs[b * A + lane] = p;
    }
    if (lane == 0) {
      if (b < B) adv[b] = ad;
      term[r] = b < B ? ad * logf(pc) * w : 0.f;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int j = 0; j < HC; ++j) sum += (double)term[j];
    part[blockIdx.x] = sum;
  }
}

// loss = sign * (the chunks' sums added in chunk order) / B, rounded to float32 once
__global__ void k_head_loss_sum(const double* __restrict__ part, int64_t chunks, int64_t B, double sign, float* __restrict__ loss) {
  if (threadIdx.x || blockIdx.x) return;
  double s = 0.0;
  for (int64_t ch = 0; ch < chunks; ++ch) s += part[ch];
  *loss = (float)(sign * s / (double)B);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
bool hd_shape_ok(const char* who, int64_t batch, int32_t n_actions) { return lt_batch_ok(who, batch) && ai_actions_ok(who, n_actions); }

bool hd_args_ok(const char* who, std::initializer_list<const void*> required, std::initializer_list<const void*> aligned, int64_t batch,
                int32_t n_actions) {
  return lt_args_ok(who, required, [&] { return hd_shape_ok(who, batch, n_actions); }, aligned, "the tensors and the scratch");
}

unsigned hd_tiles(int64_t batch) { return (unsigned)((batch + HT_M - 1) / HT_M); }

}  // namespace

extern "C" int ippm_head_scratch_bytes(int64_t batch, int32_t n_actions, int64_t* bytes) {
  if (!bytes) { ippm_set_error("ippm_head_scratch_bytes: null argument"); return -1; }
  if (!hd_shape_ok("ippm_head_scratch_bytes", batch, n_actions)) return -1;
  *bytes = HeadScratch::bytes(batch);
  return 0;
}

extern "C" int ippm_head_forward(const float* h, const float* fc1_w, const float* fc1_b, const float* fc3_w, const float* fc3_b, int64_t batch,
                                 int32_t n_actions, void* scratch, float* a1, float* logits, void* stream) {
  const char* who = "ippm_head_forward";
  if (!hd_args_ok(who, {h, fc1_w, fc1_b, fc3_w, fc3_b, a1, logits}, {h, fc1_w, fc1_b, fc3_w, a1, scratch}, batch, n_actions)) return -1;
  hipLaunchKernelGGL(k_head_rows<true>, dim3(hd_tiles(batch)), dim3(256), 0, S_(stream), h, fc1_w, fc1_b, fc3_w, fc3_b, a1, logits, batch,
                     (int)n_actions);
  IPPM_LAUNCH_CHECK("head_forward");
  return 0;
}

extern "C" int ippm_critic_loss(const float* q, const int32_t* action, const float* td, int64_t batch, int32_t n_actions, void* scratch,
                                float* loss, float* q_chosen, float* dq, void* stream) {
  const char* who = "ippm_critic_loss";
  if (!hd_args_ok(who, {q, action, td, scratch, loss, q_chosen, dq}, {scratch}, batch, n_actions)) return -1;
  const HeadScratch sc(scratch, batch);
  const int64_t chunks = lt_ceil_div(batch, HC);
  hipLaunchKernelGGL(k_critic_loss, dim3((unsigned)chunks), dim3(HC), 0, S_(stream), q, action, td, batch, (int)n_actions, sc.loss, q_chosen, dq);
  hipLaunchKernelGGL(k_head_loss_sum, dim3(1), dim3(64), 0, S_(stream), static_cast<const double*>(sc.loss), chunks, batch, 1.0, loss);
  IPPM_LAUNCH_CHECK("critic_loss");
  return 0;
}

extern "C" int ippm_actor_loss(const float* logits, const float* q_values, const uint8_t* mask, const int32_t* action, int64_t batch,
                               int32_t n_actions, float eps, const float* eps_dev, void* scratch, float* loss, float* adv, float* probs,
                               float* dlogits, void* stream) {
  const char* who = "ippm_actor_loss";
  if (!hd_args_ok(who, {logits, q_values, mask, action, scratch, loss, adv, dlogits}, {scratch}, batch, n_actions)) return -1;
  const HeadScratch sc(scratch, batch);
  const int64_t chunks = lt_ceil_div(batch, HC);
  hipLaunchKernelGGL(k_actor_loss, dim3((unsigned)chunks), dim3(256), 0, S_(stream), logits, q_values, mask, action, batch, (int)n_actions, eps,
                     eps_dev, sc.loss, adv, probs, dlogits);
  hipLaunchKernelGGL(k_head_loss_sum, dim3(1), dim3(64), 0, S_(stream), static_cast<const double*>(sc.loss), chunks, batch, -1.0, loss);
  IPPM_LAUNCH_CHECK("actor_loss");
  return 0;
}

extern "C" int ippm_head_backward(const float* dlogits, const float* scale_dev, const float* a1, const float* h, const float* fc1_w,
                                  const float* fc3_w, int64_t batch, int32_t n_actions, void* scratch, float* gh, float* g_fc1_w, float* g_fc1_b,
                                  float* g_fc3_w, float* g_fc3_b, void* stream) {
  const char* who = "ippm_head_backward";
  if (!hd_args_ok(who, {dlogits, a1, h, fc1_w, fc3_w, scratch, gh, g_fc1_w, g_fc1_b, g_fc3_w, g_fc3_b}, {a1, h, fc1_w, fc3_w, scratch, gh}, batch,
                  n_actions))
    return -1;
  const HeadScratch sc(scratch, batch);
  const int64_t chunks = lt_ceil_div(batch, HC);
  const int A = n_actions;
  hipStream_t s = S_(stream);
  hipLaunchKernelGGL(k_head_gz1, dim3(hd_tiles(batch)), dim3(256), 0, s, dlogits, scale_dev, fc3_w, a1, sc.gz1, batch, A);
  hipLaunchKernelGGL(k_head_rows<false>, dim3(hd_tiles(batch)), dim3(256), 0, s, static_cast<const float*>(sc.gz1), fc1_w,
                     static_cast<const float*>(nullptr), static_cast<const float*>(nullptr), static_cast<const float*>(nullptr), gh,
                     static_cast<float*>(nullptr), batch, A);
  hipLaunchKernelGGL(k_head_wgrad, dim3((unsigned)(chunks * 5)), dim3(256), 0, s, static_cast<const float*>(sc.gz1), dlogits, scale_dev, h, a1,
                     sc.partial, batch, A);
  hipLaunchKernelGGL(k_head_wgrad_sum, dim3((unsigned)((HP_FLOATS + 255) / 256)), dim3(256), 0, s, static_cast<const float*>(sc.partial), chunks, A,
                     g_fc1_w, g_fc1_b, g_fc3_w, g_fc3_b);
  IPPM_LAUNCH_CHECK("head_backward");
  return 0;
}
