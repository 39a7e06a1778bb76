// The bf16 matrix-core tile that the inference layers (ippm_bf16_net.h) and the update kernels (conv4x4_train.hip, conv5x5_train.hip,
// head_train.hip) are built on -- everything that belongs to the tile and not to a network: the float32 -> bf16 conversions, the LDS
// geometry, one K step of MFMAs, the double-buffered K loop, the walk over a lane's outputs, the chunk-order sum of partial results and
// the argument checks of the host side.  Each piece is written ONCE here; what stays in a kernel is what is particular to it (row
// addressing, tap walk, transposition, which operand is rounded how).  Two kernels, k_conv4x4 and k_conv5x5, write the K loop and the
// store out themselves, because they measured slower on lt_k_loop and lt_for_outputs (profiles/r20/README.md): a change to either
// of those two pieces has to be made there as well.
//
// Workgroup tile: 128 rows (m) x 128 output channels (n), 4 wavefronts of 64 x 64 each, K in steps of 64 through LDS (rows padded by 16
// bytes: the 16-byte fragment reads of 16 rows then fall into 16 different bank groups).  The weights are the FIRST operand of
// mfma_f32_16x16x32_bf16, so a lane's 4 accumulator registers are 4 consecutive n of one m: one 8- or 16-byte store.
// Staging of a row-major operand: thread -> chunk column sc = tid & 7 (8 k) and the rows sr + 32 i, sr = tid >> 3.
//
// Everything here sits in an unnamed namespace: each translation unit that includes the header owns its instantiations.
#pragma once
#include <cstdint>
#include <initializer_list>
#include <string>

#include "ippm_internal.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- float32 -> bf16 ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint16_t ai_bf16(float x) {   // round to nearest even (NaN kept quiet)
  uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// ai_bf16(ippm_relu(x)) in one pass over the bits: NaN is kept by the test the conversion makes anyway, and what is left of the ReLU --
// everything with the sign bit set, -0 and -Inf included, becomes +0 -- is one integer max where ippm_relu's two compares and two selects
// in front of the conversion cost the layer kernel 1.3 % (profiles/r14/)
__device__ __forceinline__ uint16_t ai_relu_bf16(float x) {
  uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u = (uint32_t)max((int32_t)u, 0);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// two floats -> two bf16 in one word (the first in the low half), round to nearest even: gfx950's packed conversion, one instruction
// where ai_bf16 is six -- for the kernels whose staging converts far more elements per MFMA than the 256-channel layers do
__device__ __forceinline__ uint32_t lt_cvt2(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(floatx2{lo, hi}, bf16x2));
}

// Eight floats -> eight bf16 in four words, the two ways: lt_round8 on ai_bf16, lt_cvt8 on the packed conversion.  The two agree on every
// finite value and may differ in the payload bits of a NaN; tests/test_hip_bf16_operand_classes.py pins which entry point uses which.
__device__ __forceinline__ u32x4 lt_round8(const float (&v)[8]) {
  return u32x4{(uint32_t)ai_bf16(v[0]) | ((uint32_t)ai_bf16(v[1]) << 16), (uint32_t)ai_bf16(v[2]) | ((uint32_t)ai_bf16(v[3]) << 16),
               (uint32_t)ai_bf16(v[4]) | ((uint32_t)ai_bf16(v[5]) << 16), (uint32_t)ai_bf16(v[6]) | ((uint32_t)ai_bf16(v[7]) << 16)};
}
__device__ __forceinline__ u32x4 lt_cvt8(const float (&v)[8]) {
  return u32x4{lt_cvt2(v[0], v[1]), lt_cvt2(v[2], v[3]), lt_cvt2(v[4], v[5]), lt_cvt2(v[6], v[7])};
}

// ---- the tile ----------------------------------------------------------------------------------------------------------------------
constexpr int LT_M = 128, LT_N = 128, LT_K = 64, LT_LD = LT_K + 8;

template <int NT>
__device__ __forceinline__ void lt_zero(floatx4 (&acc)[4][NT]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) acc[a][b] = floatx4{0.f, 0.f, 0.f, 0.f};
}

// 8 k in a register -> this thread's chunk column of row sr + 32 i of a row-major LDS tile.  (The kernels store a row of each operand
// in turn, each as soon as it is rounded: LDS stores keep their order, and the first ones should leave early.)
__device__ __forceinline__ void lt_stage_row(uint16_t* S, int i, const u32x4& reg) {
  const int sc = threadIdx.x & 7, sr = threadIdx.x >> 3;
  *reinterpret_cast<u32x4*>(&S[(sr + 32 * i) * LT_LD + sc * 8]) = reg;
}

// One K step of a wavefront's 64 x 64 share of the tile: acc[n tile][m tile] += Ws[wn ..][k] * As[wm ..][k] over the LT_K k staged in LDS
// (rows of LT_LD elements; a lane reads row fr = lane & 15 of a 16-row fragment and the 8 k from fk = (lane >> 4) * 8 on).
__device__ __forceinline__ void lt_mma_step(const uint16_t* As, const uint16_t* Ws, int wm, int wn, int fr, int fk, floatx4 (&acc)[4][4]) {
#pragma unroll
  for (int kk = 0; kk < LT_K; kk += 32) {
    bf16x8 af[4], wf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      af[t] = *reinterpret_cast<const bf16x8*>(&As[(wm + t * 16 + fr) * LT_LD + kk + fk]);
      wf[t] = *reinterpret_cast<const bf16x8*>(&Ws[(wn + t * 16 + fr) * LT_LD + kk + fk]);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], af[mt], acc[nt][mt], 0, 0, 0);
  }
}

// What the K loop does about the operands of the step after the last one.  LT_GUARDED: a branch, uniform over the workgroup, skips the
// loads.  LT_RELOAD_LAST: the last step loads its own operands again -- no branch around the loads (k_actor_layer).
enum LtPrefetch { LT_GUARDED, LT_RELOAD_LAST };
// LT_ROLLED: #pragma unroll 1 -- for the kernels whose trip count is a compile-time constant (the loop would be unrolled whole) and for
// k_conv5x5_wgrad.  LT_FREE leaves the choice to the compiler, which doubles the body of k_conv4x4<false>.
enum LtUnroll { LT_FREE, LT_ROLLED };

// The double-buffered K loop: load(s) brings the operands of step s from memory into registers, stage() writes the loaded registers to
// LDS, mma() multiplies what is in LDS.  The loads of step s + 1 are issued before the MFMAs of step s and land while those run.
template <LtPrefetch PREFETCH, LtUnroll UNROLL, class Load, class Stage, class Mma>
__device__ __forceinline__ void lt_k_loop(int nsteps, Load load, Stage stage, Mma mma) {
  auto step = [&](int s) __attribute__((always_inline)) {
    __syncthreads();   // every wavefront has read the previous step's fragments: LDS may be overwritten
    stage();
    __syncthreads();   // every thread's share of this step is in LDS: the fragments may be read
    if (PREFETCH == LT_RELOAD_LAST) load(s + 1 < nsteps ? s + 1 : s);
    else if (s + 1 < nsteps) load(s + 1);
    mma();
  };
  load(0);
  if (UNROLL == LT_ROLLED) {
#pragma unroll 1
    for (int s = 0; s < nsteps; ++s) step(s);
  } else {
    for (int s = 0; s < nsteps; ++s) step(s);
  }
}

// The K loop around lt_mma_step, the MMA of every kernel whose wavefronts split M x N.
template <LtPrefetch PREFETCH, LtUnroll UNROLL, class Load, class Stage>
__device__ __forceinline__ void lt_k_loop(int nsteps, Load load, Stage stage, const uint16_t* As, const uint16_t* Ws, int wm, int wn,
                                          floatx4 (&acc)[4][4]) {
  const int lane = threadIdx.x & 63, fr = lane & 15, fk = (lane >> 4) * 8;
  lt_k_loop<PREFETCH, UNROLL>(nsteps, load, stage, [&]() __attribute__((always_inline)) { lt_mma_step(As, Ws, wm, wn, fr, fk, acc); });
}

// The lane's outputs of a wavefront's 4 x MT tiles of 16 x 16, tile(nt, mt) = D[n][m]: the lane holds m = lane & 15 and four consecutive n of
// every tile, the lane's quarter of the 16.  row(m) is asked once per m tile for what the kernel needs to know about its row m (where
// it is stored, as a rule); a row whose answer converts to false is skipped.  f(r, n, v): v = the outputs (m, n .. n + 3) of the row
// that r = row(m) stands for; m and n are counted within the wavefront's share.
template <int MT, class Tile, class Row, class F>
__device__ __forceinline__ void lt_for_tiles(Tile tile, Row row, F f) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const auto r = row(mt * 16 + (lane & 15));
    if (!r) continue;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const floatx4 d = tile(nt, mt);
      f(r, nt * 16 + (lane >> 4) * 4, float4{d[0], d[1], d[2], d[3]});
    }
  }
}

// ... of the accumulators acc[n tile][m tile] that the K loop leaves
template <int MT, class Row, class F>
__device__ __forceinline__ void lt_for_outputs(const floatx4 (&acc)[4][MT], Row row, F f) {
  lt_for_tiles<MT>([&](int nt, int mt) __attribute__((always_inline)) { return acc[nt][mt]; }, row, f);
}

// out[MAP::out(i)] = the partial sums partial[chunk][MAP::STRIDE] of element i added in chunk order; one thread per element, the reads
// coalesced.  The grid is exact: the elements summed are a multiple of 256.
template <class MAP>
__global__ void __launch_bounds__(256) k_partial_sum(const float* __restrict__ partial, int64_t chunks, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  float s = 0.f;
  for (int64_t k = 0; k < chunks; ++k) s += partial[k * MAP::STRIDE + i];
  out[MAP::out(i)] = s;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
constexpr int64_t LT_MAX_BATCH = (int64_t)1 << 24;          // keeps every grid below 2^31 workgroups

inline int64_t lt_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline bool lt_batch_ok(const char* who, int64_t batch) {
  if (batch < 1 || batch > LT_MAX_BATCH) { ippm_set_error(std::string(who) + ": batch must be in [1, 2^24]"); return false; }
  return true;
}

// what: names the pointers in the message; nulls among them are the optional ones
inline bool lt_aligned_ok(const char* who, std::initializer_list<const void*> aligned, const char* what) {
  for (const void* p : aligned)
    if (reinterpret_cast<uintptr_t>(p) & 15) { ippm_set_error(std::string(who) + ": " + what + " must be 16-byte aligned"); return false; }
  return true;
}

// required: may not be null; shape_ok(): the entry point's range checks, made between the two; aligned: must be 16-byte aligned
template <class ShapeOk>
bool lt_args_ok(const char* who, std::initializer_list<const void*> required, ShapeOk shape_ok, std::initializer_list<const void*> aligned,
                const char* what) {
  for (const void* p : required)
    if (!p) { ippm_set_error(std::string(who) + ": null argument"); return false; }
  return shape_ok() && lt_aligned_ok(who, aligned, what);
}

}  // namespace
