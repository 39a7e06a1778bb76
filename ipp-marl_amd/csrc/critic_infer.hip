// Native bf16 inference of the critic convnet (critic/network.py:12-47): the actor's trunk over the 12 planes of a critic state, fc3,
// no softmax.  The trunk (pack, layer kernel, fc3's product) and the numerical contract are ippm_bf16_net.h's, shared with the actor
// (actor_infer.hip); the critic is its 12-plane instantiation (conv1's K = 300, zero-padded to 320: 5 K steps; a kernel row is 60
// contiguous floats of the state, the next one 132 further on) plus k_critic_head: Q in float32 and the Q of a chosen action.
#include <cmath>

#include "ippm_bf16_net.h"

namespace {

using CP = NetPack<IPPM_CRITIC_PLANES>;

// ---- fc3 + the chosen action's Q: one wavefront per 16 samples ---------------------------------------------------------------------
// q (unless NULL) gets the 16 x A tile as contiguous floats; q_sel[b] (unless NULL) = q[b][action[b]], NaN for an action outside
// [0, A): nothing is read with such an index.
__global__ void __launch_bounds__(64)
k_critic_head(const uint16_t* __restrict__ h, const uint16_t* __restrict__ w, const float* __restrict__ bias, int64_t B, int A,
              const int32_t* __restrict__ action, float* __restrict__ q, float* __restrict__ q_sel) {
  __shared__ float L[16][AI_NPAD + 1];
  const int lane = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * 16;
  ai_fc3_tile(h, w, bias, b0, B, L);
  if (q) {
    const int rows = B - b0 < 16 ? (int)(B - b0) : 16;
    for (int i = lane; i < rows * A; i += 64) {
      const int r = i / A;
      q[b0 * A + i] = L[r][i - r * A];
    }
  }
  if (q_sel && lane < 16 && b0 + lane < B) {
    const int a = action[b0 + lane];
    q_sel[b0 + lane] = (a >= 0 && a < A) ? L[lane][a] : NAN;
  }
}

}  // namespace

extern "C" int ippm_critic_pack_bytes(int32_t n_actions, int64_t* bytes) {
  return ai_pack_bytes<IPPM_CRITIC_PLANES>("ippm_critic_pack_bytes", n_actions, bytes);
}

extern "C" int ippm_critic_pack(const float* conv1_w, const float* conv1_b, const float* conv2_w, const float* conv2_b, const float* conv3_w,
                                const float* conv3_b, const float* fc1_w, const float* fc1_b, const float* fc3_w, const float* fc3_b,
                                int32_t n_actions, void* packed, void* stream) {
  const float* const p[10] = {conv1_w, conv1_b, conv2_w, conv2_b, conv3_w, conv3_b, fc1_w, fc1_b, fc3_w, fc3_b};
  return ai_pack<IPPM_CRITIC_PLANES>("ippm_critic_pack", p, n_actions, packed, stream);
}

extern "C" int ippm_critic_scratch_bytes(int64_t batch, int64_t* bytes) { return ai_scratch_bytes("ippm_critic_scratch_bytes", batch, bytes); }

extern "C" int ippm_critic_forward(const void* packed, const float* state, int64_t batch, int32_t n_actions, const int32_t* action,
                                   void* scratch, float* q, float* q_sel, void* stream) {
  if (!packed || !state || !scratch) { ippm_set_error("ippm_critic_forward: null argument"); return -1; }
  if (!q && !q_sel) { ippm_set_error("ippm_critic_forward: q and q_sel are both NULL: nothing to compute"); return -1; }
  if (q_sel && !action) { ippm_set_error("ippm_critic_forward: q_sel needs action"); return -1; }
  if (!ai_forward_args_ok("ippm_critic_forward", packed, scratch, batch, n_actions)) return -1;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint16_t* w = static_cast<const uint16_t*>(packed);
  const float* bias = reinterpret_cast<const float*>(static_cast<const char*>(packed) + CP::BIAS_BYTES);
  const int64_t S = batch < AI_SLICE ? batch : (int64_t)AI_SLICE;
  const NetScratch act(scratch, S);
  for (int64_t lo = 0; lo < batch; lo += S) {
    const int64_t nb = batch - lo < S ? batch - lo : S;
    ai_launch_trunk<IPPM_CRITIC_PLANES>(packed, state + lo * (11 * 11 * IPPM_CRITIC_PLANES), nb, act, s);
    hipLaunchKernelGGL(k_critic_head, dim3((unsigned)((nb + 15) / 16)), dim3(64), 0, s, act.act4, w + CP::W5, bias + 1024, nb, (int)n_actions,
                       action ? action + lo : nullptr, q ? q + lo * n_actions : nullptr, q_sel ? q_sel + lo : nullptr);
  }
  IPPM_LAUNCH_CHECK("critic_forward");
  return 0;
}
