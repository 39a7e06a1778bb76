// Native bf16 inference of the actor convnet (actor/network.py:10-96): conv 5x5 -> 4x4 -> 4x4 (11 -> 7 -> 4 -> 1), fc1, fc3, softmax,
// epsilon mix.  The trunk (pack, layer kernel, fc3's product) and the numerical contract are ippm_bf16_net.h's, shared with the critic
// (critic_infer.hip); the actor is its 7-plane instantiation plus k_actor_head: softmax and the epsilon mix, in float32.
#include "ippm_bf16_net.h"

namespace {

using AP = NetPack<IPPM_ACTOR_PLANES>;

// ---- fc3 + softmax + epsilon mix: one wavefront per 16 samples --------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_actor_head(const uint16_t* __restrict__ h, const uint16_t* __restrict__ w, const float* __restrict__ bias, int64_t B, int A, float eps,
             const float* __restrict__ eps_dev, float* __restrict__ probs, float* __restrict__ logits) {
  __shared__ float L[16][AI_NPAD + 1];
  const int lane = threadIdx.x;
  const int64_t m = (int64_t)blockIdx.x * 16 + lane;
  ai_fc3_tile(h, w, bias, (int64_t)blockIdx.x * 16, B, L);
  if (lane < 16 && m < B) {
    const float e = eps_dev ? *eps_dev : eps;
    float mx = L[lane][0];
    for (int a = 1; a < A; ++a) mx = fmaxf(mx, L[lane][a]);
    float ex[AI_NPAD], s = 0.f;
#pragma unroll
    for (int a = 0; a < AI_NPAD; ++a) {
      ex[a] = a < A ? expf(L[lane][a] - mx) : 0.f;
      s += ex[a];
    }
    const float uni = e / (float)A;
#pragma unroll
    for (int a = 0; a < AI_NPAD; ++a)
      if (a < A) {
        probs[m * A + a] = (1.f - e) * (ex[a] / s) + uni;
        if (logits) logits[m * A + a] = L[lane][a];
      }
  }
}

}  // namespace

extern "C" int ippm_actor_pack_bytes(int32_t n_actions, int64_t* bytes) {
  return ai_pack_bytes<IPPM_ACTOR_PLANES>("ippm_actor_pack_bytes", n_actions, bytes);
}

extern "C" int ippm_actor_pack(const float* conv1_w, const float* conv1_b, const float* conv2_w, const float* conv2_b, const float* conv3_w,
                               const float* conv3_b, const float* fc1_w, const float* fc1_b, const float* fc3_w, const float* fc3_b,
                               int32_t n_actions, void* packed, void* stream) {
  const float* const p[10] = {conv1_w, conv1_b, conv2_w, conv2_b, conv3_w, conv3_b, fc1_w, fc1_b, fc3_w, fc3_b};
  return ai_pack<IPPM_ACTOR_PLANES>("ippm_actor_pack", p, n_actions, packed, stream);
}

extern "C" int ippm_actor_scratch_bytes(int64_t batch, int64_t* bytes) { return ai_scratch_bytes("ippm_actor_scratch_bytes", batch, bytes); }

extern "C" int ippm_actor_forward(const void* packed, const float* obs, int64_t batch, int32_t n_actions, float eps, const float* eps_dev,
                                  void* scratch, float* probs, float* logits, void* stream) {
  if (!packed || !obs || !scratch || !probs) { ippm_set_error("ippm_actor_forward: null argument"); return -1; }
  if (!ai_forward_args_ok("ippm_actor_forward", packed, scratch, batch, n_actions)) return -1;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint16_t* w = static_cast<const uint16_t*>(packed);
  const float* bias = reinterpret_cast<const float*>(static_cast<const char*>(packed) + AP::BIAS_BYTES);
  const int64_t S = batch < AI_SLICE ? batch : (int64_t)AI_SLICE;
  const NetScratch act(scratch, S);
  for (int64_t lo = 0; lo < batch; lo += S) {
    const int64_t nb = batch - lo < S ? batch - lo : S;
    ai_launch_trunk<IPPM_ACTOR_PLANES>(packed, obs + lo * (11 * 11 * IPPM_ACTOR_PLANES), nb, act, s);
    hipLaunchKernelGGL(k_actor_head, dim3((unsigned)((nb + 15) / 16)), dim3(64), 0, s, act.act4, w + AP::W5, bias + 1024, nb, (int)n_actions,
                       eps, eps_dev, probs + lo * n_actions, logits ? logits + lo * n_actions : nullptr);
  }
  IPPM_LAUNCH_CHECK("actor_forward");
  return 0;
}
