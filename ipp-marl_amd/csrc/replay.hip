// The replay buffer of the COMA round (batch_memory.py: add / build_td_targets / the minibatch sampling of the learners), three launches
// where a tensor library issues one per array:
//   ippm_replay_store      a rollout step's transition into slot (w, t) of the five buffers [W,T,E,N,...] + the three return accumulators
//   ippm_td_lambda_buffer  K8 straight from buffer order (q_sel, rewards in; td, discounted return out, all [W,T,E,N])
//   ippm_replay_gather     a minibatch of the five training arrays by an int64 index list
//
// All three are plain data movement (the TD kernel: K8's arithmetic, ippm_td_lambda_at, at other strides); every element has one owner, no
// workgroup waits on another, and nothing is accumulated across lanes -- so what they write is what the one-array-at-a-time form writes, bit
// for bit (the accumulators: one float32 add per step).
//
// Alignment.  An observation row is 847 floats = 3388 bytes: rows, and slot bases whenever E*N is not a multiple of 4, are 4-byte aligned
// only.  rp_copy takes 16-byte accesses only where BOTH addresses are 16-byte aligned (state rows: 1452 floats = 363 x 16 bytes), dword
// accesses where both are 4-byte aligned, bytes otherwise (mask rows of n_actions bytes); lanes always walk consecutive elements, so a
// wavefront covers contiguous lines in every form.  The decision is uniform over a workgroup.
#include "ippm_internal.h"

namespace {

constexpr int RP_OBS = 11 * 11 * IPPM_ACTOR_PLANES;      // floats per observation row (847)
constexpr int RP_STATE = 11 * 11 * IPPM_CRITIC_PLANES;   // floats per state row (1452)
constexpr int RP_CHUNK = 16384;                          // bytes per workgroup of the store's copies: 256 lanes x 4 x 16 bytes
constexpr int RP_MAX_ACTIONS = 32;

// nbytes from src to dst by the 256 threads of a workgroup (src == nullptr: zeros)
__device__ __forceinline__ void rp_copy(void* dst, const void* src, size_t nbytes, int tid) {
  const uintptr_t both = reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src);   // (a null src constrains nothing)
  char* d = static_cast<char*>(dst);
  const char* s = static_cast<const char*>(src);
  size_t done = 0;
  if ((both & 15) == 0) {
    const size_t n16 = nbytes >> 4;
    for (size_t i = tid; i < n16; i += 256)
      reinterpret_cast<uint4*>(d)[i] = s ? reinterpret_cast<const uint4*>(s)[i] : make_uint4(0u, 0u, 0u, 0u);
    done = n16 << 4;
  }
  if ((both & 3) == 0) {
    const size_t n4 = (nbytes - done) >> 2;
    for (size_t i = tid; i < n4; i += 256)
      reinterpret_cast<uint32_t*>(d + done)[i] = s ? reinterpret_cast<const uint32_t*>(s + done)[i] : 0u;
    done += n4 << 2;
  }
  for (size_t i = done + tid; i < nbytes; i += 256) d[i] = s ? s[i] : (char)0;
}

struct StoreSeg {
  const char* src;
  char* dst;
  int64_t bytes;
  int32_t wg0;      // first workgroup of the segment
};

struct StoreArgs {
  StoreSeg seg[4];  // obs, state, action, mask: contiguous blocks of one slot
  int32_t n_seg;    // 4, or 0 (store = 0: the accumulators only)
  int32_t wg_acc;   // first workgroup of the rewards / accumulators
  const float* reward;          // [E,2]
  const float* agent_reward;    // [E,N,2] or null
  const int32_t* last_agent;    // [E] or null
  float* buf_reward;            // this slot's [E] (COMA) / [E,N] (DeepQ), or null
  float* ret;
  float* abs_ret;
  float* team_ret;
  int32_t E, N;
};

// Workgroups [0, wg_acc): RP_CHUNK bytes each of one of the four copies.  Workgroups from wg_acc on: one thread per env (COMA) or per
// (env, agent) (DeepQ) writes the slot's reward; the threads below E also advance the env's three accumulators, one float32 add each.
__global__ void __launch_bounds__(256) k_replay_store(const StoreArgs a) {
  const int tid = threadIdx.x;
  const int wg = (int)blockIdx.x;
  if (wg < a.wg_acc) {
    int si = 0;
    for (int i = 1; i < a.n_seg; ++i)
      if (wg >= a.seg[i].wg0) si = i;
    const StoreSeg s = a.seg[si];
    const int64_t off = (int64_t)(wg - s.wg0) * RP_CHUNK;
    const int64_t left = s.bytes - off;
    rp_copy(s.dst + off, s.src + off, (size_t)(left < RP_CHUNK ? left : RP_CHUNK), tid);
    return;
  }
  const int64_t i = (int64_t)(wg - a.wg_acc) * 256 + tid;
  const bool deepq = a.agent_reward != nullptr;
  if (a.buf_reward) {
    if (deepq) { if (i < (int64_t)a.E * a.N) a.buf_reward[i] = a.agent_reward[2 * i]; }
    else if (i < a.E) a.buf_reward[i] = a.reward[2 * i];
  }
  if (i < a.E) {
    const float team = a.reward[2 * i];
    float r0 = team, r1 = a.reward[2 * i + 1];
    if (deepq) {
      const int la = a.last_agent[i];
      const bool ok = la >= 0 && la < a.N;      // an agent outside the team: NaN into the returns, nothing read out of range
      r0 = ok ? a.agent_reward[2 * (i * a.N + la)] : __uint_as_float(0x7FC00000u);
      r1 = ok ? a.agent_reward[2 * (i * a.N + la) + 1] : __uint_as_float(0x7FC00000u);
    }
    a.ret[i] += r0;
    a.abs_ret[i] += r1;
    a.team_ret[i] += team;
  }
}

// One thread per (time step s = w*T + t, chain c = (e, n)), consecutive lanes on consecutive chains: in buffer order the chain is the fast
// index, so a wavefront's loads of step s' are one contiguous run for every s' of the walk.
__global__ void __launch_bounds__(256)
k_td_lambda_buffer(const float* __restrict__ reward, const float* __restrict__ q_sel, float* __restrict__ td, float* __restrict__ dr,
                   double gamma, double lam, int T, int len, int C, int N, int per_agent) {
  // (unsigned: C * len may be anything below 2^31, and the last workgroup's lanes count up to 255 past it)
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (unsigned)(C * len)) return;
  const int c = (int)(idx % (unsigned)C), t = (int)(idx / (unsigned)C);
  // rewards: [len, C] (one per agent) or [len, E] broadcast over the env's agents
  const float* r = per_agent ? reward + c : reward + c / N;
  const size_t rs = per_agent ? (size_t)C : (size_t)(C / N);
  float tdv, drv;
  ippm_td_lambda_at(r, rs, q_sel + c, (size_t)C, [T](int i) { return i % T == T - 1; }, t, len, gamma, lam, tdv, drv);
  td[idx] = tdv;
  dr[idx] = drv;
}

struct GatherArgs {
  const float* buf_state;
  const float* buf_obs;
  const int32_t* buf_action;
  const uint8_t* buf_mask;
  const float* buf_td;
  float* states;
  float* obs;
  int32_t* actions;
  uint8_t* masks;
  float* td;
  int32_t* bad;
  int64_t n;
  int32_t A;
};

// One workgroup per output row.  The index is range-checked here: a row outside [0, n) is written as zeros and counted.
__global__ void __launch_bounds__(256) k_replay_gather(const GatherArgs a, const int64_t* __restrict__ idx) {
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const int64_t i = idx[row];
  const bool ok = i >= 0 && i < a.n;
  const size_t src = ok ? (size_t)i : 0;
  if (a.states) rp_copy(a.states + row * RP_STATE, ok ? a.buf_state + src * RP_STATE : nullptr, RP_STATE * sizeof(float), tid);
  if (a.obs) rp_copy(a.obs + row * RP_OBS, ok ? a.buf_obs + src * RP_OBS : nullptr, RP_OBS * sizeof(float), tid);
  if (a.masks && tid < a.A) a.masks[row * a.A + tid] = ok ? a.buf_mask[src * a.A + tid] : (uint8_t)0;
  if (tid == 64 && a.actions) a.actions[row] = ok ? a.buf_action[src] : 0;
  if (tid == 128 && a.td) a.td[row] = ok ? a.buf_td[src] : 0.0f;
  if (tid == 192 && !ok && a.bad) atomicAdd(a.bad, 1);
}

bool rp_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace

extern "C" int ippm_replay_store(const float* obs, const float* state, const int32_t* action, const uint8_t* mask, const float* reward,
                                 const float* agent_reward, const int32_t* last_agent, int32_t n_envs, int32_t n_agents, int32_t n_actions,
                                 int32_t waves, int32_t steps, int32_t w, int32_t t, int32_t store, float* buf_obs, float* buf_state,
                                 int32_t* buf_action, uint8_t* buf_mask, float* buf_reward, float* ret, float* abs_ret, float* team_ret,
                                 void* stream) {
  const std::string who = "ippm_replay_store";
  if (!reward || !ret || !abs_ret || !team_ret) { ippm_set_error(who + ": null argument"); return -1; }
  if ((agent_reward != nullptr) != (last_agent != nullptr)) { ippm_set_error(who + ": agent_reward and last_agent go together"); return -1; }
  if (store && (!obs || !state || !action || !mask || !buf_obs || !buf_state || !buf_action || !buf_mask || !buf_reward)) {
    ippm_set_error(who + ": null argument (store != 0 needs the transition and the five buffers)");
    return -1;
  }
  if (n_envs < 1 || n_agents < 1 || (int64_t)n_envs * n_agents > (1 << 24)) {
    ippm_set_error(who + ": n_envs and n_agents must be positive, n_envs * n_agents at most 2^24");
    return -1;
  }
  if (n_actions < 1 || n_actions > RP_MAX_ACTIONS) { ippm_set_error(who + ": n_actions must be in [1, 32]"); return -1; }
  if (waves < 1 || steps < 1 || w < 0 || w >= waves || t < 0 || t >= steps) {
    ippm_set_error(who + ": the slot (w, t) must lie inside [0, waves) x [0, steps)");
    return -1;
  }
  if (!rp_aligned4(obs) || !rp_aligned4(state) || !rp_aligned4(action) || !rp_aligned4(reward) || !rp_aligned4(agent_reward) ||
      !rp_aligned4(last_agent) || !rp_aligned4(buf_obs) || !rp_aligned4(buf_state) || !rp_aligned4(buf_action) || !rp_aligned4(buf_reward) ||
      !rp_aligned4(ret) || !rp_aligned4(abs_ret) || !rp_aligned4(team_ret)) {
    ippm_set_error(who + ": float and int32 arrays must be 4-byte aligned");
    return -1;
  }
  const int64_t EN = (int64_t)n_envs * n_agents;
  const int64_t slot = (int64_t)w * steps + t;
  StoreArgs a = {};
  int32_t wg = 0;
  if (store) {
    const int64_t bytes[4] = {EN * RP_OBS * 4, EN * RP_STATE * 4, EN * 4, EN * n_actions};
    const char* src[4] = {reinterpret_cast<const char*>(obs), reinterpret_cast<const char*>(state), reinterpret_cast<const char*>(action),
                          reinterpret_cast<const char*>(mask)};
    char* dst[4] = {reinterpret_cast<char*>(buf_obs), reinterpret_cast<char*>(buf_state), reinterpret_cast<char*>(buf_action),
                    reinterpret_cast<char*>(buf_mask)};
    for (int i = 0; i < 4; ++i) {
      a.seg[i] = {src[i], dst[i] + slot * bytes[i], bytes[i], wg};
      wg += (int32_t)((bytes[i] + RP_CHUNK - 1) / RP_CHUNK);      // (at most 2^24 * 5808 / 16384 < 2^23 each)
    }
    a.n_seg = 4;
    a.buf_reward = buf_reward + slot * (agent_reward ? EN : (int64_t)n_envs);
  }
  a.wg_acc = wg;
  a.reward = reward; a.agent_reward = agent_reward; a.last_agent = last_agent;
  a.ret = ret; a.abs_ret = abs_ret; a.team_ret = team_ret;
  a.E = n_envs; a.N = n_agents;
  const int64_t threads = (store && agent_reward) ? EN : (int64_t)n_envs;
  wg += (int32_t)((threads + 255) / 256);
  hipLaunchKernelGGL(k_replay_store, dim3((unsigned)wg), dim3(256), 0, S_(stream), a);
  IPPM_LAUNCH_CHECK("ippm_replay_store");
  return 0;
}

extern "C" int ippm_td_lambda_buffer(ippm_ctx* ctx, const float* reward, int32_t reward_per_agent, const float* q_sel, float* td_target,
                                     float* disc_return, int32_t waves, int32_t steps, int32_t n_envs, int32_t n_agents, void* stream) {
  const std::string who = "ippm_td_lambda_buffer";
  if (!ctx || !reward || !q_sel || !td_target || !disc_return) { ippm_set_error(who + ": null argument"); return -1; }
  if (waves < 1 || steps < 1 || n_envs < 1 || n_agents < 1 || (int64_t)waves * steps * n_envs * n_agents >= ((int64_t)1 << 31)) {
    ippm_set_error(who + ": waves, steps, n_envs and n_agents must be positive, their product below 2^31");
    return -1;
  }
  const int C = n_envs * n_agents, len = waves * steps;
  const int total = C * len;
  hipLaunchKernelGGL(k_td_lambda_buffer, dim3((unsigned)(((int64_t)total + 255) / 256)), dim3(256), 0, S_(stream), reward, q_sel, td_target,
                     disc_return,
                     ctx->cfg.gamma, ctx->cfg.lambda_, (int)steps, len, C, (int)n_agents, reward_per_agent ? 1 : 0);
  IPPM_LAUNCH_CHECK("ippm_td_lambda_buffer");
  return 0;
}

extern "C" int ippm_replay_gather(const float* buf_state, const float* buf_obs, const int32_t* buf_action, const uint8_t* buf_mask,
                                  const float* buf_td, int64_t n, const int64_t* idx, int64_t count, int32_t n_actions, float* states,
                                  float* obs, int32_t* actions, uint8_t* masks, float* td, int32_t* bad, void* stream) {
  const std::string who = "ippm_replay_gather";
  if (!idx) { ippm_set_error(who + ": null argument (idx)"); return -1; }
  if ((states && !buf_state) || (obs && !buf_obs) || (actions && !buf_action) || (masks && !buf_mask) || (td && !buf_td)) {
    ippm_set_error(who + ": null argument (an output without its buffer)");
    return -1;
  }
  if (n < 1 || n > ((int64_t)1 << 40)) { ippm_set_error(who + ": n must be in [1, 2^40]"); return -1; }
  if (count < 0 || count > ((int64_t)1 << 31) - 1) { ippm_set_error(who + ": count must be in [0, 2^31)"); return -1; }
  if (n_actions < 1 || n_actions > RP_MAX_ACTIONS) { ippm_set_error(who + ": n_actions must be in [1, 32]"); return -1; }
  if (!rp_aligned4(buf_state) || !rp_aligned4(buf_obs) || !rp_aligned4(buf_action) || !rp_aligned4(buf_td) || !rp_aligned4(states) ||
      !rp_aligned4(obs) || !rp_aligned4(actions) || !rp_aligned4(td) || !rp_aligned4(bad) || (reinterpret_cast<uintptr_t>(idx) & 7)) {
    ippm_set_error(who + ": float and int32 arrays must be 4-byte aligned, idx 8-byte aligned");
    return -1;
  }
  if (count == 0) return 0;
  GatherArgs a = {buf_state, buf_obs, buf_action, buf_mask, buf_td, states, obs, actions, masks, td, bad, n, n_actions};
  hipLaunchKernelGGL(k_replay_gather, dim3((unsigned)count), dim3(256), 0, S_(stream), a, idx);
  IPPM_LAUNCH_CHECK("ippm_replay_gather");
  return 0;
}
