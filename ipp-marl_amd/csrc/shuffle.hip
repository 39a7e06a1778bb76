// The minibatch order of the COMA round as a pure function of (seed; round, data_pass): ippm_minibatch_permutation writes the permutation
// pi of [0, n) that the learners cut their minibatches from -- the one random stream of a training run that used to live in a generator's
// hidden state.
//
// pi is cycle-walking over a balanced Feistel network.  With k the bit length of n - 1 and h = max(1, ceil(k / 2)), E is a bijection of
// [0, 4^h) (two halves of h bits, IPPM_SHUFFLE_ROUNDS rounds whose round function is word 0 of one Philox4x32-10 call), and pi(i) is the
// first of E(i), E(E(i)), ... below n.  It exists because i < n lies on a cycle of E that returns to [0, n); 4^h < 4n for n >= 3, so a walk
// visits fewer than four points on average.
//
// One lane per i, a data-dependent loop, six Philox calls per visited point: ALU work only, one 8-byte store per lane, no LDS, no
// cooperation between lanes.  With team_prefix the rank pi(i) among the flying transitions is mapped to its buffer row by a binary search
// in the envs' prefix sums.
#include "ippm_internal.h"

namespace {

struct ShuffleArgs {
  const int64_t* round_dev;       // int64[1] read in place of `round`, or null
  const int32_t* team_prefix;     // int32[n_envs + 1] exclusive prefix sums of the envs' flying agents, or null
  int64_t* idx;
  int64_t round;
  uint32_t k0, k1;                // the seed's words
  uint32_t n;
  uint32_t h;                     // bits per half
  uint32_t data_pass;
  int32_t n_envs, n_agents;
};

__global__ void __launch_bounds__(256) k_minibatch_permutation(const ShuffleArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;       // (n < 2^31: the last workgroup's lanes stay below 2^32)
  if (i >= a.n) return;
  const uint64_t round = (uint64_t)(a.round_dev ? a.round_dev[0] : a.round);
  const uint32_t r_lo = (uint32_t)round, r_hi = (uint32_t)(round >> 32);
  const uint32_t h = a.h, mask = (1u << h) - 1u;            // h <= 16: a point of the domain fits 32 bits
  uint32_t x = i;
  do {
    uint32_t L = x >> h, R = x & mask;
#pragma unroll
    for (uint32_t r = 0; r < IPPM_SHUFFLE_ROUNDS; ++r) {
      const uint32_t f = ippm_philox(R, r_lo, ippm_stream_word(r, a.data_pass, IPPM_DOMAIN_SHUFFLE), r_hi, a.k0, a.k1).v[0] & mask;
      const uint32_t nr = L ^ f;
      L = R;
      R = nr;
    }
    x = (L << h) | R;
  } while (x >= a.n);
  int64_t row = (int64_t)x;
  if (a.team_prefix) {
    // rank x among the flying transitions -> (block, env, agent) -> row of a [blocks, n_envs, n_agents] buffer
    const int32_t F = a.team_prefix[a.n_envs];
    if (F < 1) {
      row = -1;      // no one flies: not a row of any buffer (the gather counts it as bad)
    } else {
      const uint32_t block = x / (uint32_t)F, s = x % (uint32_t)F;
      int lo = 0, hi = a.n_envs;                            // the env e with team_prefix[e] <= s < team_prefix[e + 1], lo <= e < hi
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)a.team_prefix[mid] <= s) lo = mid; else hi = mid;
      }
      const int64_t agent = (int64_t)s - a.team_prefix[lo];
      row = ((int64_t)block * a.n_envs + lo) * a.n_agents + agent;
    }
  }
  a.idx[i] = row;
}

}  // namespace

extern "C" int ippm_minibatch_permutation(uint64_t seed, int64_t round, const int64_t* round_dev, int32_t data_pass, int64_t n,
                                          const int32_t* team_prefix, int32_t n_envs, int32_t n_agents, int64_t* idx, void* stream) {
  const std::string who = "ippm_minibatch_permutation";
  if (!idx) { ippm_set_error(who + ": null argument (idx)"); return -1; }
  if (n < 1 || n >= ((int64_t)1 << 31)) { ippm_set_error(who + ": n must be in [1, 2^31)"); return -1; }
  if (data_pass < 0 || data_pass >= 65536) { ippm_set_error(who + ": data_pass must be in [0, 65536)"); return -1; }
  if (team_prefix && (n_envs < 1 || n_agents < 1)) {
    ippm_set_error(who + ": team_prefix needs n_envs and n_agents of at least 1");
    return -1;
  }
  if ((reinterpret_cast<uintptr_t>(idx) & 7) || (reinterpret_cast<uintptr_t>(round_dev) & 7) || (reinterpret_cast<uintptr_t>(team_prefix) & 3)) {
    ippm_set_error(who + ": idx and round_dev must be 8-byte aligned, team_prefix 4-byte aligned");
    return -1;
  }
  uint32_t k = 0;                                           // bit length of n - 1
  for (uint64_t v = (uint64_t)(n - 1); v; v >>= 1) ++k;
  const uint32_t h = k < 2 ? 1u : (k + 1) / 2;
  ShuffleArgs a = {round_dev, team_prefix, idx, round, (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), (uint32_t)n, h,
                   (uint32_t)data_pass, team_prefix ? n_envs : 0, team_prefix ? n_agents : 0};
  hipLaunchKernelGGL(k_minibatch_permutation, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S_(stream), a);
  IPPM_LAUNCH_CHECK("ippm_minibatch_permutation");
  return 0;
}
