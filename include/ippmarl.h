/*
 * ippmarl.h -- C-ABI of libippmarl.so: the MI355X (gfx950) implementation of the ipp-marl hot path
 * (multi-UAV environment step + COMA target/advantage arithmetic).
 *
 * The reference (dmar-bonn/ipp-marl) is pure Python and has no FFI; its seam is the Python object
 * surface (COMAWrapper / Agent / Mapping / ...).  This header is the boundary a maintainer binds with
 * ctypes; every entry point cites the reference function(s) it replaces, paths
 * relative to marl_framework/.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; ippm_last_error() gives a thread-local message;
 *   - the CALLER owns every buffer: plain device pointers (e.g. torch.Tensor.data_ptr()), contiguous,
 *     dtype/shape as documented; the library allocates only the opaque context (a few KB of tables);
 *   - every launch takes an explicit hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     nothing synchronises except ippm_sync and ippm_read_counters;
 *   - no global mutable state: contexts are independent and may be used from different threads;
 *   - batched over E independent environments ("envs"); N = agents per env; maps are gx rows x gy columns,
 *     row index = x-cell, contiguous index = y-cell (reference: map[xl:xr, yu:yd], mappings.py:46-49).
 *
 * Array layouts (E envs, N agents, A actions, S = cfg.tile_stride)
 *   episode   int64  [E]          episode number of each env (seeds truth, start states, Philox streams)
 *   pos       int32  [E,N,3]      UAV position in metres (x,y,z)
 *   rect      int32  [E,N,4]      clipped footprint [yu,yd,xl,xr], half-open when sliced (cameras.py:62-77).  The kernels take any
 *                                 rectangle with 0 <= yu < yd <= gy-1, 0 <= xl < xr <= gx-1 (the reference's clip never includes the last
 *                                 row or column) that is no larger than the largest footprint, yd-yu <= 2 max radius_y, xr-xl <= 2 max
 *                                 radius_x (code tiles and K3's launch are sized from the radii): there is no minimum size, and nothing
 *                                 ties it to the lattice.  An EMPTY rectangle (yd <= yu or xr <= xl) is an agent without a footprint:
 *                                 K3 senses nothing for it and its message adds nothing to any map (with prior 0.5 that is the
 *                                 reference's update with an all-0.5 map2communicate; with any other prior the reference would still
 *                                 shift every cell by logit(prior) for such a message, the library does not: the reference has no agent
 *                                 without a footprint).  The carried region ws[.., 1..4] may be any box inside the grid.
 *   truth     uint8  [E,TRB]      ground truth, BIT-PACKED: cell (x,y) = bit (x*gy+y) of the env's little-endian bit string,
 *                                 TRB = ceil(gx*gy/32)*4 bytes (ceil((gx*gy+8)/32)*4 when gy is not a multiple of 4: one spare byte
 *                                 behind the last cell's, for the 2-byte loads of groups that straddle a byte)
 *   local     float  [E,N,gx,gy]  per-agent occupancy belief, stored as LOG-ODDS ln(p/(1-p)) (0 = prior 0.5);
 *   global    float  [E,gx,gy]    fused team belief, log-odds.  ippm_logodds_to_prob / ippm_prob_to_logodds
 *                                 convert at the boundary (DESIGN.md "log-odds storage")
 *   code      uint8  [E,N,TB]     last measurement of each agent, 1 bit per cell (1 = observed occupied).  With col =
 *                                 y-(yu & ~3): when gy % 4 == 0 the four grid-aligned cells of a lane group share the low
 *                                 nibble of byte [x-xl][col/4] (row stride S/4, TB = S*S/4); otherwise one byte per cell at
 *                                 [x-xl][col] (row stride S, TB = S*S).  (1-byte-per-cell planes cost K3 27 % of its time.)
 *   flips     uint8  same layout as code; 1 = this cell's observation is flipped (parity mode)
 *   comm      uint8  [E,N,N]      comm[e,i,j] = 1 iff agent i receives agent j's message (diagonal = 1)
 *   mask      uint8  [E,N,A]      action mask after boundary + collision masking
 *   action    int32  [E,N]
 *   ws        int32  [E,N+1,IPPM_WS_WORDS]  fusion workspace (deferred-clamp state + per-step op plan);
 *                                 initialised by ippm_reset_episode, otherwise opaque (zero-fill to start)
 *   sums      double [E,8]        reward accumulators: [0]=S1 [1]=S2 [2]=T (running weighted entropy of the
 *                                 global map), [3..5] scratch; initialised by ippm_reset_episode
 *   area      double [E,N+1,121]  11x11 area sums of every belief map (slot N = the global map): area[b] = sum over cells of
 *                                 (11*overlap of the cell with row bin bx) * (same for by) * p(cell); area / (gx*gy) is the
 *                                 exact area average cv2.resize(map, (11,11), INTER_AREA) of utils/state.py:22-41.  Optional
 *                                 (NULL = not tracked): when given, every kernel that writes a map keeps it up to date, so
 *                                 the K6 feature builders never stream a map; ippm_area_sums rebuilds it from scratch.
 */
#ifndef IPPMARL_H
#define IPPMARL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IPPM_VERSION 500
#define IPPM_MAX_AGENTS 16
#define IPPM_MAX_LATTICE 64 /* lattice points per horizontal axis */
#define IPPM_MAX_Z 8        /* altitude levels */
#define IPPM_MAX_ACTIONS 27
#define IPPM_FEAT 11        /* the reference's networks hard-wire an 11x11 lattice (actor/network.py:19-21) */
#define IPPM_ACTOR_PLANES 7
#define IPPM_CRITIC_PLANES 12
#define IPPM_WS_WORDS 160
/* ippm_plan_step flags */
#define IPPM_STEP_COMM 1   /* comm matrix + local-fusion plans */
#define IPPM_STEP_GLOBAL 2 /* global-fusion plan */
#define IPPM_STEP_MOVE 4   /* K1 mask/act/move (+ footprints of the new positions) */
#define IPPM_STEP_TILES 8  /* accepted, implied: the work list's form follows the context (ippm_tile_form), see ippm_plan_step */
/* fault[e] (ippm_plan_step): bits 0..n_agents-1 = agents whose action mask became empty at the LAST step; this bit is sticky
 * (the caller clears it): the env's tile work list did not fit its slice at some step (ruled out by the capacity bound of the
 * list; an env that shows it is no longer fused: ippm_fuse_step skips an overflowed list and counts it in counters.reserved[0]) */
#define IPPM_FAULT_WORK_OVERFLOW 0x40000000
#define IPPM_SENSE_REC_WORDS 8  /* words per agent of ippm_plan_step's rect_next / ippm_sense_step's rect_in */

/* Derived constants, computed on the host in float64 with the reference's expression order
 * (ippmarl/derived.py) and handed over as plain integers/floats. */
typedef struct ippm_config {
  int32_t n_agents;
  int32_t grid_x, grid_y;             /* cells: GridMap.x_dim / y_dim (grid_maps.py:17-50) */
  int32_t space_x, space_y, space_z;  /* lattice dims (state_space.py:16-21) */
  int32_t spacing, min_altitude;      /* metres */
  int32_t x_dim_m, y_dim_m;           /* world size in metres */
  int32_t n_actions;                  /* 4 | 6 | 9 | 27 (action_space.py) */
  int32_t budget;                     /* episode has budget+1 steps */
  int32_t env_seed;                   /* params.environment.seed (start states: state_space.py:29) */
  int32_t tile_stride;                /* S: row stride (and row count) of code/flips tiles, multiple of 4 */
  int32_t fix_range;                  /* 0: per-episode range from {0,15,25,100} (communication_log.py:22-31) */
  int32_t reserved0;
  int32_t centre_x[IPPM_MAX_LATTICE]; /* floor(x_m / res_x) per lattice index (cameras.py:66) */
  int32_t centre_y[IPPM_MAX_LATTICE]; /* floor(y_m / res_x) -- the reference uses res_x for both axes */
  int32_t radius_x[IPPM_MAX_Z];       /* floor(0.5*floor(2 z tan(ax/2)/res_x)) per altitude index */
  int32_t radius_y[IPPM_MAX_Z];
  float logit_meas[IPPM_MAX_Z][2];    /* ln(y/(1-y)) in float32 for y = f32(round(noise,3)), f32(round(1-noise,3)) */
  float meas_value[IPPM_MAX_Z][2];    /* the two measurement values themselves (simulations.py:47-51) */
  uint32_t flip_threshold[IPPM_MAX_Z];/* observation flipped iff philox word < threshold = floor(noise*2^32) */
  float prior;                        /* mapping.prior; != 0.5 takes the explicit full-grid path of the fusion (every message shifts
                                         every cell; chain in float64 registers, one rounding per fusion: maps and returns at 1e-5
                                         like the default) */
  float clip_lo, clip_hi;             /* 1e-4, 0.9999 (mappings.py:110-111, state.py:119-120) */
  float logit_prior;                  /* ln(prior/(1-prior)); 0 for the default prior 0.5 */
  float logit_clip;                   /* ln(clip_hi/(1-clip_hi)) = 9.21024...; the clip is symmetric in log-odds */
  float logit_weight_thr;             /* ln(0.501/0.499): class-weight thresholds of utils/state.py:65-66 */
  double comm_range;                  /* metres, used when fix_range != 0 */
  double failure_rate;                /* link drop probability (communication_log.py:46-54) */
  uint64_t philox_seed;               /* key of the counter-based RNG (production randomness) */
  double gamma, lambda_;              /* TD(lambda) (batch_memory.py:17-21) */
  float logit_noise[IPPM_MAX_Z];      /* ln((1-noise)/noise) from the float64 noise level: the hypothetical updates of
                                         IG_baseline.get_individual_ig use the scalar noise, not a float32 measurement */
  double logit_prior_f64;             /* ln(prior/(1-prior)) in float64, as mappings.py:114 forms it from the Python float: the
                                         whole-grid path of prior != 0.5 runs its chain in float64 registers */
} ippm_config;

typedef struct ippm_ctx ippm_ctx;

/* Algorithmic work counters accumulated by the kernels (cells, not bytes; see DESIGN.md for bytes/cell). */
typedef struct ippm_counters {
  uint64_t sense_cells;        /* K3: footprint cells sensed+updated */
  uint64_t fuse_local_cells;   /* K4: cells read+written by local fusion (union per map) */
  uint64_t fuse_local_ops;     /* K4: sum over (cell, op) pairs = the reference's per-neighbour work */
  uint64_t fuse_global_cells;  /* K5: cells read+written by global fusion */
  uint64_t fuse_global_ops;
  uint64_t feature_cells;      /* K6: map cells streamed by the feature builders */
  uint64_t reserved[2];        /* [0]: fusion launches that were handed a work list of the other form and skipped it (0 in a
                                  correct call sequence); [1]: cells whose value ippm_settle_clamps changed */
} ippm_counters;

const char* ippm_last_error(void);
int ippm_version(void);
int ippm_config_size(void); /* sizeof(ippm_config): lets a binding verify its struct mirror */

int ippm_ctx_create(const ippm_config* cfg, ippm_ctx** out);
int ippm_ctx_destroy(ippm_ctx* ctx);
int ippm_sync(ippm_ctx* ctx, void* stream);
int ippm_read_counters(ippm_ctx* ctx, ippm_counters* out, int reset, void* stream); /* synchronises */

/* Kernel timing (measurement aid; no reference counterpart).  While enabled, every launch of the classes below carries a
 * HIP event pair bound to the dispatch itself (hipExtLaunchKernelGGL start/stop events): their difference is the kernel's own
 * begin-to-end duration -- the figure rocprofv3's kernel trace reports -- with no barrier packet added to the stream.
 * ippm_read_kernel_times synchronises the stream and returns, for one class, the number of timed launches since the last
 * reset, their summed and shortest duration in microseconds and the name of the last kernel launched in that class as the
 * compiler (and rocprofv3) spells it.  At most IPPM_TIMED_CAP launches per class are held between two resetting reads. */
#define IPPM_T_SENSE 0        /* K3: k_sense_tiles / k_sense_update */
#define IPPM_T_FUSE 1         /* K4 + K5: k_fuse_rows */
#define IPPM_T_PLAN 2         /* k_plan_step */
#define IPPM_T_ACTOR_FEAT 3   /* K6 actor */
#define IPPM_T_CRITIC_FEAT 4  /* K6 critic */
#define IPPM_T_RESET 5        /* reset: scalars, truth split, prior fills */
#define IPPM_T_TERRAIN 6      /* random-field synthesis passes, the terrain library's draw */
#define IPPM_T_RESET_MAPS 7   /* ippm_reset_maps: box-limited prior fill + start-position sensing */
#define IPPM_T_AGENT_REWARD 8 /* ippm_agent_rewards: k_agent_rewards */
#define IPPM_TIMED_CLASSES 9
int ippm_kernel_timing(ippm_ctx* ctx, int32_t enable);
int ippm_read_kernel_times(ippm_ctx* ctx, int32_t cls, int32_t reset, int64_t* launches, double* total_us, double* min_us,
                           char* name, int32_t name_len, void* stream);

/* ---- reset ---------------------------------------------------------------------------------------
 * ippm_reset_episode replaces Mapping.__init__ -> Simulation.simulate_map -> gaussian_random_field
 * (mapping/simulations.py:34-40, mapping/ground_truths.py:42-56: half-plane split drawn from the legacy
 * MT19937 stream np.random.seed(episode)), AgentStateSpace.get_random_agent_state
 * (agent/state_space.py:28-51: RandomState(seed*episode*agent_id)), Mapping.init_priors
 * (mappings.py:126-132) and CommunicationLog.__init__'s per-episode range (communication_log.py:22-31).
 * The MT19937 streams are regenerated on the device, bit-exactly.
 * truth may be NULL (caller supplies its own terrain; split_pct int32 [E,2] is required otherwise);
 * local, global, comm_range_out (float [E]), sums and area may be NULL. */
int ippm_reset_episode(ippm_ctx* ctx, const int64_t* episode, int32_t* pos, uint8_t* truth, float* local,
                       float* global, int32_t* split_pct, float* comm_range_out, int32_t* ws, double* sums,
                       double* area, int32_t n_envs, void* stream);

/* Reset of the maps in one pass for the batched step (16-byte layout, grid_y >= 44): prior fill of local and global maps
 * (Mapping.init_priors, mappings.py:126-132) restricted to the bounding box of what the last episode wrote into each map (kept in
 * `ws` by ippm_plan_step; full != 0: whole maps -- first use, or after maps were written by other entry points), fused with the
 * start-position sensing of every agent (the stage-0 ippm_sense_update: agent.py:43-49 -> mappings.py:32-78), which needs
 * `truth` in place.  Call after ippm_reset_episode (with local = global = NULL there) and after the terrain is generated;
 * writes local, global, code, rect and the boxes in ws.  flips as for ippm_sense_update (NULL: Philox). */
int ippm_reset_maps(ippm_ctx* ctx, const int64_t* episode, const int32_t* pos, const uint8_t* truth, float* local, float* global,
                    const uint8_t* flips, uint8_t* code, int32_t* rect, int32_t* ws, int32_t full, int32_t n_envs, void* stream);

/* Elementwise conversions between the stored log-odds and the reference's probabilities (n floats). */
int ippm_logodds_to_prob(ippm_ctx* ctx, const float* src, float* dst, int64_t n, void* stream);
int ippm_prob_to_logodds(ippm_ctx* ctx, const float* src, float* dst, int64_t n, void* stream);
/* clip(p, 1e-4, 0.9999) of n stored log-odds in place: the full-grid input clip of one stand-alone fuse_map call. */
int ippm_clamp_logodds(ippm_ctx* ctx, float* maps, int64_t n, void* stream);

/* Plain device-to-device copy with 16-byte lane accesses (n_bytes and both pointers multiples of 16): the streaming-rate
 * denominator bench.py quotes next to the HBM peak. */
int ippm_stream_copy(ippm_ctx* ctx, const void* src, void* dst, int64_t n_bytes, void* stream);

/* ---- K2: Camera.project_field_of_view (sensors/cameras.py:46-79) ------------------------------------ */
int ippm_footprint(ippm_ctx* ctx, const int32_t* pos, int32_t* rect, int32_t* rect_unclipped, int32_t n_envs,
                   void* stream);

/* ---- K3: Mapping.update_grid_map = Simulation.get_measurement + apply_update ---------------------------
 * (mapping/mappings.py:32-78,109-124; mapping/simulations.py:42-65).  Computes rect from pos, senses the
 * footprint (flip source: explicit `flips` tiles, or Philox(seed; episode, agent, stage) when NULL),
 * Bayes-updates local[e,i] in place and stores the measurement codes.  `stage` = 0 for the start-position
 * sensing, t+1 for step t.  agent_sel >= 0 restricts the call to one agent (drop-in single-agent API). */
int ippm_sense_update(ippm_ctx* ctx, const int64_t* episode, const int32_t* pos, const uint8_t* truth,
                      float* local, const uint8_t* flips, uint8_t* code, int32_t* rect, int32_t* ws,
                      int32_t stage, int32_t agent_sel, int32_t n_envs, void* stream);
/* K3 as the closing kernel of a batched env step (COMAWrapper.steps' `agent.step` calls, coma_wrapper.py:106-134):
 * rect_in (optional) = the sense records ippm_plan_step wrote for the new positions, int32 [E,N,IPPM_SENSE_REC_WORDS] (the
 * footprint and the measurement constants of its altitude: saves the dependent pos -> lattice index -> centre-table and
 * pos -> altitude -> sensor-table loads in front of the map accesses; when given, the record's footprint is the one sensed and
 * published on every grid -- the z of `pos` must still be the record's altitude: the one-cell-per-lane kernel with area sums and
 * the next step's plans take the measurement's log-odds from it); area (optional) = tracked area sums, updated for local[e,i];
 * sums + reward (optional, together) = complete the reward of the step's global fusion in the same launch
 * (what ippm_reward_finalize does; the fusion of ippm_fuse_step leaves it open). */
int ippm_sense_step(ippm_ctx* ctx, const int64_t* episode, const int32_t* pos, const uint8_t* truth, float* local,
                    const uint8_t* flips, uint8_t* code, const int32_t* rect_in, int32_t* rect, int32_t* ws, double* area,
                    double* sums, float* reward, int32_t stage, int32_t agent_sel, int32_t n_envs, void* stream);

/* ---- comm: CommunicationLog.get_messages (agent/communication_log.py:39-58) ---------------------------
 * draws: float64 [E,N,N] replacing np.random.random_sample() per ordered pair, or NULL -> Philox.
 * comm_range: float [E] per-env range or NULL -> cfg.comm_range. */
int ippm_comm_matrix(ippm_ctx* ctx, const int64_t* episode, const int32_t* pos, const float* comm_range,
                     const double* draws, uint8_t* comm, int32_t t, int32_t n_envs, void* stream);

/* ---- K4: Agent.receive_messages -> Mapping.fuse_map(..., "local") (agent/agent.py:62-71,
 * mappings.py:82-89).  For each agent i the measurements of the received agents j != i are fused into
 * local[e,i] in ascending j; every map cell is read and written at most once.  `ws` carries the deferred
 * full-grid input clip of the reference (DESIGN.md "deferred clamp").  agent_sel >= 0 fuses only that agent's map
 * (drop-in Agent.receive_messages). */
int ippm_fuse_local(ippm_ctx* ctx, float* local, const uint8_t* code, const int32_t* rect, const int32_t* pos,
                    const uint8_t* comm, int32_t* ws, int32_t agent_sel, int32_t n_envs, void* stream);
/* ippm_comm_matrix followed by ippm_fuse_local for all agents, with the comm matrix and the fusion plans built by ONE
 * small kernel (both sit on the critical path of every step).  Same results as the two calls. */
int ippm_comm_fuse_local(ippm_ctx* ctx, const int64_t* episode, const int32_t* pos, const float* comm_range,
                         const double* draws, uint8_t* comm, float* local, const uint8_t* code, const int32_t* rect,
                         int32_t* ws, int32_t t, int32_t n_envs, void* stream);

/* ---- K5: Mapping.fuse_map(..., "global") + get_global_reward (mappings.py:91-102, utils/reward.py:11-82,
 * utils/state.py:53-121).  Fuses all N measurements into global[e] in place and returns
 * reward[e] = (22*S1/S2 - 0.5, 10*S1/(gx*gy) - 0.17) and sums[e] = (S1, S2, T, ...) in float64, where T is
 * the running weighted entropy of the map (initialised by ippm_reset_episode; re-seed it with
 * ippm_weighted_entropy if the map is replaced from outside). */
int ippm_fuse_global_reward(ippm_ctx* ctx, float* global, const uint8_t* code, const int32_t* rect,
                            const int32_t* pos, int32_t* ws, double* sums, float* reward, int32_t n_envs,
                            void* stream);

/* ---- the batched step in three launches: ippm_plan_step -> ippm_fuse_step -> ippm_sense_step ---------------------------
 * ippm_plan_step: everything of an env step that touches no map, one wavefront per env, selected by `flags`:
 *   IPPM_STEP_COMM    CommunicationLog.get_messages for every agent + the local-fusion plans (as ippm_comm_fuse_local)
 *   IPPM_STEP_GLOBAL  the global-fusion plan (as ippm_fuse_global_reward's first stage)
 *   IPPM_STEP_MOVE    K1 = ippm_mask_act_move on the same positions (comm and the plans see the pre-move ones); also writes
 *                     rect_next int32 [E,N,IPPM_SENSE_REC_WORDS] (optional) = the sense records of the NEW positions for
 *                     ippm_sense_step: {yu, yd, xl, xr (clipped footprint), float bits of the two measurement log-odds minus
 *                     logit(prior) at the new altitude, its flip threshold, 0}.
 *                     Only policies that do not depend on this step's observations (0 explicit, 1 uniform) can share a call
 *                     with COMM/GLOBAL; a learned policy calls MOVE separately after the actor.
 *   work (optional, int32 [ippm_work_words()]): with COMM | GLOBAL the kernel also lists the non-empty work items of the
 *   step's fusion for ippm_fuse_step, every env into its own slice (count + items: written, never accumulated, so there is
 *   nothing to clear between steps).  The list has one of two forms, chosen by the CONTEXT (ippm_tile_form()), not by the
 *   caller: self-contained one-trip tile items (rows x column interval x op mask, each at most 1024 cells) on contexts that have
 *   the tile form -- 16-byte lane groups (grid_y >= 44) and mapping.prior == 0.5 --, runs of rows of a plan's hull (map, run)
 *   on all others.  ippm_fuse_step of the same context consumes whichever form ippm_plan_step wrote, with or without area
 *   sums.  IPPM_STEP_TILES is accepted for source compatibility and changes nothing (it is implied where the tile form exists
 *   and ignored where it does not).  A list that a kernel cannot read (written by another context's plan step, or overflowed)
 *   fuses nothing and is counted in ippm_counters.reserved[0]; an overflowed one also sets IPPM_FAULT_WORK_OVERFLOW in fault[e].
 * ippm_fuse_step: K4 for all local maps and K5 for all global maps from the plans above, in one launch; keeps `area`
 *   (optional) up to date; leaves the reward sums open (ippm_sense_step or ippm_reward_finalize completes them).  With the
 *   `work` list of the same step's ippm_plan_step a fixed number of resident wavefronts strides over exactly the non-empty
 *   items; without it (NULL) the grid enumerates every (map, run) pair.
 * ippm_reward_finalize: reward[e] = (22*S1/S2 - 0.5, 10*S1/(gx*gy) - 0.17) from the accumulated sums (utils/reward.py:25-40). */
/* Mixed team sizes in one batch (BASELINE config 5: "mixed team sizes 2-16 UAVs").  The reference's team size is a per-run
 * parameter (coma_wrapper.py:25-26, missions/episode_generator.py:99-102); here env e of a batch may fly n_active[e] <= n_agents
 * UAVs: it then evolves exactly like a run of the reference with n_agents = n_active[e] (same episode number): agents
 * >= n_active[e] are heard by nobody, hear nobody, do not move, sense or publish, and the agent-id plane of the network inputs is
 * (i + 1) / n_active[e].  n_active: DEVICE int32 [n_envs], caller-owned, read at every launch of the batched step
 * (ippm_plan_step, ippm_sense_step, ippm_reset_maps, ippm_actor_features, ippm_critic_features; ippm_fuse_step does not read it:
 * it executes the plans ippm_plan_step wrote, and an agent that does not fly gets an EMPTY plan at every plan step, so team sizes
 * may change between any two steps); NULL (the default): every env flies n_agents.  Arrays keep their [E, n_agents, ...] strides;
 * rows of inactive agents are zero (observations, critic states) or not meaningful.
 * The single-purpose entry points (ippm_comm_matrix, ippm_fuse_local, ippm_ig_*, ...) do not look at it. */
int ippm_set_team_sizes(ippm_ctx* ctx, const int32_t* n_active);
/* Dirty slabs: what the episode reset has to fill.  Without them (the default) ippm_plan_step keeps ONE bounding box per map of
 * everything fusions and sensing wrote since the episode's reset (ws words 6-7, 14-15) and ippm_reset_maps writes the prior into that
 * box: 51 % of a local map and 87 % of the global one for 38 % / 58 % written at BASELINE config 2.  With a registered slab array --
 * slabs: DEVICE int32 [ippm_dirty_slab_words(n_envs)] = [n_envs, n_agents + 1, 2, ceil(grid_x / 16)], caller-owned, any contents (the
 * next ippm_reset_maps with full = 1 initialises it) -- the plan kernel marks, per 16-row slab of a map, the column interval the step's
 * plans and sense records touch (fire-and-forget atomic min / max), and ippm_reset_maps fills every slab's own interval (42 % / 69 %) and
 * re-arms it with the new episode's start footprint.  Maps written by other entry points (ippm_sense_update, ippm_fuse_local, host
 * copies) are not tracked either way: pass full = 1 to the next ippm_reset_maps.  NULL: back to the boxes.  Measured (round 6,
 * BASELINE config 2): the marks cost the plan kernel 3.8 us per step and the fill gains nothing from its fewer bytes, so the Python
 * host registers a slab array only on request (IPPM_DIRTY_SLABS=1).  Mirrors nothing in the
 * reference (mapping/mappings.py:126-132 allocates fresh prior maps per episode). */
int ippm_dirty_slab_words(ippm_ctx* ctx, int32_t n_envs, int64_t* words);
int ippm_set_dirty_slabs(ippm_ctx* ctx, int32_t* slabs);
/* Clamp backlog: the deferred clamp's clips, paid only when a map is read.  A plan that takes messages puts clamp-only
 * ops ahead of its real ops (over the region the last fusion or left-behind footprints may have left out of range, and over the agent's
 * last footprint); the cells of those that no real op meets are loaded, clipped and stored although nothing needs the clipped value in
 * memory until somebody looks at the map: every later op and ippm_sense_step clip their input themselves, ippm_reset_maps discards the
 * cells, and their reward terms are exact zeros.  With a registered backlog --
 * backlog: DEVICE int32 [ippm_clamp_backlog_words(n_envs)], caller-owned, 16-byte aligned, ZEROED before the first use; per map the
 * bounding box of the clips it is owed and the exact list of the rectangles written unclamped since its last fusion (budget + 2 entries:
 * one footprint per step of an episode and the fusion's own rectangle) -- the planners keep that list, and ippm_plan_step with
 * IPPM_STEP_DEFER_CLAMPS (tile form only; ignored elsewhere and without a backlog) pushes no clamp-only op: the rectangles join the
 * owed box.  A plan step WITHOUT the flag pays everything owed as part of its own clamp ops (today's plans plus the box).
 * ippm_settle_clamps (one launch, an early exit for maps that owe nothing) clips every cell of a map's owed box that is not legitimately
 * unclamped at that moment, cell for cell what the undeferred plans would have left, and empties the box: call it before ANYTHING other
 * than ippm_plan_step / ippm_fuse_step / ippm_sense_step / the resets reads or writes `local` / `global` (read-back, features, area sums,
 * ippm_agent_rewards, scoring, the planners' candidate gains, captured graphs, ...).  Do not defer when area sums are tracked.  The resets
 * (ippm_reset_episode, ippm_reset_maps) empty the backlog of the maps they reset.  The list holds an episode: a caller that steps a map more
 * than budget + 1 times between resets settles and stops deferring at that point (past it the list overflows, plans fall back to the
 * undeferred path by themselves, but a box still owed then can no longer be settled exactly).  `rect` = the published footprints
 * (ippm_sense_step's), `ws` the workspace.  Cells changed by the settles are counted in ippm_counters.reserved[1].  NULL: no backlog (default). */
#define IPPM_STEP_DEFER_CLAMPS 16
int ippm_clamp_backlog_words(ippm_ctx* ctx, int32_t n_envs, int64_t* words);
int ippm_set_clamp_backlog(ippm_ctx* ctx, int32_t* backlog);
int ippm_settle_clamps(ippm_ctx* ctx, float* local, float* global, const int32_t* ws, const int32_t* rect, int32_t* backlog,
                       int32_t n_envs, void* stream);
/* Storage layout of the belief maps (`local`, `global` of every entry point of this context).  0 (the default): row-major, cell (x, y) at
 * float x * grid_y + y -- the reference's numpy layout (mapping/mappings.py:18-25).  1: TILE STORAGE -- 128-byte tiles of 4 rows x 8 cells, the
 * tiles in row-major order: cell (x, y) at float (x >> 2) * 4 grid_y + (y >> 3) * 32 + (x & 3) * 8 + (y & 7).  Same size, same values; every
 * entry point that takes maps reads and writes them in the context's layout (ippm_maps_relayout converts between the two), everything
 * else -- truth bits, code tiles, footprints, plans, area sums, features -- is unchanged.  A footprint then touches whole lines only, which
 * keeps its price however many maps a launch ranges over (DESIGN.md "tile storage").  Needs the tile form (ippm_tile_form) and grid_x % 4 ==
 * 0, grid_y % 8 == 0: rc -2 otherwise.  Set it BEFORE the maps are first written; switching with live maps needs ippm_maps_relayout. */
int ippm_set_map_layout(ippm_ctx* ctx, int32_t tiled);
int ippm_map_layout(ippm_ctx* ctx, int32_t* tiled);
/* 1 where the configuration can take tile storage AND it has been measured to pay for a batch of n_envs envs: the batch's maps take 2 GB or more and
 * footprint rows are at most 256 cells (row-major rows cost the more per cell the more maps a launch ranges over, whole lines keep their price: BASELINE
 * config 4's per-GPU shape -8 .. -16 % per env step, config 2's shape -7 % at 2048 envs and -15 % at 4096 but +3 % at its 1024, config 5's 1024 x 1024
 * grid +3 %) -- what the Python host's map_layout="auto" follows for envs WITHOUT tracked area sums.  The advice is about the env-only kernels
 * (area == NULL): with area sums tracked, a tile walk's lanes fall into a third as many area bins per instruction as a row walk's and their LDS atomics
 * queue up (K3 85 -> 190 us, fusion 198 -> 232 at 2048 envs of config 2's shape), so a training rollout keeps rows. */
int ippm_map_layout_advice(ippm_ctx* ctx, int32_t n_envs, int32_t* tiled);
/* n_maps maps of grid_x * grid_y floats from `src` to `dst` (src != dst): to_tiled = 1 row-major -> tile storage, 0 the other way
 * (whatever the context's own layout is). */
int ippm_maps_relayout(ippm_ctx* ctx, const float* src, float* dst, int32_t n_maps, int32_t to_tiled, void* stream);
int ippm_plan_step(ippm_ctx* ctx, const int64_t* episode, int32_t* pos, const float* comm_range, const double* draws,
                   uint8_t* comm, const int32_t* rect, int32_t* ws, int32_t t, int32_t flags, const float* probs,
                   const int32_t* action_in, int32_t policy, uint8_t* mask, int32_t* action, int32_t* fault,
                   int32_t* rect_next, int32_t* work, int32_t n_envs, void* stream);
int ippm_fuse_step(ippm_ctx* ctx, float* local, float* global, const uint8_t* code, int32_t* ws, double* sums, double* area,
                   const int32_t* work, int32_t n_envs, void* stream);
int ippm_work_words(ippm_ctx* ctx, int32_t n_envs, int64_t* words); /* length of `work` in int32 words for n_envs envs */
int ippm_tile_form(ippm_ctx* ctx, int32_t* yes); /* 1: this configuration has the tile form (IPPM_STEP_TILES) */
int ippm_reward_finalize(ippm_ctx* ctx, double* sums, float* reward, int32_t n_envs, void* stream);

/* ---- DeepQ per-agent information-gain rewards (coma_wrapper.py:113-133 with mission type "DeepQ"; utils/reward.py:11-82,
 * utils/state.py:53-121, mappings.py:109-124).  For every agent i of env e: the reward of fusing ONLY agent i's fresh measurement
 * m_i into the global map K of this step, get_global_reward(K, K (+) m_i):
 *   S1_i = sum over cells of w(K (+) m_i) (H(K) - H(K (+) m_i)),  S2_i = sum of w(K (+) m_i) H(K) = T + sum (w(K (+) m_i) - w(K)) H(K)
 * with T = sums[e][2], the running weighted entropy of K, and agent_reward[e,i] = (22 S1_i/S2_i - 0.5, 10 S1_i/(gx*gy) - 0.17).
 * K (+) m_i clips every cell of K and adds the measurement's log-odds minus logit(prior): with prior 0.5 only agent i's footprint
 * differs from K, with any other prior every cell shifts (the kernel then walks the whole grid).
 *   global   float [E,gx,gy] in the context's map layout: K, read only;
 *   code     the measurement codes K3 wrote for the new positions;
 *   rect     int32 [E,N,IPPM_SENSE_REC_WORDS]: the sense records of the new footprints (ippm_plan_step's rect_next: footprint
 *            words 0-3, float bits of the two measurement log-odds minus logit(prior) in words 4-5);
 *   sums     double [E,8] after the step's reward was completed (reads [e][2] = T(K));
 *   agent_sums   double [E,N,2] = (S1_i, S2_i), optional (NULL);  agent_reward float [E,N,2] = (relative, absolute).
 * Agents that do not fly (ippm_set_team_sizes) get 0 in both outputs.  Writes nothing else.
 * Call after ippm_sense_step(sums, reward) of the batched step (or, one env at a time, after the last agent's sensing and the
 * reward of ippm_fuse_global_reward) and before the next fusion writes K or the codes. */
int ippm_agent_rewards(ippm_ctx* ctx, const float* global, const uint8_t* code, const int32_t* rect, const double* sums,
                       double* agent_sums, float* agent_reward, int32_t n_envs, void* stream);

/* Full-grid weighted entropy sum(w(p) H(p)) per map (utils/state.py:53-121, "reward" mode); n_maps maps of
 * gx*gy floats; out float64 [n_maps].  truth != NULL: weights from ground truth ("eval" mode), map m uses
 * truth[m / maps_per_truth]. */
int ippm_weighted_entropy(ippm_ctx* ctx, const float* maps, const uint8_t* truth, int32_t maps_per_truth,
                          double* out, int32_t n_maps, void* stream);

/* get_global_reward on two explicit maps (utils/reward.py:11-82): sums float64 [n_maps,2] = (S1,S2);
 * reward float [n_maps,2] = (relative, absolute) or NULL. */
int ippm_reward_from_maps(ippm_ctx* ctx, const float* before, const float* after, double* sums, float* reward,
                          int32_t n_maps, void* stream);

/* ---- K1: AgentActionSpace.get_action_mask + apply_collision_mask + ActorNetwork.do_eps_exploration +
 * action_to_position (agent/action_space.py:25-589, actor/network.py:90-96, coma_wrapper.py:97-104).
 * Sequential over the agents of an env (agent i is masked against the already-moved j < i).
 * policy: 0 = explicit `action_in`; 1 = uniform over the valid mask (Philox); 2 = sample from
 * probs*mask (Philox, "train"); 3 = argmax of probs*mask ("eval").  probs float [E,N,A] (policy 2/3).
 * fault[e] != 0 when an agent's mask became empty (the reference's torch.multinomial raises there): bit i = agent i, this step's
 * bits replace the last step's (IPPM_FAULT_WORK_OVERFLOW is kept). */
/* AgentActionSpace.get_action_mask (mask_in == NULL) / apply_collision_mask (mask_in = the mask to refine) for a batch
 * of single agents: pos int32 [B,3]; others int32 [B,max_others,3] = positions of already-moved agents, n_others
 * int32 [B] (NULL: none); masks uint8 [B,A] (agent/action_space.py:25-196,309-589). */
int ippm_action_mask(ippm_ctx* ctx, const int32_t* pos, const int32_t* others, const int32_t* n_others,
                     int32_t max_others, const uint8_t* mask_in, uint8_t* mask_out, int32_t* next_pos, int32_t batch,
                     void* stream); /* next_pos int32 [B,A,3] or NULL: action_to_position for every action */

int ippm_mask_act_move(ippm_ctx* ctx, const int64_t* episode, int32_t* pos, const float* probs,
                       const int32_t* action_in, int32_t policy, int32_t t, uint8_t* mask, int32_t* action,
                       int32_t* fault, int32_t n_envs, void* stream);

/* ---- K6: network inputs (actor/transformations.py:14-176, critic/transformations.py:17-132,
 * utils/state.py:22-41).  obs float [E,N,11,11,7]; state float [E,N,11,11,12].
 * The maps enter through their area sums `area` double [E,N+1,121] (tracked by the map kernels, or rebuilt by
 * ippm_area_sums): the feature builders never stream a map.
 * ippm_actor_features must run after the local fusion of step t (uses the fused local maps' sums, the published
 * measurements/rects/positions and comm); ippm_critic_features after the global fusion and K1 of step t with
 * pos_pre = the pre-move positions.
 * ippm_area_sums: area slots of n_maps log-odds maps from scratch (a streaming pass: 16-byte loads, 2 rows in flight);
 *   map m belongs to env m / maps_per_env, slot slot0 + m % maps_per_env (local maps: maps_per_env = N, slot0 = 0; global
 *   maps: maps_per_env = 1, slot0 = N).
 * ippm_area_resize: cv2.resize(src, (11,11), INTER_AREA) of n_arrays plain float arrays [rows,cols] -> dst float
 *   [n_arrays,11,11]; scratch double [n_arrays,121]. */
int ippm_actor_features(ippm_ctx* ctx, const double* area, const uint8_t* code, const int32_t* rect,
                        const int32_t* pos, const uint8_t* comm, int32_t t, float* obs, int32_t n_envs,
                        void* stream);
int ippm_critic_features(ippm_ctx* ctx, const double* area, const int32_t* rect, const int32_t* pos_pre,
                         const int32_t* action, const float* obs, float* state, int32_t n_envs, void* stream);
int ippm_area_sums(ippm_ctx* ctx, const float* maps, double* area, int32_t n_maps, int32_t maps_per_env, int32_t slot0,
                   void* stream);
int ippm_area_resize(ippm_ctx* ctx, const float* src, int32_t rows, int32_t cols, float* dst, double* scratch,
                     int32_t n_arrays, void* stream);
/* calculate_w_entropy on n explicit probabilities (utils/state.py:53-121): grid = clip(p, 1e-4, 0.9999), se = H(grid),
 * weightings = class weight of `target` (NULL: of p itself -- "reward"/"actor"/"global"; the ground truth for "eval"),
 * w_entropy = weightings * se.  Every output may be NULL. */
int ippm_entropy_maps(ippm_ctx* ctx, const float* prob, const float* target, float* w_entropy, float* weightings,
                      float* se, float* grid, int64_t n, void* stream);

/* ---- K7: COMA counterfactual advantage (actor/learner.py:55-95).  probs/q float [B,A], mask uint8 [B,A],
 * action int32 [B] -> advantage float [B], pi_tilde float [B,A] (may be NULL).  batch <= 0: returns 0, launches nothing and
 * writes nothing. */
int ippm_coma_advantage(ippm_ctx* ctx, const float* probs, const float* q, const uint8_t* mask,
                        const int32_t* action, float* advantage, float* pi_tilde, int32_t batch, void* stream);

/* col2im of the input gradient of a stride-1, unpadded kernel x kernel convolution evaluated as a GEMM (the learners' conv2:
 * actor/network.py:19-21, critic/network.py:21-23; MIOpen's float32 backward-data kernel runs it at a third of the forward's
 * rate).  cols float [batch*out_h*out_w, kernel*kernel*channels] (tap-major, channel-minor) -> grad_x float
 * [batch, out_h+kernel-1, out_w+kernel-1, channels] (channels-last).  No context needed. */
int ippm_col2im_nhwc(const float* cols, float* grad_x, int32_t batch, int32_t out_h, int32_t out_w, int32_t kernel,
                     int32_t channels, void* stream);

/* activation(conv(x)) of the learners' convnets (actor/network.py:72-80, critic/network.py:33-41) with the convolution run
 * bias-free by the library: y = max(x + bias, 0) IN PLACE on channels-last rows x float [rows, channels]; and its backward
 * pass grad_x = grad_y * (y > 0), grad_bias[c] += sum over rows of grad_x[., c] (grad_bias must be zeroed by the caller).
 * channels % 4 == 0 and channels / 4 divides 256; 16-byte aligned buffers.  No context needed. */
int ippm_bias_relu_nhwc(float* x, const float* bias, int64_t rows, int32_t channels, void* stream);
int ippm_bias_relu_backward_nhwc(const float* grad_y, const float* y, float* grad_x, float* grad_bias, int64_t rows,
                                 int32_t channels, void* stream);

/* ---- native bf16 inference of the actor (actor/network.py:10-96): conv 5x5 -> 4x4 -> 4x4, fc1, fc3, softmax, epsilon mix, all on
 * the matrix cores of gfx950.  No context needed.  Numerical contract: the input and the weights of every layer are rounded to bf16
 * (nearest even), products accumulate in float32, the float32 bias is added to the accumulator, ReLU, and the activation is rounded to
 * bf16 once, at the store; logits, softmax and (1 - eps) * softmax + eps / n_actions are float32.  Deterministic (fixed K order, no
 * atomics, no split-K): a sample's outputs are the same bits alone, at any position of any batch, and from run to run.
 *   ippm_actor_pack_bytes    size of the packed weight blob (n_actions in [1, 32]).
 *   ippm_actor_pack          one kernel: the float32 parameters in PyTorch's layouts (conv*_w [O,C,kh,kw], fc*_w [O,I]; fc2 is unused by
 *                            the network) -> packed (16-byte aligned): bf16 [O][K] per layer with K tap-major, channel-minor (conv1's
 *                            K = 175 zero-padded to 192, fc3's rows zero-padded to 32; conv3 is the plain product over conv2's output
 *                            flattened in (H, W, C) order), then the float32 biases.  Cheap and capturable: repack after every update.
 *   ippm_actor_scratch_bytes size of the caller-owned scratch for batches up to `batch` (bf16 channels-last activations; the forward
 *                            walks larger batches in slices of 4096 samples, so the scratch stays below 141 MB).
 *   ippm_actor_forward       obs float [batch,11,11,7] (what ippm_actor_features writes) -> probs float [batch,n_actions] and, unless
 *                            NULL, logits float [batch,n_actions].  eps_dev (device float, may be NULL: use eps) is read by the kernel, for
 *                            callers that record the launch into a graph.  Any batch >= 1; every output element is written; the scratch
 *                            needs no initialisation.  No host synchronisation, no allocation, launches on `stream` only. */
int ippm_actor_pack_bytes(int32_t n_actions, int64_t* bytes);
int ippm_actor_pack(const float* conv1_w, const float* conv1_b, const float* conv2_w, const float* conv2_b, const float* conv3_w,
                    const float* conv3_b, const float* fc1_w, const float* fc1_b, const float* fc3_w, const float* fc3_b,
                    int32_t n_actions, void* packed, void* stream);
int ippm_actor_scratch_bytes(int64_t batch, int64_t* bytes);
int ippm_actor_forward(const void* packed, const float* obs, int64_t batch, int32_t n_actions, float eps, const float* eps_dev,
                       void* scratch, float* probs, float* logits, void* stream);

/* ---- native bf16 inference of the critic (critic/network.py:12-47): the actor's trunk over the 12 planes of a critic state and fc3,
 * in the actor's kernels and under the actor's numerical contract word for word (bf16 inputs and weights, float32 accumulation and bias,
 * ReLU, one bf16 rounding at the store, fixed K order); Q is float32.  No softmax: the log_softmax over the batch that the reference's
 * critic also returns is a logged metric and is not computed here.  No context needed.
 *   ippm_critic_pack_bytes    size of the packed weight blob (n_actions in [1, 32]).
 *   ippm_critic_pack          as ippm_actor_pack, for conv1_w [256,12,5,5]: conv1's K = 300 zero-padded to 320.
 *   ippm_critic_scratch_bytes size of the caller-owned scratch for batches up to `batch` (slices of 4096 samples, as the actor's).
 *   ippm_critic_forward       state float [batch,11,11,12] (what ippm_critic_features writes) -> q float [batch,n_actions] unless NULL,
 *                             and, when action (int32 [batch]) and q_sel are given, q_sel[b] = q[b][action[b]] (float [batch]); an action
 *                             outside [0, n_actions) gives NaN in q_sel[b] and reads nothing out of range.  An error when q and q_sel
 *                             are both NULL, or q_sel is given without action.  Any batch >= 1; every output element is written; the
 *                             scratch needs no initialisation.  No host synchronisation, no allocation, launches on `stream` only. */
int ippm_critic_pack_bytes(int32_t n_actions, int64_t* bytes);
int ippm_critic_pack(const float* conv1_w, const float* conv1_b, const float* conv2_w, const float* conv2_b, const float* conv3_w,
                     const float* conv3_b, const float* fc1_w, const float* fc1_b, const float* fc3_w, const float* fc3_b,
                     int32_t n_actions, void* packed, void* stream);
int ippm_critic_scratch_bytes(int64_t batch, int64_t* bytes);
int ippm_critic_forward(const void* packed, const float* state, int64_t batch, int32_t n_actions, const int32_t* action, void* scratch,
                        float* q, float* q_sel, void* stream);

/* ---- conv2 of the learners' convnets on the bf16 matrix cores, for the COMA update (actor/network.py:19-28, critic/network.py): the
 * stride-1, unpadded 4x4 convolution with 256 input and 256 output channels, forward and both gradients, over channels-last float32
 * tensors: x [batch,ih,iw,256] with 4 <= ih, iw <= 11, y and gy [batch,ih-3,iw-3,256], w and gw in PyTorch's contiguous [256,256,4,4].
 * Numerical contract: every operand tensor (x, w, gy) is rounded to bf16 (nearest even) on its way in, products accumulate in float32
 * on mfma_f32_16x16x32_bf16, outputs are float32 and not rounded again; bias-free.  Deterministic: no float atomics, every output
 * element has one owner and a fixed summation order; forward and input gradient of a sample do not depend on the batch around it, the
 * weight gradient depends on the inputs and the batch size only (not on the device, the grid or the scratch's previous content).
 *   ippm_conv4x4_bf16_scratch_bytes  size of the caller-owned scratch for `batch`: the two bf16 weight packs (4 MiB), then the weight
 *                                    gradient's float32 partial sums, 4 MiB per chunk of IPPM_CONV4X4_WGRAD_CHUNK samples.  Forward and
 *                                    input gradient use the packs only.  Needs no initialisation; every call repacks what it reads.
 *   ippm_conv4x4_bf16_forward        y[b,oy,ox,o] = sum over ty,tx,c of x[b,oy+ty,ox+tx,c] * w[o,c,ty,tx].
 *   ippm_conv4x4_bf16_grad_input     gx[b,iy,ix,c] = sum over the taps (ty,tx) with (iy-ty, ix-tx) inside the output, and over o, of
 *                                    gy[b,iy-ty,ix-tx,o] * w[o,c,ty,tx]: a gather, every element of gx is written once.
 *   ippm_conv4x4_bf16_grad_weight    gw[o,c,ty,tx] = sum over b,oy,ox of gy[b,oy,ox,o] * x[b,oy+ty,ox+tx,c]: per-chunk partial sums in the
 *                                    scratch, added in chunk order by a second kernel.
 * -1 with ippm_last_error set for a null pointer, batch outside [1, 2^24], ih or iw outside [4, 11], a scratch or tensor that is not
 * 16-byte aligned; nothing is launched then.  No context needed, no host synchronisation, no allocation, launches on `stream` only. */
#define IPPM_CONV4X4_WGRAD_CHUNK 256
int ippm_conv4x4_bf16_scratch_bytes(int64_t batch, int32_t ih, int32_t iw, int64_t* bytes);
int ippm_conv4x4_bf16_forward(const float* x, const float* w, int64_t batch, int32_t ih, int32_t iw, void* scratch, float* y, void* stream);
int ippm_conv4x4_bf16_grad_input(const float* gy, const float* w, int64_t batch, int32_t ih, int32_t iw, void* scratch, float* gx,
                                 void* stream);
int ippm_conv4x4_bf16_grad_weight(const float* gy, const float* x, int64_t batch, int32_t ih, int32_t iw, void* scratch, float* gw,
                                  void* stream);

/* ---- conv1 of the COMA update on the bf16 matrix cores (csrc/conv5x5_train.hip): the stride-1, unpadded 5x5 convolution from `planes`
 * (7: actor, 12: critic) input planes of an 11x11 map to 256 channels of a 7x7 map, over channels-last float32 tensors: x [B,11,11,planes],
 * y and gy [B,7,7,256]; w and gw in PyTorch's [256,planes,5,5].  The contract of the 4x4 family above, word for word: every operand tensor
 * (x, w, gy) is rounded to bf16 (nearest even) on its way into LDS, products accumulate in float32 on mfma_f32_16x16x32_bf16, outputs are
 * float32 and not rounded again.  K = 25 * planes is zero-padded to a multiple of 64 (175 -> 192, 300 -> 320); the padded columns are
 * zeros, never memory.  Deterministic: no float atomics, every output element has one owner and a fixed summation order; a sample's
 * forward does not depend on the batch around it, the weight gradient depends on the inputs and the batch size only (not on the device,
 * the grid or the scratch's previous content).  No input gradient: the layer's input is data.
 *   ippm_conv5x5_bf16_scratch_bytes  size of the caller-owned scratch for `batch`: the bf16 weight pack (256 x padded K), then the weight
 *                                    gradient's float32 partial sums (256 x padded K per chunk of IPPM_CONV5X5_WGRAD_CHUNK samples).  The
 *                                    forward uses the pack only.  Needs no initialisation; every call writes what it reads.
 *   ippm_conv5x5_bf16_forward        y[b,oy,ox,o] = sum over ty,tx,c of x[b,oy+ty,ox+tx,c] * w[o,c,ty,tx]; with `bias` (float [256])
 *                                    non-null, y = max(that + bias[o], 0) at the store: the float32 bits of ippm_bias_relu_nhwc run
 *                                    on the bias-free output.
 *   ippm_conv5x5_bf16_grad_weight    gw[o,c,ty,tx] = sum over b,oy,ox of gy[b,oy,ox,o] * x[b,oy+ty,ox+tx,c]: per-chunk partial sums in the
 *                                    scratch, added in chunk order by a second kernel.
 * -1 with ippm_last_error set for a null pointer (but `bias`), batch outside [1, 2^24], planes other than 7 or 12, a scratch or tensor
 * that is not 16-byte aligned; nothing is launched then.  No context needed, no host synchronisation, no allocation, launches on
 * `stream` only. */
#define IPPM_CONV5X5_WGRAD_CHUNK 64
int ippm_conv5x5_bf16_scratch_bytes(int64_t batch, int32_t planes, int64_t* bytes);
int ippm_conv5x5_bf16_forward(const float* x, const float* w, const float* bias, int64_t batch, int32_t planes, void* scratch, float* y,
                              void* stream);
int ippm_conv5x5_bf16_grad_weight(const float* gy, const float* x, int64_t batch, int32_t planes, void* scratch, float* gw, void* stream);

/* ---- the heads of the COMA update (csrc/head_train.hip): everything behind conv3 in a learner's forward-with-gradient pass -- fc1, ReLU,
 * fc3 (actor/network.py:81-88, critic/network.py:42-47), the loss (critic/learner.py:76-92; actor/learner.py:52-97) and the
 * gradients back to conv3's output h [batch,256] -- over float32 tensors in PyTorch's layouts: fc1_w [256,256], fc1_b [256], fc3_w
 * [n_actions,256], fc3_b [n_actions], n_actions in [1, 32]; a1, gh [batch,256]; logits, q, dlogits, probs [batch,n_actions].
 * Numerical contract, the 4x4 family's extended: both operands of the six products z1 = h W1^T, logits = a1 W3^T, ga1 = dlogits W3,
 * gh = gz1 W1, gW1 = gz1^T h, gW3 = dlogits^T a1 are rounded to bf16 (nearest even) on their way in, products accumulate in float32 on
 * mfma_f32_16x16x32_bf16, outputs are float32 and not rounded again.  Everything else is float32 on unrounded values: the bias adds,
 * a1 = relu(z1 + b1) with the NaN-passing ReLU of ippm_bias_relu_nhwc, gz1 = ga1 [a1 > 0], gb1 = sum_b gz1, gb3 = sum_b dlogits and the
 * losses' per-row arithmetic (the ONE sum over the batch that makes a loss is carried in double and rounded to float32 once).  Deterministic: no float atomics, every output element has one owner and a fixed summation order; a sample's a1, logits,
 * dlogits (times batch) and gh are the same bits alone and in any batch; the sums over the batch (gW1, gb1, gW3, gb3, the losses) are
 * per-chunk partial sums of IPPM_HEAD_WGRAD_CHUNK samples in the scratch, added in chunk order by a second kernel: they depend on the
 * inputs and the batch size only (not on the device, the grid or the scratch's previous content).
 *   ippm_head_scratch_bytes  size of the caller-owned scratch for `batch`: the losses' partial sums (a double per chunk, rounded up to 16
 *                            bytes: all the two loss entry points use), gz1 [batch,256], the gradients' partial sums (296 064 bytes per
 *                            chunk).  Needs no initialisation.
 *   ippm_head_forward        a1 = relu(h W1^T + b1), logits = a1 W3^T + b3: one kernel.  Uses no scratch (NULL is accepted).
 *   ippm_critic_loss         loss = mean_b (q[b,a_b] - td_b)^2 (float [1]); q_chosen[b] = q[b,a_b]; dq[b,a] = 2 (q[b,a_b] - td_b) / batch
 *                            at a = a_b and 0 elsewhere.  action int32 [batch]; one outside [0, n_actions) gives NaN in its row and in
 *                            the loss and reads nothing out of range.
 *   ippm_actor_loss          with s = softmax(logits) (the maximum subtracted, as ippm_actor_forward), p = (1 - eps) s + eps / n_actions
 *                            (eps_dev, a device float, wins over eps when non-NULL): adv = ippm_coma_advantage's arithmetic on (p, q_values,
 *                            mask, action), bit for bit; w_b = sum_a mask[b,a] / n_actions; loss = -mean_b adv_b log p[b,a_b] w_b;
 *                            dlogits[b,a] = -(adv_b w_b / batch) (1 - eps) s[b,c] ([a == c] - s[b,a]) / p[b,c], c = a_b (adv is not
 *                            differentiated).  mask uint8 [batch,n_actions]; probs (p) may be NULL.
 *   ippm_head_backward       from dlogits * scale (scale_dev: a device float, NULL = 1; the product is float32, before any rounding):
 *                            gh [batch,256] and the gradients of fc1_w, fc1_b, fc3_w, fc3_b in the parameters' layouts.  a1 is
 *                            ippm_head_forward's.
 * -1 with ippm_last_error set for a null pointer (but the optional ones), batch outside [1, 2^24], n_actions outside [1, 32], a
 * scratch, h, a1, gh, fc1_w, fc1_b or fc3_w that is not 16-byte aligned; nothing is launched then.  No context needed, no host
 * synchronisation, no allocation, launches on `stream` only. */
#define IPPM_HEAD_WGRAD_CHUNK 64
int ippm_head_scratch_bytes(int64_t batch, int32_t n_actions, int64_t* bytes);
int ippm_head_forward(const float* h, const float* fc1_w, const float* fc1_b, const float* fc3_w, const float* fc3_b, int64_t batch,
                      int32_t n_actions, void* scratch, float* a1, float* logits, void* stream);
int ippm_critic_loss(const float* q, const int32_t* action, const float* td, int64_t batch, int32_t n_actions, void* scratch, float* loss,
                     float* q_chosen, float* dq, void* stream);
int ippm_actor_loss(const float* logits, const float* q_values, const uint8_t* mask, const int32_t* action, int64_t batch,
                    int32_t n_actions, float eps, const float* eps_dev, void* scratch, float* loss, float* adv, float* probs,
                    float* dlogits, void* stream);
int ippm_head_backward(const float* dlogits, const float* scale_dev, const float* a1, const float* h, const float* fc1_w,
                       const float* fc3_w, int64_t batch, int32_t n_actions, void* scratch, float* gh, float* g_fc1_w, float* g_fc1_b,
                       float* g_fc3_w, float* g_fc3_b, void* stream);

/* ---- native Adam (csrc/optim.hip): the optimizer step of the learners (actor/learner.py:32, critic/learner.py:48: torch.optim.Adam(parameters,
 * lr) with its defaults -- betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad) for up to 16 float32 tensors in ONE kernel launch, which
 * can also clear the gradients and rewrite a network's bf16 inference pack from the stepped parameters.  No context needed.
 * Arithmetic contract (a contract of this library, not a promise to match any other implementation's bits).  Per step,
 * scalars in double:  b1p <- b1p * beta1;  b2p <- b2p * beta2 (one multiplication each, no pow);  step = float(lr / (1 - b1p));
 * rs = float(sqrt(1 - b2p));  w1 = float(1 - beta1);  w2 = float(1 - beta2);  B2 = float(beta2);  E = float(eps).  Per element, float32, every
 * operation rounded on its own in this order, nothing contracted into an FMA:
 *     m <- m + w1 (g - m);   v <- B2 v + w2 (g g);   den = sqrtf(v) / rs + E;   p <- p - step (m / den).
 * NaN and Inf propagate as IEEE arithmetic propagates them: a non-finite gradient element reaches its own p, m, v (and pack element) only.
 * Float32 subnormal operands are outside the contract.  Deterministic: every element has one owner, there are no float atomics.
 * The state blob is caller-owned, 16-byte aligned, ippm_adam_state_bytes long, and laid out as follows (a binding may hand out views):
 *     byte 0   int64  t        steps taken            byte 8   double b1p = beta1^t       byte 16  double b2p = beta2^t
 *     byte 24  uint32 ticket   0 between launches     bytes 28-63 padding
 *     byte 64  for tensor 0, 1, ... in turn: float m[numel], padded to a multiple of 4 floats, then float v[numel], padded likewise
 *              (so every span starts 16-byte aligned: tensor i's m is (numel_0' + ... + numel_{i-1}') * 8 bytes behind byte 64, numel' = numel
 *              rounded up to a multiple of 4, and its v follows numel_i' * 4 bytes later).
 *   ippm_adam_state_bytes  size of the blob for n_tensors in [1, 16] tensors of numel[i] in [1, 2^36] elements.
 *   ippm_adam_init         one kernel: t = 0, both powers 1, ticket 0, every moment (and the padding) 0, whatever the blob held.
 *   ippm_adam_step         one kernel, capturable: nothing the host passes changes from step to step -- the counters live in the blob and
 *                          advance inside the launch (the last workgroup to finish writes them; no workgroup waits on another), so a
 *                          recorded launch steps again at every replay.  params / grads: HOST arrays of n_tensors device pointers (they
 *                          travel as kernel arguments).  flags & IPPM_ADAM_ZERO_GRAD: the lane that read a gradient element stores +0.0f
 *                          there.  packed != NULL (16-byte aligned; pack_planes = 7 or 12, else both 0 / NULL): the tensors must be the ten
 *                          of a network in the order conv1.w, conv1.b, conv2.w, conv2.b, conv3.w, conv3.b, fc1.w, fc1.b, fc3.w, fc3.b with
 *                          the sizes of that network for n_actions in [1, 32], and the same launch rewrites EVERY byte of the pack:
 *                          afterwards it equals what ippm_actor_pack (7) / ippm_critic_pack (12) writes from the stepped parameters,
 *                          whatever it held before.
 * -1 with ippm_last_error set for a null pointer, n_tensors outside [1, 16], a numel outside [1, 2^36], a state or pack that is not 16-byte
 * aligned, lr or eps that is not finite or negative, a beta outside [0, 1), unknown flags, pack_planes other than 0, 7, 12, a pack without
 * pack_planes (or the reverse), a pack with n_tensors != 10, n_actions outside [1, 32] or sizes that are not that network's; nothing is
 * launched then.  No host synchronisation, no allocation, launches on `stream` only. */
#define IPPM_ADAM_ZERO_GRAD 1
#define IPPM_ADAM_MAX_TENSORS 16
int ippm_adam_state_bytes(const int64_t* numel, int32_t n_tensors, int64_t* bytes);
int ippm_adam_init(void* state, const int64_t* numel, int32_t n_tensors, void* stream);
int ippm_adam_step(void* state, float* const* params, float* const* grads, const int64_t* numel, int32_t n_tensors, double lr, double beta1,
                   double beta2, double eps, int32_t flags, int32_t pack_planes, int32_t n_actions, void* packed, void* stream);

/* ---- native training metrics (csrc/metrics.hip): the 32 scalars the reference logs per training step (coma_mission.py:208-424,
 * critic/learner.py:100-190, actor/learner.py:36-200), reduced on the device from the arrays a minibatch step has anyway.  A round of
 * n_minibatches minibatches ("slots") of `batch` rows and n_actions actions accumulates into a caller-owned blob; one closing launch
 * writes double out[IPPM_METRICS_SCALARS] on the device, in this order:
 *    0 critic loss mean            1 TD target mean      2 TD target std        3 chosen-Q mean       4 Q mean (post-step, all actions)
 *    5 Q min     6 Q std           7 explained variance (y_true = disc, y_pred = td)                 8 disc. return mean    9 ... std
 *   10 |disc - q_chosen| mean     11 ... std            12 "log probs according to critic"           13-18 critic gradient figures
 *   19 actor loss mean            20 advantage mean     21 advantage std       22 log p(chosen) mean  23 policy entropy
 *   24 KL figure                  25 "hidden state entropy"                    26-31 actor gradient figures
 * Definitions (quirks of the reference included): every std is the unbiased one over all rows of all slots (one element: NaN); 7 uses
 * population variances, and with a zero variance of disc it is 1 if the residual's variance is zero too, else 0; 12 is the mean over all
 * rows of q_new[b,a_b] - logsumexp_{b'} q_new[b',a_b], the log-softmax over the BATCH axis of each slot; 23 is the mean over rows of
 * -sum_a p log p (0 log 0 is NaN); 24 is (1 / (batch n_actions)) sum_{slot,b,a} p_old (log p_old - p_after), i.e. log(p_old / exp(p_after))
 * summed over the slots and averaged over (b, a); 25 is the mean over slots of the mean square of hidden0; a gradient figure is
 * (|g_w|_1 + |g_b|_1) / 2 for conv1, conv2, conv3, fc1, [fc2: always 0], fc3.  An action outside [0, n_actions) gives NaN in 12 and 22 and
 * reads nothing out of range.
 * Arithmetic contract: every element is converted to double first; log and exp are double.  A workgroup owns
 * IPPM_METRICS_CHUNK rows of one slot; within a chunk, lane values are reduced by one fixed tree (wavefront shuffles, then LDS); moments
 * travel as (n, sum, M2) and are merged by Chan's formula, a column's log-sum-exp as (max, sum exp(x - max)); the closing launch merges the
 * chunks of a slot in chunk order, then the slots in slot order.  No atomics, no workgroup waits on another.  Every call overwrites all
 * partials of its slot (grad_l1: of its net), so the blob needs no initialisation and `out` depends on the inputs, batch, n_actions and
 * n_minibatches only -- not on the order of the calls, the grid, or what the blob held.  NaN and Inf propagate to the scalars their element
 * enters, and to no other.
 *   ippm_metrics_bytes        size of the blob (16-byte aligned, caller-owned).
 *   ippm_metrics_critic       slot's critic arrays: loss float [1]; q_chosen (pre-step), td, disc float [batch]; q_new float
 *                             [batch,n_actions] (post-step); action int32 [batch].
 *   ippm_metrics_actor        slot's actor arrays: loss float [1]; adv float [batch]; probs float [batch,n_actions] (epsilon-mixed);
 *                             action int32 [batch]; hidden0 float [256], the conv features of the slot's first sample.
 *   ippm_metrics_actor_after  the KL figure's terms of a slot: probs_old as given to ippm_metrics_actor, probs_after the updated actor's.
 *   ippm_metrics_grad_l1      the L1 norms of a net's ten gradients (net 0: critic, 1: actor); grads: a HOST array of 10 device pointers in
 *                             the order of the Adam step's tensors (conv1.w, conv1.b, ... fc1.w, fc1.b, fc3.w, fc3.b); numel in [1, 2^36].
 *   ippm_metrics_finalize     one workgroup: everything above -> out.
 * -1 with ippm_last_error set for a null pointer, batch outside [2, 2^24] (at 1 the reference's squeeze() changes the softmax axis),
 * n_actions outside [2, 32], n_minibatches outside [1, 65536], a slot outside [0, n_minibatches), a net other than 0 or 1, n_tensors other
 * than 10, a blob that is not 16-byte aligned, an array that is not 4-byte aligned (out: 8); nothing is launched then.  No context needed, no
 * host synchronisation, no allocation; pointers and the slot travel by value, launches on `stream` only (capturable). */
#define IPPM_METRICS_SCALARS 32
#define IPPM_METRICS_CHUNK 256
int ippm_metrics_bytes(int32_t n_minibatches, int64_t batch, int32_t n_actions, int64_t* bytes);
int ippm_metrics_critic(void* acc, int32_t slot, int32_t n_minibatches, const float* loss, const float* q_chosen, const float* td,
                        const float* disc, const float* q_new, const int32_t* action, int64_t batch, int32_t n_actions, void* stream);
int ippm_metrics_actor(void* acc, int32_t slot, int32_t n_minibatches, const float* loss, const float* adv, const float* probs,
                       const int32_t* action, const float* hidden0, int64_t batch, int32_t n_actions, void* stream);
int ippm_metrics_actor_after(void* acc, int32_t slot, int32_t n_minibatches, const float* probs_old, const float* probs_after,
                             int64_t batch, int32_t n_actions, void* stream);
int ippm_metrics_grad_l1(void* acc, int32_t net, float* const* grads, const int64_t* numel, int32_t n_tensors, void* stream);
int ippm_metrics_finalize(const void* acc, int32_t n_minibatches, int64_t batch, int32_t n_actions, double* out, void* stream);

/* ---- native rollout log (csrc/rollout_log.hip): the per-round return / reward statistics and the action and altitude histograms the
 * reference logs beside the training metrics (coma_mission.py:174-267).  One launch per rollout step writes that step's share of n_waves
 * waves of n_steps steps of n_envs envs into a caller-owned blob; one closing launch writes, on the device,
 *   double out[IPPM_ROLLOUT_SCALARS]: mean, population std (np.std), max, min of
 *      0-3  the absolute episode returns (n_waves n_envs values)
 *      4-7  the per-step relative rewards (n_waves n_steps n_envs values)
 *      8-11 the relative episode returns (n_waves n_envs values)
 *   int64 counts[IPPM_ROLLOUT_COUNTS]: [0,32) actions flown, [32,64) altitude levels reached, [64] entries counted in no bin.
 * Arithmetic contract: the step call stores both reward columns of its (wave, step) slot as float32.  An episode's
 * return is the float32 sum of its step rewards in step order, starting from the first one -- the adds of ippm_replay_store, bit for bit,
 * so max and min of a return series are exactly those of the accumulators.  Statistics convert every element to double first; a thread of
 * the closing workgroup forms the moments (n, sum, M2) of its max(2, ceil(episodes / 256) rounded up to even) consecutive episodes
 * (wave-major, then env) in two passes, and the 256 shares are merged by Chan's formula in one fixed tree (neighbours first over the
 * wavefront, then the four wavefronts in order): an order that depends on the sizes only.  One element gives std 0.  No floating-point
 * atomics, no workgroup waits on another.  NaN and Inf reach all four scalars of the series they enter (max and min keep a NaN as np.max
 * and np.min do) and no other series, and never the counts.  Counts are exact integers, one set of bins per workgroup of
 * IPPM_ROLLOUT_ROWS (env, agent) rows (wavefront ballots, then integer adds in LDS), summed in int64 by the closing launch: an agent a >=
 * n_active[e] is counted nowhere; a flying agent adds one entry per histogram: its action to bin action if that is in [0, n_actions), else
 * to counts[64]; its altitude to bin 32 + (z - min_altitude) / spacing if that is an integer in [0, n_levels), else to counts[64]; nothing
 * is read or written out of range for either.  Every step call overwrites everything of its slot that is ever read, so the blob needs no
 * initialisation and the result depends on the inputs and the sizes only -- not on the order of the calls, the grid, or what the blob
 * held.  The blob is wave-major and a slot's place does not depend on n_waves: the closing call may name fewer waves than the blob was
 * sized for and reduces those first waves.
 *   ippm_rollout_log_bytes     size of the blob (16-byte aligned, caller-owned).
 *   ippm_rollout_log_step      slot (wave, step): reward float [n_envs,2] = (relative, absolute); agent_reward NULL, or float
 *                              [n_envs,n_agents,2] (DeepQ): the row of the LAST FLYING agent (n_active[e] - 1, or n_agents - 1; clamped
 *                              into the table) replaces reward[e]; action int32 [n_envs,n_agents]; pos int32 [n_envs,n_agents,3] with
 *                              pos[..,2] the altitude in metres after the move; n_active NULL (all fly) or int32 [n_envs].
 *   ippm_rollout_log_finalize  one workgroup: the first n_waves waves -> out, counts.
 * -1 with ippm_last_error set for a null required pointer, n_envs outside [1, 2^20], n_agents outside [1, 32], n_actions outside [2, 32],
 * n_levels outside [1, 32], spacing < 1, n_steps or n_waves outside [1, 4096], wave or step out of range, a blob that is not 16-byte
 * aligned, an array that is not 4-byte aligned (out, counts: 8); nothing is launched then.  No context needed, no host synchronisation, no
 * allocation; pointers and indices travel by value, launches on `stream` only (capturable). */
#define IPPM_ROLLOUT_SCALARS 12
#define IPPM_ROLLOUT_COUNTS 65
#define IPPM_ROLLOUT_ROWS 1024
int ippm_rollout_log_bytes(int32_t n_waves, int32_t n_steps, int32_t n_envs, int32_t n_agents, int64_t* bytes);
int ippm_rollout_log_step(void* log, int32_t wave, int32_t step, int32_t n_waves, int32_t n_steps, const float* reward,
                          const float* agent_reward, const int32_t* action, const int32_t* pos, const int32_t* n_active, int32_t n_envs,
                          int32_t n_agents, int32_t n_actions, int32_t min_altitude, int32_t spacing, int32_t n_levels, void* stream);
int ippm_rollout_log_finalize(const void* log, int32_t n_waves, int32_t n_steps, int32_t n_envs, int32_t n_agents, double* out,
                              int64_t* counts, void* stream);

/* ---- K8: BatchMemory.build_td_targets (batch_memory.py:120-162) over `chains` independent transition
 * lists of length `len` (row-major [chains,len]): reward float, done uint8, q_sel float = target critic
 * Q(s_t)[a_t] -> td_target, discounted_return float.  chains <= 0 or len <= 0: returns 0, launches nothing and writes nothing;
 * chains * len above 2^31 - 1 is refused (-1 with a message, nothing launched). */
int ippm_td_lambda(ippm_ctx* ctx, const float* reward, const uint8_t* done, const float* q_sel, float* td_target,
                   float* disc_return, int32_t chains, int32_t len, void* stream);

/* ---- the replay buffer of the COMA round (csrc/replay.hip; batch_memory.py: add, build_td_targets, and the learners' minibatch
 * sampling): one launch per rollout step, one per target build, one per minibatch.  The buffers are contiguous arrays in BUFFER ORDER
 * [waves, steps, n_envs, n_agents, ...]: buf_obs float [.,11,11,7], buf_state float [.,11,11,12], buf_action int32 [.], buf_mask uint8
 * [.,n_actions], buf_reward float [waves,steps,n_envs] (one team reward per env) or [waves,steps,n_envs,n_agents] (one per agent).  Pure
 * data movement: every element has one owner, nothing is summed across lanes, so the results are the bytes that array-by-array copies and
 * index operations produce.  Float and int32 arrays need 4-byte alignment only (an observation row is 3388 bytes); 16-byte accesses are
 * taken where both addresses allow them, dword accesses otherwise.
 *   ippm_replay_store      one rollout step.  With store != 0 the transition -- obs [E,N,11,11,7], state [E,N,11,11,12], action [E,N],
 *                          mask [E,N,n_actions], what ippm_actor_features / ippm_critic_features / ippm_mask_act_move wrote -- is copied
 *                          into slot (w, t) of the five buffers, and in every case the three per-env accumulators (float [E]) advance by
 *                          exactly one float32 add each.  reward float [E,2] = (relative, absolute).  COMA form (agent_reward and
 *                          last_agent NULL): buf_reward[w,t,e] = reward[e,0]; ret[e] += reward[e,0]; abs_ret[e] += reward[e,1];
 *                          team_ret[e] += reward[e,0].  DeepQ form (agent_reward float [E,N,2], last_agent int32 [E], both given):
 *                          buf_reward[w,t,e,n] = agent_reward[e,n,0]; ret[e] += agent_reward[e,last_agent[e],0]; abs_ret[e] +=
 *                          agent_reward[e,last_agent[e],1]; team_ret[e] += reward[e,0]; a last_agent outside [0, n_agents) adds NaN to
 *                          ret and abs_ret and reads nothing out of range.  store == 0: the accumulators only (the transition and the
 *                          buffers may be NULL).  No context needed.
 *   ippm_td_lambda_buffer  ippm_td_lambda (K8) on one chain per (env, agent) over all waves in time order, read from and written in buffer
 *                          order without a transposed copy: q_sel float [waves,steps,n_envs,n_agents], reward as buf_reward above
 *                          (reward_per_agent = 0: [waves,steps,n_envs], broadcast over the env's agents; != 0: one per agent), step
 *                          steps - 1 of every wave is terminal -> td_target and disc_return float [waves,steps,n_envs,n_agents].  The
 *                          per-(chain, t) arithmetic is ippm_td_lambda's own code at other strides: the same bits as ippm_td_lambda on
 *                          the transposed arrays.
 *   ippm_replay_gather     a minibatch: for r < count, row idx[r] (int64, device) of the buffers seen as `n` rows -> row r of states
 *                          [count,11,11,12], obs [count,11,11,7], actions [count], masks [count,n_actions], td [count] (from buf_td float
 *                          [n], e.g. td_target above).  Any output may be NULL and is then skipped, and its buffer may be NULL too.  Every
 *                          index is checked in the kernel: a row with idx[r] outside [0, n) is written as zeros in every output and
 *                          counted into bad (int32 [1], optional, never reset here); nothing outside the buffers is read.  count == 0
 *                          launches nothing.  No context needed.
 * -1 with ippm_last_error set for a null required pointer, n_envs or n_agents < 1, n_actions outside [1, 32], a slot outside the buffers,
 * agent_reward without last_agent (or the reverse), a product of the dimensions of 2^31 or more (TD), n < 1, count < 0, a misaligned
 * array; nothing is launched then.  No host synchronisation, no allocation, launches on `stream` only. */
int ippm_replay_store(const float* obs, const float* state, const int32_t* action, const uint8_t* mask, const float* reward,
                      const float* agent_reward, const int32_t* last_agent, int32_t n_envs, int32_t n_agents, int32_t n_actions,
                      int32_t waves, int32_t steps, int32_t w, int32_t t, int32_t store, float* buf_obs, float* buf_state,
                      int32_t* buf_action, uint8_t* buf_mask, float* buf_reward, float* ret, float* abs_ret, float* team_ret,
                      void* stream);
int ippm_td_lambda_buffer(ippm_ctx* ctx, const float* reward, int32_t reward_per_agent, const float* q_sel, float* td_target,
                          float* disc_return, int32_t waves, int32_t steps, int32_t n_envs, int32_t n_agents, void* stream);
int ippm_replay_gather(const float* buf_state, const float* buf_obs, const int32_t* buf_action, const uint8_t* buf_mask,
                       const float* buf_td, int64_t n, const int64_t* idx, int64_t count, int32_t n_actions, float* states, float* obs,
                       int32_t* actions, uint8_t* masks, float* td, int32_t* bad, void* stream);

/* ---- the minibatch order of a training round, keyed like every other random stream ---------------------------------------------------
 * ippm_minibatch_permutation writes idx[i] = pi(i) for i < n (int64, device): the permutation of [0, n) that the learners cut the
 * minibatches of data pass `data_pass` of training round `round` from -- the `idx` of ippm_replay_gather.  A pure function of
 * (seed; round, data_pass, n): no generator state exists anywhere.  round_dev (device int64[1], or NULL) is read IN THE KERNEL in place of
 * `round` when given: a recorded round advances it on the device and needs no host-side argument.
 *   pi: cycle-walking over a balanced Feistel network keyed by Philox.  k = bit length of n - 1 (0 for n = 1), h = max(1, ceil(k / 2)),
 *   mask = 2^h - 1; the domain [0, 4^h) holds [0, n) and is smaller than 4n for n >= 3.  E(x): L = x >> h, R = x & mask; for r = 0 ..
 *   IPPM_SHUFFLE_ROUNDS - 1:  f = Philox4x32-10(counter = (R, round & 0xFFFFFFFF, stream word(agent = r, stage = data_pass, domain = 4),
 *   round >> 32), key = (seed & 0xFFFFFFFF, seed >> 32)).word0 & mask;  (L, R) <- (R, L ^ f);  E(x) = (L << h) | R.  The stream word is
 *   (agent & 0xFF) | (stage & 0xFFFF) << 8 | domain << 24, as for the env's streams (domains 0-3: flips, actions, comm, terrain).
 *   pi(i) = the first of E(i), E(E(i)), ... that is < n (i lies on a cycle of E that returns to [0, n)).  tests/shuffle_ref.py restates it.
 *   Mixed team sizes: team_prefix (device int32[n_envs + 1], or NULL) = the exclusive prefix sums of the envs' flying agents; then n counts
 *   FLYING transitions (a multiple of F = team_prefix[n_envs], read in the kernel), and rank q = pi(i) becomes a row of buffers in
 *   [blocks, n_envs, n_agents] order: block = q / F, s = q % F, e = the env with team_prefix[e] <= s < team_prefix[e + 1] (binary search),
 *   a = s - team_prefix[e], idx[i] = (block * n_envs + e) * n_agents + a -- the flying rows in ascending order, indexed by pi.  F < 1
 *   writes -1 everywhere.  Without team_prefix, n_envs and n_agents are ignored.
 * One lane per i, six Philox calls per point visited.  No context, no host synchronisation, no allocation, no scratch; launches on `stream`
 * only and can be captured; writes idx[0 .. n) and nothing else.  -1 with ippm_last_error set, and nothing launched, for a NULL idx,
 * n outside [1, 2^31), data_pass outside [0, 65536), team_prefix with n_envs < 1 or n_agents < 1, idx or round_dev not 8-byte aligned,
 * team_prefix not 4-byte aligned. */
#define IPPM_SHUFFLE_ROUNDS 6
int ippm_minibatch_permutation(uint64_t seed, int64_t round, const int64_t* round_dev, int32_t data_pass, int64_t n,
                               const int32_t* team_prefix, int32_t n_envs, int32_t n_agents, int64_t* idx, void* stream);

/* ---- greedy information-gain planner (IG_baseline.py:222-325) and evaluation metrics -------------------------
 * ippm_ig_candidates (K9): gains float [E,N,A] = expected weighted entropy reduction over the footprint each valid action
 * leads to, / 1000 (get_individual_ig); masked actions get 0.  ippm_ig_select (K10): get_relative_ig +
 * get_cell_utilities (when communication != 0) + argmax -> action int32 [E,N]; utilities float [E,N,A] optional.
 * An agent whose candidates all have zero gain gets 0 / 0 = nan relative gains, and np.argmax's rule applies (the first nan
 * is the maximum), as in the reference.
 * ippm_f1_counts: int64 [n_maps,3] = (tp, fp, fn) of the map thresholded at log-odds > logodds_threshold (0 <=> p > 0.5)
 * against the truth (utils/utils.py:64-76: sklearn f1_score(...)[1] = 2tp / (2tp + fp + fn)).  Cells whose evidence
 * cancels exactly sit at p = 0.5 +- rounding noise in the reference, which decides their class there; the threshold lets
 * a caller bracket that. */
int ippm_ig_candidates(ippm_ctx* ctx, const float* local, const int32_t* pos, const uint8_t* mask, float* gains,
                       int32_t n_envs, void* stream);
int ippm_ig_select(ippm_ctx* ctx, const int32_t* pos, const uint8_t* mask, const float* gains, int32_t communication,
                   int32_t* action, float* utilities, int32_t n_envs, void* stream);
int ippm_f1_counts(ippm_ctx* ctx, const float* maps, const uint8_t* truth, int32_t maps_per_truth, float logodds_threshold,
                   int64_t* out, int32_t n_maps, void* stream);

/* ---- scoring of belief maps: what every comparison script of the reference reports per step (coma_test.py:84-97,150-196,
 * IG_baseline.py:84-97, random_baseline.py, lawn_mower.py), in ONE streaming read of the maps (4 B + 1 bit per cell).
 *   maps     n_maps whole maps of gx*gy float log-odds in the context's map layout; map m is scored against truth[m / maps_per_truth]
 *            (the bit-packed planes; maps_per_truth = 1 for global maps, N for the agents' local maps);
 *   entropy  double [n_maps]: sum over the cells with truth bit 1 of H(sigmoid(clamp(L, +-logit_clip))) in bits -- the "eval" weighting
 *            of utils/state.py:53-121 as IG_baseline.py:84-97 uses it; the mean over the target cells is entropy / (tp + fn);
 *   counts   int64 [n_maps,3,3]: (tp, fp, fn) of the target class for the map thresholded at L > thr_k, thr = (+logodds_delta, 0,
 *            -logodds_delta) (utils/utils.py:64-76; DESIGN.md section 7 on why +-1e-5 bracket the exactly-cancelled cells);
 *   scratch  double [ippm_score_scratch(n_maps)], caller-owned: the per-part partial sums.
 * Every output element is written (nothing to zero beforehand).  Deterministic: no atomics, and the parts a map is summed in depend on
 * the grid only -- a map scores the same, bit for bit, alone and in any batch.  The entropy of a nearly saturated cell is evaluated in
 * the planner's series form (relative error below 1e-6 up to the clip; the log2(1 + e) form of ippm_weighted_entropy loses 6e-5 there). */
int ippm_score_scratch(ippm_ctx* ctx, int32_t n_maps, int64_t* doubles);
int ippm_score_maps(ippm_ctx* ctx, const float* maps, const uint8_t* truth, int32_t maps_per_truth, float logodds_delta,
                    double* entropy, int64_t* counts, double* scratch, int32_t n_maps, void* stream);

/* Synthetic random-field terrain: the device ends of the spectral synthesis the reference performs for every episode
 * (mapping/ground_truths.py:16-40; mapping/simulations.py:34-40) and then overwrites with the half-plane split.  The
 * caller runs the two FFTs and the sqrt(P(k)) product between the calls (ippmarl/terrain.py uses rocFFT via torch.fft).
 * ippm_terrain_noise: standard-normal white noise float [E,gx,gy] from Philox(seed; episode, cell), so an episode's
 *   terrain is the same in every batch and on every rank.
 * Power-of-two grids (sides 8..1024) do the whole synthesis in the library: the spectrum is drawn directly (the FFT of
 *   real N(0,1) noise is Hermitian complex white noise) and inverted in two LDS passes.
 *   ippm_terrain_spectrum: spec complex64 [E,gx,gy/2+1] = amp[gx,gy/2+1] * bin noise, Philox(seed; episode, bin).
 *   ippm_terrain_field: field float [E,gx,gy] = unnormalised inverse real transform of `spec`, or, when spec is NULL,
 *     of the spectrum ippm_terrain_spectrum would have written for (episode, amp) (drawn in-kernel, never stored);
 *     work = complex64 [E,gy/2+1,gx] scratch.  range_keys (uint32 [E,2], optional) receives each field's (min, max)
 *     as order-preserving keys (key = ~bits for negative floats, bits | 0x80000000 otherwise) for ippm_terrain_pack.
 * ippm_terrain_pack: truth bit = (f - min f)/(max f - min f) >= 0.5 per env (ground_truths.py:32-40), written in the
 *   bit-packed truth layout above; min/max are taken from range_keys when given, else reduced here. */
int ippm_terrain_noise(ippm_ctx* ctx, const int64_t* episode, float* noise, int32_t n_envs, void* stream);
int ippm_terrain_spectrum(ippm_ctx* ctx, const int64_t* episode, const float* amp, float* spec, int32_t n_envs, void* stream);
int ippm_terrain_field(ippm_ctx* ctx, const int64_t* episode, const float* amp, const float* spec, float* work, float* field,
                       uint32_t* range_keys, int32_t n_envs, void* stream);
int ippm_terrain_pack(ippm_ctx* ctx, const float* field, const uint32_t* range_keys, uint8_t* truth, int32_t n_envs, void* stream);
/* ippm_terrain_truth = ippm_terrain_field(spec = NULL) + ippm_terrain_pack without ever storing the field: the second transform
 * pass runs twice (once for the field's min / max, once more for the threshold bits, same arithmetic), which moves half the bytes
 * of writing the field and reading it back -- or, for sides of 128 / 256 cells in batches of 128 envs or more, runs once with one
 * workgroup per env that holds the env's rows in registers; the same truth and keys bit for bit.  work: complex64 [E,gy/2+1,gx] scratch; range_keys: uint32 [4*E + 4] scratch (per env:
 * min key, max key, and two words + a trailing record for the one-launch form of the pass, IPPM_TERRAIN_ONE_LAUNCH=1: arrivals, a
 * fault word that stays 0 unless an in-launch wait gave up, the launch's ticket counter). */
int ippm_terrain_truth(ippm_ctx* ctx, const int64_t* episode, const float* amp, float* work, uint32_t* range_keys, uint8_t* truth,
                       int32_t n_envs, void* stream);

/* ---- terrain library: episodes over caller-supplied ground-truth maps ------------------------------------------------------------------
 * The caller hands over n_maps binary maps of lgx x lgy cells once; they are kept bit-packed on the device, and every reset cuts each
 * env's truth plane out of them: a map, a crop window of the grid's size and, optionally, one of the 8 symmetries of the square, drawn
 * from (philox_seed, episode) alone -- fixed episodes mean the same truth in every batch, on every rank, whoever flies them.
 *   THE DRAW of episode ep under seed s:
 *     r = Philox4x32-10(counter = (0, ep & 0xFFFFFFFF, stream word(agent 0, stage 0, domain 5), ep >> 32), key = (s & 0xFFFFFFFF, s >> 32))
 *     (the counter convention of the action and comm draws; domain 5 is this draw's own); mulhi(w, n) = (uint64) w * n >> 32.
 *     sym  bit 0 (flip x) and bit 1 (flip y) = r[3] & 3 when flags & IPPM_LIBRARY_FLIP, else 0;
 *          bit 2 (transpose) = (r[3] >> 2) & 1 when flags & IPPM_LIBRARY_TRANSPOSE, else 0.
 *     m    = mulhi(r[0], n_maps).
 *     The window has wr x wc library cells, (gx, gy) untransposed, (gy, gx) transposed:
 *     x0 = mulhi(r[1], lgx - wr + 1), y0 = mulhi(r[2], lgy - wc + 1).
 *     truth(x, y) = L_m[u][v] with x' = (sym & 1) ? gx - 1 - x : x, y' = (sym & 2) ? gy - 1 - y : y and
 *     (u, v) = (x0 + x', y0 + y') untransposed, (x0 + y', y0 + x') transposed.
 *   Sizes, checked on the host before any launch (-1 with ippm_last_error set, nothing launched): n_maps >= 1, lgx >= gx and lgy >= gy;
 *   with IPPM_LIBRARY_TRANSPOSE also lgx >= gy and lgy >= gx; one packed map stays below 2^31 bytes; flags has no other bits.
 *   LAYOUT of the packed library (a C caller may pack on the host): uint32 words, map m, row u starts at word (m * lgx + u) * lw with
 *   lw = ceil(lgy / 32); cell v of the row is bit v & 31 of word v >> 5; bits past lgy are zero.  ippm_terrain_library_bytes =
 *   n_maps * lgx * lw * 4: no tail padding -- the draw reads single words through a bounds-checked buffer resource of the drawn map.
 * ippm_terrain_library_pack: cells uint8 [n_maps, lgx, lgy] on the device, nonzero = target class -> lib.  One launch, every byte of lib
 *   is written; needs no context.
 * ippm_terrain_library_draw: one launch (timed under IPPM_T_TERRAIN) writes, for every env, ALL ippm truth bytes of its plane (the
 *   row-major bit string of the truth layout above whatever the maps' storage layout; the padding bits behind the last cell and the spare
 *   byte of grids with gy % 4 != 0 are written as zero) and, when draws is given, draws int32 [E,4] = (m, x0, y0, sym).  Grid and seed are
 *   the context's.  No atomics, no scratch, no allocation, no synchronisation; launches on `stream` only and can be captured.  Any
 *   n_envs >= 1 whose workgroups (n_envs * ceil(truth words / 256), or n_envs * ceil(gx / 32) when transposing) stay below 2^31. */
#define IPPM_LIBRARY_FLIP 1
#define IPPM_LIBRARY_TRANSPOSE 2
int ippm_terrain_library_bytes(int32_t n_maps, int32_t lgx, int32_t lgy, int64_t* bytes);
int ippm_terrain_library_pack(const uint8_t* cells, int32_t n_maps, int32_t lgx, int32_t lgy, uint32_t* lib, void* stream);
int ippm_terrain_library_draw(ippm_ctx* ctx, const int64_t* episode, const uint32_t* lib, int32_t n_maps, int32_t lgx, int32_t lgy,
                              int32_t flags, int32_t* draws, uint8_t* truth, int32_t n_envs, void* stream);

/* Host helpers (no GPU needed): exported so that CPU-only tests can pin the device's integer streams and
 * resize weights to NumPy / the oracle. */
int ippm_area_weights(int32_t n_src, int32_t n_dst, int32_t* bin0, float* w0, float* w1);
int ippm_host_philox(const uint32_t* ctr_key6, uint32_t* out4);           /* Philox4x32-10(c0..c3,k0,k1) */
int ippm_host_start_state(int32_t env_seed, int64_t episode, int32_t agent, int32_t spacing, int32_t space_x,
                          int32_t space_y, int32_t* out3);                /* state_space.py:28-51 */
int ippm_host_truth_params(int64_t episode, int32_t* out2);               /* ground_truths.py:43-48 */
/* the draw of ippm_terrain_library_draw for one episode: out4 = (m, x0, y0, sym); the same size checks and error returns */
int ippm_host_library_draw(uint64_t seed, int64_t episode, int32_t n_maps, int32_t lgx, int32_t lgy, int32_t gx, int32_t gy,
                           int32_t flags, int32_t* out4);

#ifdef __cplusplus
}
#endif
#endif /* IPPMARL_H */
