"""Batched COMA training loop: E device-resident environments roll out in lock step, the update runs on the whole
buffer.  Mirrors the cadence of COMAMission.execute (missions/coma_mission.py:48-172): rollout -> TD(lambda) targets
(K8) -> data_passes x batch_number minibatch steps of critic then actor (K7 inside the actor step).

One "update" = TD-target build + data_passes * batch_number Adam steps of each net, exactly the reference's round; the
number of transitions per round scales with the number of batched envs (reference: 300; here waves * T * E * N).
"""
from __future__ import annotations

import copy
from typing import Dict, Optional

import torch

from . import _ffi
from . import critic_native
from . import metrics_native
from . import optim_native
from . import replay_native
from . import rollout_native
from . import round as seams
from . import shuffle_native
from . import switches
from .actor_native import NativeActor, resolve_mode
from .learners import ActorLearner, CriticLearner
from .networks import ActorNetwork, CriticNetwork, epsilon_schedule, resolve_conv2_update, resolve_head_update, resolve_trunk_update
from .parallel import GradAllReducer, broadcast_module, episode_ids
from .vec_env import VecEnv, POLICY_ARGMAX, POLICY_EXPLICIT, POLICY_SAMPLE, POLICY_UNIFORM


class COMATrainer:
    def __init__(self, params: Dict, n_envs: int, device: str = "cuda:0", philox_seed: int = 3, waves_per_update: int = 1,
                 quirks: str = "reference", rank: int = 0, world: int = 1, first_episode: int = 1,
                 terrain: str = "split", graphs: bool = False, placement_draws: int = 0, team_sizes=None,
                 terrain_library=None, library_augment: str = "d4",
                 shuffle: Optional[str] = None, rollout_log: Optional[str] = None, metrics: Optional[str] = None,
                 buffer: Optional[str] = None,
                 actor_inference: Optional[str] = None, critic_inference: Optional[str] = None, adam: Optional[str] = None,
                 head_update: Optional[str] = None, conv2_update: Optional[str] = None, trunk_update: Optional[str] = None):
        self.params = params
        self.philox_seed = int(philox_seed)
        # the ten opt-in paths (switches.TABLE; None reads the switch's environment variable): resolved before anything needs the GPU;
        # what each selects is described in its module's docstring and in INTEGRATION.md
        self.shuffle = shuffle_native.resolve_mode(shuffle)                       # where the minibatch order of update() comes from
        self.metrics = metrics_native.resolve_mode(metrics)                       # who computes update(diagnostics=True)'s 32 scalars
        self.buffer = replay_native.resolve_mode(buffer)                          # who writes, chains and gathers the buf_* tensors
        self.rollout_log = rollout_native.resolve_mode(rollout_log)               # who computes the log a ``keep_rollout_log`` trainer keeps
        self.adam = optim_native.resolve_mode(adam)                               # the learners' optimizer
        self.head_update = resolve_head_update(head_update)                       # fc1, fc3 and the losses of the forward with gradients
        self.trunk_update = resolve_trunk_update(trunk_update)                    # conv1, conv2, conv3 of the forward with gradients
        self.conv2_update = resolve_conv2_update(conv2_update)                    # conv2 alone of the forward with gradients
        self.actor_inference = resolve_mode(actor_inference)                      # every no-grad use of the actor
        self.critic_inference = critic_native.resolve_mode(critic_inference)      # the TD targets and the post-step Q
        self._shuffle = self._metrics = self._replay = self._rollout_log = self._native = None
        self._native_critic = self._native_target = None
        self._graph_metrics = False
        self.rollout_log_waves = None     # waves the native log holds (None: waves_per_update); set it before the first logged rollout
        self.eval_wave = 0                # the native log's slot of the next eval wave; read_rollout_log("eval", ...) rewinds it
        self.step_replays = 0             # recorded rollout steps replayed so far
        # team_sizes: mixed team sizes in one batch (VecEnv): the transitions of agents that do not fly never enter a minibatch
        # terrain="library": every episode flies over a crop of `terrain_library` (VecEnv).  The library is not part of the trainer's state
        # or fingerprint: a resumed run must be given the same maps and `library_augment` to fly the same episodes.
        self.env = VecEnv(params, n_envs, device=device, philox_seed=philox_seed, terrain=terrain, team_sizes=team_sizes,
                          terrain_library=terrain_library, library_augment=library_augment)
        # mission type DeepQ (coma_wrapper.py:113-171): every agent's transition carries ITS information gain (VecEnv.agent_reward, on
        # for DeepQ), each (env, agent) TD chain is built from its own rewards, and the return is the last flying agent's, as the
        # reference's EpisodeGenerator sums it; team_return keeps the COMA team reward beside it
        self.deepq = params["experiment"]["missions"].get("type") == "DeepQ"
        if self.deepq and not self.env.agent_rewards:
            raise _ffi.IppmError("COMATrainer: mission type DeepQ needs the per-agent rewards of the env")
        # Large batches: where the allocator put the maps decides ~10 % of the rollout's map kernels (VecEnv.tune_placement).  The
        # search is OPT-IN (placement_draws > 1; bench.py passes its own --placement-draws): it steps the env for ~10 ms a draw and
        # holds candidate arenas within half of the free memory while it runs, which a caller should ask for, not find out about.
        self.placement = self.env.tune_placement(placement_draws) if placement_draws > 1 else None
        self.device = self.env.device
        self.rank, self.world = rank, world
        self.first_episode = first_episode
        self.waves_per_update = waves_per_update
        self.quirks = quirks
        d = self.env.d
        self.T, self.E, self.N, self.A = d.budget + 1, self.env.E, d.n_agents, d.n_actions
        net = params["networks"]
        self.data_passes, self.batch_number = net["data_passes"], net["batch_number"]
        self.actor = ActorNetwork(params)
        self.critic = CriticNetwork(params)
        # the reference builds TD targets with a deepcopy of the critic taken at construction that is
        # never synchronised; quirks="fixed" uses the learner's synchronised target network instead
        self.frozen_target = copy.deepcopy(self.critic).to(self.device).eval()
        # graphs: the round is launch-bound at small env counts (the reference's own 5 episodes per round: ~3000 launches of a
        # few microseconds of work each, Python between them); capture_graphs() records every rollout step and the whole update
        # into hipGraphs.  graphs=True changes the optimizer IMPLEMENTATION for every round of this trainer, recorded or not: both
        # Adam instances are torch's fused capturable form (step counters on the device, one kernel per step), whose update agrees
        # with the default form to float32 rounding, not bit for bit; their state is not part of save_actor's pickle.  (adam="native"
        # has one implementation for both.)
        self.graphs = bool(graphs)
        self._step_graphs = self._update_graph = None
        self.actor_learner = ActorLearner(params, self.actor, self.device, ctx=self.env.ctx, capturable=self.graphs, adam=self.adam,
                                          head_update=self.head_update, conv2_update=self.conv2_update, trunk_update=self.trunk_update,
                                          metrics=self.metrics)
        self.critic_learner = CriticLearner(params, self.critic, self.device, capturable=self.graphs, adam=self.adam,
                                            head_update=self.head_update, conv2_update=self.conv2_update, trunk_update=self.trunk_update,
                                            metrics=self.metrics)
        for m in (self.actor, self.critic, self.critic_learner.target_critic, self.frozen_target):
            broadcast_module(m)
        # gradients of both nets live in one flat buffer (critic, then actor): the data-parallel average is one all-reduce of a
        # view, and the actor's gradients of minibatch b travel together with the critic's of minibatch b+1
        self.reducer = GradAllReducer().attach(self.critic, self.actor, skip=GradAllReducer.unused_fc2)
        self._grads_checked = False
        W, T, E, N = waves_per_update, self.T, self.E, self.N
        dev = self.device
        self.buf_obs = torch.empty(W, T, E, N, 11, 11, 7, device=dev)
        self.buf_state = torch.empty(W, T, E, N, 11, 11, 12, device=dev)
        self.buf_action = torch.empty(W, T, E, N, dtype=torch.int32, device=dev)
        self.buf_mask = torch.empty(W, T, E, N, self.A, dtype=torch.uint8, device=dev)
        # rewards: one per env (COMA: the team reward, broadcast to its agents' chains) or one per (env, agent) (DeepQ)
        self.buf_reward = torch.empty(W, T, E, N, device=dev) if self.deepq else torch.empty(W, T, E, device=dev)
        # index of the last agent that flies in each env: whose reward a DeepQ episode's return sums (coma_wrapper.py:113-171)
        last = (self.env.n_active.long() - 1) if self.env.n_active is not None else torch.full((E,), N - 1, dtype=torch.long, device=dev)
        self._last_agent = last.view(E, 1, 1).expand(E, 1, 2).contiguous()
        self.wave = 0          # rollout waves done so far (defines the episode numbers)
        self.filled = 0        # waves currently in the buffer
        self.train_step = 0
        self.eps = epsilon_schedule(params, 0)
        self.eps_dev = torch.full((), float(self.eps), dtype=torch.float32, device=dev)   # epsilon as the graphs read it
        self.ret = torch.zeros(E, device=dev)
        self.abs_ret = torch.zeros(E, device=dev)
        self.team_ret = torch.zeros(E, device=dev)   # the COMA team reward summed (= ret unless DeepQ)
        self.keep_rollout_log = False
        self._log_wave = None             # slot of the native rollout log the current wave's steps write (None: no log launch)
        self.last_rollout = None
        self.last_diagnostics = None
        if self.buffer == "native":
            self._replay = replay_native.NativeReplay(
                self.env.ctx, (self.buf_obs, self.buf_state, self.buf_action, self.buf_mask, self.buf_reward),
                (self.ret, self.abs_ret, self.team_ret), self.batch_number, last_agent=last if self.deepq else None)
        if self.shuffle == "native":
            flying = E * N if self.env.n_active is None else int(self.env.n_active.sum())
            self._shuffle = shuffle_native.NativeShuffle(self.philox_seed, self.data_passes, W * T * flying, dev, self.env.n_active, E, N)
        self._order = seams.NativeOrder(self, self._shuffle) if self._shuffle is not None else seams.TorchOrder(self)
        if self.critic_inference == "native":
            self.critic_learner.inference = self._native_critic = critic_native.NativeCritic(self.critic, self.device)
            self._native_critic.reserve(W * T * E * N)
            self.native_target()

    # ------------------------------------------------------------------------------------------------
    def rollout(self, mode: str = "train") -> Dict[str, float]:
        """One wave: E episodes in lock step (EpisodeGenerator.execute for every env at once)."""
        env = self.env
        eps_ids = episode_ids(self.first_episode, self.wave, self.E, self.rank, self.world)
        # the reference anneals epsilon with the episode index (actor/network.py:53-58); one wave = E episodes
        self.eps = epsilon_schedule(self.params, int(eps_ids[0]))
        self.eps_dev.fill_(float(self.eps))
        env.reset(eps_ids)
        w = self.filled
        ret, abs_ret = self.ret.zero_(), self.abs_ret.zero_()
        self.team_ret.zero_()
        policy = POLICY_ARGMAX if mode == "eval" else POLICY_SAMPLE
        step_rewards, step_actions, step_altitudes = [], [], []
        native_log = self.rollout_log == "native" and self.keep_rollout_log
        replay = self._step_graphs is not None and mode == "train" and w == 0 and (native_log or not self.keep_rollout_log)
        # (the native log's slot: train waves follow the buffer's, eval waves their own counter)
        self._log_wave = (w if mode == "train" else self.eval_wave) if native_log else None
        if replay and self.actor_inference == "native":
            self.native_actor().sync()    # (weights written from the host since the last pack: the recorded steps read the pack)
        for t in range(self.T):
            if replay:
                self._step_graphs[t].replay()
                self.step_replays += 1
                # (the host-side bookkeeping of the env that a replayed step skips: the step counter, no fusion pending, the
                #  observations held are those of step t)
                env.t, env._pending_t, env._obs_t = t + 1, None, t
                continue
            reward = self._rollout_step(t, w, policy, mode == "train", self.eps_dev if self.graphs else self.eps)
            if self.keep_rollout_log and not native_log:
                step_rewards.append(reward[:, 0].clone())
                step_actions.append(env.action.clone())
                step_altitudes.append(env.pos[:, :, 2].clone())
        if native_log:
            self._log_wave = None
            if mode == "eval":
                self.eval_wave += 1
        elif self.keep_rollout_log:   # per-episode figures for the mission log (coma_mission.py:78-82)
            self.last_rollout = dict(episode_returns=ret.clone(), absolute_returns=abs_ret.clone(),
                                     rewards=torch.stack(step_rewards, 1), actions=torch.stack(step_actions, 1),
                                     altitudes=torch.stack(step_altitudes, 1))
        self.wave += 1
        if mode == "train":
            self.filled += 1
        return {"episode_return": float(ret.mean()), "absolute_return": float(abs_ret.mean()),
                "team_return": float(self.team_ret.mean()), "eps": self.eps, "faults": int(env.fault.ne(0).sum())}

    def _rollout_step(self, t: int, w: int, policy: int, store: bool, eps):
        """One lock-step env step of all E envs: observations -> actor -> move + sense (+ the transition into the buffer)."""
        env = self.env
        obs = env.build_observations(t)
        probs = self._act(obs, eps)
        reward, done, state = env.steps(t, policy=policy, probs=probs.view(self.E, self.N, self.A))
        team = reward
        if self._replay is not None:
            # one launch: the transition into slot (w, t) and one float32 add on each of ret, abs_ret, team_ret
            self._replay.store(w, t, obs, state, env.action, env.mask, reward, env.agent_reward if self.deepq else None, store=store)
            # (the returned reward is read by rollout()'s torch log only: the DeepQ gather is spent when that log is kept)
            if self.deepq and self.keep_rollout_log and self._log_wave is None:
                reward = self.last_agent_reward()
        else:
            if self.deepq:
                reward = self.last_agent_reward()
            if store:
                self.buf_obs[w, t].copy_(obs)
                self.buf_state[w, t].copy_(state)
                self.buf_action[w, t].copy_(env.action)
                self.buf_mask[w, t].copy_(env.mask)
                self.buf_reward[w, t].copy_(env.agent_reward[..., 0] if self.deepq else reward[:, 0])
            self.ret += reward[:, 0]
            self.abs_ret += reward[:, 1]
            self.team_ret += team[:, 0]
        if self._log_wave is not None:
            self._log_step(t, team)
        return reward

    def _log_step(self, t: int, reward: torch.Tensor):
        """Step ``t``'s share of the native rollout log into slot (``_log_wave``, t): one launch on the current stream, after env.steps.
        DeepQ hands over the per-agent rewards (the kernel takes the last flying agent's row) instead of spending the gather."""
        env = self.env
        self.native_rollout_log().step(self._log_wave, t, reward, env.agent_reward if self.deepq else None, env.action, env.pos,
                                       env.n_active)

    def native_rollout_log(self):
        """The NativeRolloutLog of this trainer (built on first use, for ``rollout_log_waves`` waves; the recorded steps hold its
        addresses, so it is never rebuilt)."""
        if self._rollout_log is None:
            if torch.cuda.is_current_stream_capturing():
                raise _ffi.IppmError("COMATrainer: the native rollout log must be allocated before a capture")
            d = self.env.d
            waves = max(int(self.rollout_log_waves or 0), self.waves_per_update, 1)
            self._rollout_log = rollout_native.NativeRolloutLog(waves, self.T, self.E, self.N, self.A, d.min_altitude, d.spacing, d.space_z,
                                                                self.device)
        return self._rollout_log

    def read_rollout_log(self, mode: str = "train", n_waves: int = 1):
        """The native rollout log of the last ``n_waves`` logged waves of ``mode`` (slots 0 .. n_waves - 1: a round's train waves, or the
        eval waves since the last read): the closing launch and ONE device-to-host copy -> (scalars under the reference's ``mode``-prefixed
        tags, action counts, {altitude in metres: count}, entries counted in no bin)."""
        if self.rollout_log != "native":
            raise _ffi.IppmError('read_rollout_log needs COMATrainer(rollout_log="native")')
        log = self.native_rollout_log()
        if not 1 <= n_waves <= log.W:
            raise _ffi.IppmError(f"read_rollout_log: n_waves must be in [1, {log.W}] (rollout_log_waves), got {n_waves}")
        log.finalize(n_waves)
        if mode == "eval":
            self.eval_wave = 0
        return log.read(mode)

    def _act(self, obs: torch.Tensor, eps) -> torch.Tensor:
        """probs [E*N, A] of the current actor for the observations [E,N,11,11,7], without gradients, on the selected inference path."""
        return self._act_rows(obs.view(self.E * self.N, 11, 11, 7), eps)

    def _act_rows(self, obs: torch.Tensor, eps) -> torch.Tensor:
        """``_act`` for any number of rows [B,11,11,7] (the native metrics' post-pass forwards on the minibatches)."""
        if self.actor_inference == "native":
            return self.native_actor()(obs, eps)[0]
        with torch.no_grad():
            return self.actor(obs, eps)[0]

    def native_actor(self):
        """The NativeActor of ``self.actor`` (built on first use, rebuilt when ``self.actor`` has been replaced by another module)."""
        if self._native is None or self._native.module is not self.actor:
            self._native = NativeActor(self.actor, self.device)
            self._native.reserve(self.E * self.N)
            if self.adam == "native" and self.actor is self.actor_learner.actor:
                self.actor_learner.optimizer.attach_pack(self._native)     # every actor step rewrites this pack in its own launch
        return self._native

    def target_module(self):
        """The critic whose Q the TD targets are built from: the never-synchronised copy taken at construction
        (quirks="reference"), or the learner's target network."""
        return self.frozen_target if self.quirks == "reference" else self.critic_learner.target_critic

    def native_target(self):
        """The NativeCritic of ``target_module()`` (rebuilt when that has become another module).  The frozen copy is packed once; the
        learner's target network is repacked by ``sync()`` after a hard or soft update wrote it."""
        target = self.target_module()
        if self._native_target is None or self._native_target.module is not target:
            self._native_target = critic_native.NativeCritic(target, self.device)
            self._native_target.reserve(self.waves_per_update * self.T * self.E * self.N)
        return self._native_target

    def refresh_actor_inference(self):
        """Repack the native actor from the module's current parameters (no-op on the torch path): update() does it after its
        optimizer steps; call it after loading a state dict into ``self.actor`` by other means."""
        if self.actor_inference == "native":
            native = self.native_actor()
            if self.adam == "native" and self.actor_learner.optimizer._pack is native:
                native.sync()      # (the optimizer's steps kept the pack and its stamp current: a host-side check, no launch)
            else:
                native.refresh()

    def last_agent_reward(self) -> torch.Tensor:
        """[E, 2] DeepQ (relative, absolute) reward of the last agent that flies in each env: what the reference's wrapper returns
        and EpisodeGenerator sums into the episode's return (coma_wrapper.py:113-171)."""
        return self.env.agent_reward.gather(1, self._last_agent).squeeze(1)

    def capture_graphs(self):
        """Records the launch-bound round into hipGraphs: one graph per rollout step t of a training wave (the step number is an
        argument of several kernels, everything else -- episode numbers, epsilon, every array -- is read from fixed device
        buffers) and one graph for the whole update (TD targets + data_passes x batch_number minibatch steps of both nets, the
        minibatch permutations read from a fixed buffer that update() refills -- or, shuffle="native", written by launches inside the
        graph from a device round counter that its last node advances).  Needs one eager round first (MIOpen's kernel
        selection, allocator warm-up); waves_per_update = 1, hard target updates, one rank."""
        if not self.graphs:
            raise _ffi.IppmError("COMATrainer(graphs=True) is needed: captured optimizer steps keep their counters on the device")
        if self.waves_per_update != 1 or self.world != 1 or self.critic_learner.target_update_mode != "hard" or self.env.n_active is not None:
            raise _ffi.IppmError("capture_graphs: one wave per update, one rank, hard target updates and one team size only")
        env = self.env
        env.profile = False
        if self.actor_inference == "native":
            # parameters written from the host since the last pack: repack NOW, while launches still execute (a repack that a captured
            # step merely records would leave every eager forward after the capture on the old weights)
            self.native_actor().sync()
        if self.critic_inference == "native":    # (the same for both critic packs; their scratch is as large as the buffer already)
            self._native_critic.sync()
            self.native_target().sync()
        torch.cuda.synchronize(self.device)
        saved = {k: getattr(env, k).clone() for k in ("local", "glob", "ws", "sums", "pos", "pos_pre", "comm", "mask", "action", "fault",
                                                       "reward", "area", "rect", "rect_next", "code", "work")
                 + (("agent_reward", "agent_sums") if env.agent_rewards else ())}
        stream = torch.cuda.Stream(device=self.device)
        graphs = []
        # rollout_log="native": the log launch rides in every recorded step, logged or not (the log is allocated here, outside the capture)
        self._log_wave = None
        if self.rollout_log == "native":
            self.native_rollout_log()
            self._log_wave = 0
        for t in range(self.T):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                self._rollout_step(t, 0, POLICY_SAMPLE, True, self.eps_dev)
            graphs.append(g)
        self._log_wave = None
        n = self.T * self.E * self.N
        # metrics="native": the metric launches and the post-pass forwards are part of the recorded round (the accumulator is allocated
        # here, outside the capture); update(diagnostics=True) replays and reads ``out``, update(diagnostics=False) replays and reads nothing
        self._graph_metrics = self.metrics == "native"
        if self._graph_metrics:
            self._native_metrics(n // self.batch_number)
        perms = self._order.capture(n)      # (the fixed buffer the recorded data passes read their order from)
        self._loss_out = torch.zeros(2, device=self.device)
        filled, self.filled = self.filled, 1
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            closs, aloss = self._update_compute(perms, self.eps_dev, self._graph_metrics)
            self._loss_out[0].copy_(closs)
            self._loss_out[1].copy_(aloss)
            self._order.end_capture()
        self.filled = filled
        torch.cuda.synchronize(self.device)
        for k, v in saved.items():   # capture does not execute; keep the env's state untouched in any case
            getattr(env, k).copy_(v)
        self._step_graphs, self._update_graph = graphs, g
        env._graphs = graphs            # (the env's buffers are baked into the recording: VecEnv.tune_placement refuses from here on)

    # ------------------------------------------------------------------------------------------------
    def td_targets(self):
        """K8 over one chain per (env, agent): the transitions of all buffered waves in time order
        (BatchMemory.build_td_targets, batch_memory.py:120-162)."""
        W, T, E, N = self.filled, self.T, self.E, self.N
        target = self.target_module()
        states = self.buf_state[:W].reshape(W * T * E * N, 11, 11, 12)
        actions = self.buf_action[:W].reshape(-1)
        if self.critic_inference == "native":
            _, q_sel = self.native_target().forward(states, actions, want_q=False)    # one call: the kernel gathers the chosen Q
        else:
            q_sel = torch.empty(W * T * E * N, device=self.device)
            with torch.no_grad():
                chunk = 16384
                for lo in range(0, states.shape[0], chunk):
                    q, _ = target(states[lo:lo + chunk])
                    q_sel[lo:lo + chunk] = q.view(-1, self.A).gather(1, actions[lo:lo + chunk].long().view(-1, 1)).squeeze(1)
        if self._replay is not None:
            return self._replay.td_targets(q_sel, W)      # q_sel is in buffer order already: one launch, no permutes
        # chains: [E*N, W*T]
        q_sel = q_sel.view(W, T, E, N).permute(2, 3, 0, 1).reshape(E * N, W * T).contiguous()
        # (COMA: the env's team reward on each of its agents' chains; DeepQ: each agent's own)
        per_agent = self.buf_reward[:W] if self.deepq else self.buf_reward[:W].unsqueeze(-1).expand(W, T, E, N)
        rew = per_agent.permute(2, 3, 0, 1).reshape(E * N, W * T).contiguous()
        done = torch.zeros(W, T, dtype=torch.uint8, device=self.device)
        done[:, T - 1] = 1
        done = done.view(1, W * T).expand(E * N, W * T).contiguous()
        td = torch.empty_like(rew)
        dr = torch.empty_like(rew)
        self.env.ctx.call("ippm_td_lambda", _ffi.ptr(rew), _ffi.ptr(done), _ffi.ptr(q_sel), _ffi.ptr(td), _ffi.ptr(dr), E * N,
                          W * T, self.env.stream)
        # back to buffer order [W,T,E,N]
        to_buf = lambda x: x.view(E, N, W, T).permute(2, 3, 0, 1).reshape(-1)  # noqa: E731
        return to_buf(td), to_buf(dr)

    def update(self, diagnostics: bool = False) -> Dict[str, float]:
        """One COMA round on everything in the buffer, then clear it (coma_mission.py:89-116).  ``diagnostics``: also
        compute the reference's per-training-step TensorBoard figures from data pass 0 into ``self.last_diagnostics`` (costs one extra
        actor forward per minibatch).  metrics="torch": ippmarl.metrics on the learners' float32 records, launch by launch even when the
        round is recorded; metrics="native": libippmarl's reductions on the round as configured, replayed with the recorded round, one
        device-to-host read."""
        W, T, E, N = self.filled, self.T, self.E, self.N
        assert W > 0, "update() needs at least one rollout wave"
        n = W * T * E * N
        if self._update_graph is not None and W == 1 and (not diagnostics or self._graph_metrics):
            # the recorded round: hard target copy (a host-side decision) first, the round's minibatch order made ready, replay
            self.critic_learner.update_target_network(self.train_step, 0)
            if self.critic_inference == "native":
                self.native_target().sync()    # (the copy was written from the host: the recorded TD targets read the pack)
            self._order.before_replay(n)
            self._update_graph.replay()
            self._order.after_replay()
            self.train_step += 1
            closs, aloss = self._loss_out.tolist()
        else:
            closs, aloss = self._update_compute(None, self.eps_dev if self.graphs else self.eps, diagnostics)
        if diagnostics and self.metrics == "native":
            self.last_diagnostics = self._metrics.read()
        self.filled = 0
        total = n * self.world
        if self.env.n_active is not None:
            # mixed team sizes: every rank counts its own flying agents (the ranks' teams differ), summed over the ranks
            mine = torch.tensor([int(self.env.n_active.sum()) * W * T], dtype=torch.int64, device=self.device)
            if self.world > 1:
                import torch.distributed as dist
                if dist.get_backend() == "gloo":
                    mine = mine.cpu()
                dist.all_reduce(mine)
            total = int(mine[0])
        return {"critic_loss": float(closs), "actor_loss": float(aloss), "transitions": total,
                "adam_steps": 2 * self.data_passes * self.batch_number, "train_step": self.train_step}

    def _native_metrics(self, batch: int):
        """The NativeMetrics of a round of ``batch_number`` minibatches of ``batch`` rows (rebuilt when the minibatch size changes; a
        recorded round holds its addresses, so there it must not)."""
        if self._metrics is None or not self._metrics.matches(self.batch_number, batch, self.A):
            if torch.cuda.is_current_stream_capturing() or (self._graph_metrics and self._update_graph is not None):
                raise _ffi.IppmError("COMATrainer: the minibatch size of the recorded round's native metrics has changed")
            self._metrics = metrics_native.NativeMetrics(self.batch_number, batch, self.A, self.device)
        return self._metrics

    def valid_transitions(self, waves: int) -> Optional[torch.Tensor]:
        """Indices into the flattened [waves, T, E, N] buffers of the transitions of agents that fly (None: all of them do)."""
        if self.env.n_active is None:
            return None
        flying = torch.arange(self.N, device=self.device).view(1, self.N) < self.env.n_active.view(self.E, 1)     # [E, N]
        return flying.view(1, 1, self.E, self.N).expand(waves, self.T, self.E, self.N).reshape(-1).nonzero().view(-1)

    def _update_compute(self, perms, eps, diagnostics: bool):
        """The arithmetic of one round.  ``perms`` None: eager (draws the minibatch permutations, syncs the target network and
        counts train steps as it goes); what ``_order.capture`` returned: the form capture_graphs records (those host-side pieces are
        done by update() around the replay).  Where the order, the minibatches' rows and the diagnostics come from is behind the three
        seams of ippmarl.round, chosen here once per round."""
        W = self.filled
        eager = perms is None
        td, dr = self.td_targets()
        nv = self._order.begin_round(W)
        bs = nv // self.batch_number
        # (a diagnostics round of metrics="torch" keeps the torch gathers: its records hold minibatch tensors across minibatches)
        torch_records = diagnostics and self.metrics == "torch"
        batches = (seams.NativeBatches if self._replay is not None and not torch_records else seams.TorchBatches)(self, W, td)
        if not diagnostics:
            watcher = seams.Unobserved(self)
        elif torch_records:
            watcher = seams.TorchObserver(self, batches, dr)
        else:
            watcher = seams.NativeObserver(self, batches, dr, self._native_metrics(bs))
        critic, actor = self.critic_learner, self.actor_learner
        closs = aloss = torch.zeros((), device=self.device)
        for data_pass in range(self.data_passes):
            perm = self._order.order(data_pass, nv, perms)
            if eager:
                critic.update_target_network(self.train_step, data_pass)
            batches.begin_pass(perm, bs, self.batch_number)
            seen = watcher.begin_pass(data_pass)
            unchecked = eager and not self._grads_checked   # once: no gradient of the attached nets lives outside the reduced buffer
            # Reference order (critic/learner.py:58-105, actor/learner.py:36-101): all critic minibatches, each followed by
            # the post-step Q of ITS minibatch, then all actor minibatches with those Q.  Neither net's step feeds the
            # other's, so interleaving them -- actor(b) right after critic(b) -- computes the same numbers; it lets the
            # gradient exchange of actor(b) and critic(b+1) share one all-reduce (B+1 collectives per pass, not 2B).
            closs = critic.backward(*batches.critic(0))
            if unchecked:
                self.reducer.check_covered()
            self.reducer(self.critic)
            seen.critic_reduced(0)
            q_b = critic.apply()
            seen.critic_applied(0)
            for b in range(self.batch_number):
                seen.before_actor(b)
                aloss, _ = actor.backward(*batches.actor(b), q_b, eps)
                seen.after_actor(b)
                if unchecked and b == 0:
                    self.reducer.check_covered()
                    self._grads_checked = True
                if b + 1 < self.batch_number:
                    closs = critic.backward(*batches.critic(b + 1))
                    self.reducer(self.critic, self.actor)
                    seen.critic_reduced(b + 1)
                    seen.actor_reduced(b)
                    actor.apply()
                    q_b = critic.apply()
                    seen.critic_applied(b + 1)
                else:
                    self.reducer(self.actor)
                    seen.actor_reduced(b)
                    actor.apply()
            seen.end_pass(eps)
            if data_pass == 0 and eager:
                self.train_step += 1
        self.refresh_actor_inference()   # (recorded with the round when capture_graphs records it)
        return closs, aloss

    def train(self, n_updates: int, log=None):
        history = []
        for _ in range(n_updates):
            stats = {}
            for _ in range(self.waves_per_update):
                stats = self.rollout("train")
            stats.update(self.update())
            history.append(stats)
            if log:
                log(stats)
        return history

    # ------------------------------------------------------------------------------------------------
    def map_metrics(self, glob: Optional[torch.Tensor] = None):
        """Per-env evaluation metrics of fused global maps (default: the env's; coma_test.py:84-97,177-196;
        IG_baseline.py:84-97): mean entropy over the target cells (weights from the ground truth) and F1 of the target
        class at p > 0.5."""
        env = self.env
        glob = env.glob if glob is None else glob
        ent = torch.zeros(self.E, dtype=torch.float64, device=self.device)
        env.ctx.call("ippm_weighted_entropy", env._p(glob), env._p(env.truth), 1, _ffi.ptr(ent), self.E, env.stream)
        counts = self.f1_counts(glob, 0.0)
        tp, fp, fn = counts[:, 0].double(), counts[:, 1].double(), counts[:, 2].double()
        target = (tp + fn).clamp_min(1)
        f1 = torch.where(2 * tp + fp + fn > 0, 2 * tp / (2 * tp + fp + fn).clamp_min(1), torch.zeros_like(tp))
        return ent / target, f1

    def f1_counts(self, glob: Optional[torch.Tensor] = None, logodds_threshold: float = 0.0) -> torch.Tensor:
        """int64 [E,3] = (tp, fp, fn) of the target class for maps thresholded at log-odds > ``logodds_threshold`` (0 <=> the
        reference's p > 0.5, utils/utils.py:64-76).  Thresholds +-1e-5 leave out / take in the exactly-cancelled cells, whose class
        is rounding noise in the reference: the counts under those two are exact integers."""
        env = self.env
        glob = env.glob if glob is None else glob
        counts = torch.zeros(self.E, 3, dtype=torch.int64, device=self.device)
        env.ctx.call("ippm_f1_counts", env._p(glob), env._p(env.truth), 1, float(logodds_threshold), _ffi.ptr(counts), self.E, env.stream)
        return counts

    def global_map_with_pending(self) -> torch.Tensor:
        """The global maps with the measurements of the CURRENT positions fused in, as log-odds [E,gx,gy], without touching
        the env.  The env's own global fusion (K5) lags the sensing by one step (it fuses what was published
        before the move); the deployment scripts score the map after fusing the fresh measurements
        (coma_test.py:150-196: ``fuse_map(current_global_map, maps2communicate_list)`` of the new positions)."""
        env = self.env
        glob, ws, sums = env.glob.clone(), env.ws.clone(), env.sums.clone()
        reward = torch.empty_like(env.reward)
        env.ctx.call("ippm_fuse_global_reward", _ffi.ptr(glob), env._p(env.code), env._p(env.rect), env._p(env.pos), _ffi.ptr(ws),
                     _ffi.ptr(sums), _ffi.ptr(reward), self.E, env.stream)
        return glob

    def _fly(self, t: int, policy: str, eps, actions=None, features: bool = False, observed=None) -> torch.Tensor:
        """Step ``t`` of all envs under a named policy -> the step's reward [E,2]: "actor" (the current actor, greedy), "ig" (the greedy
        expected-information-gain planner), "random" (uniform over the valid actions) or "explicit" (``actions`` int [E,N]).
        ``observed`` is called between the observations and the move; ``features``: whether the move builds the critic's state."""
        env = self.env
        obs = env.build_observations(t, features=policy == "actor")
        if observed is not None:
            observed()
        if policy == "actor":
            probs = self._act(obs, eps)
            return env.steps(t, policy=POLICY_ARGMAX, probs=probs.view(self.E, self.N, self.A), features=features)[0]
        if policy == "random":
            return env.steps(t, policy=POLICY_UNIFORM, features=features)[0]
        if policy == "ig":
            actions = env.ig_actions(communication=True)
        return env.steps(t, policy=POLICY_EXPLICIT, actions=actions, features=features)[0]

    def evaluate(self, waves: int = 1, counts_log: Optional[list] = None) -> Dict[str, object]:
        """Greedy (argmax) deployment of the current actor, the reference's coma_test loop for E envs at once: mean return and
        the per-step curves of target entropy and F1.  Index 0 = the prior map, index t+1 = the map holding every
        measurement up to and including the sensing of step t (coma_test.py:84-97,150-196).  ``counts_log`` (a list) receives, per
        scored map, the pair of int64 [E,3] count tensors of f1_counts at log-odds thresholds +1e-5 and -1e-5."""
        returns, team_returns, ent_curves, f1_curves = [], [], [], []

        def log_counts(glob=None):
            if counts_log is not None:
                counts_log.append((self.f1_counts(glob, 1e-5).cpu(), self.f1_counts(glob, -1e-5).cpu()))

        for _ in range(waves):
            env = self.env
            eps_ids = episode_ids(self.first_episode, self.wave, self.E, self.rank, self.world)
            env.reset(eps_ids)
            e0, f0 = self.map_metrics()   # reset senses at the start cells, the global map is still the prior
            log_counts()
            ents, f1s = [e0.mean().item()], [f0.mean().item()]
            ret = torch.zeros(self.E, device=self.device)
            team_ret = torch.zeros(self.E, device=self.device)
            for t in range(self.T):
                reward = self._fly(t, "actor", self.eps, features=True)
                team_ret += reward[:, 0]
                ret += (self.last_agent_reward() if self.deepq else reward)[:, 0]
                pending = self.global_map_with_pending()
                e, f = self.map_metrics(pending)
                log_counts(pending)
                ents.append(e.mean().item())
                f1s.append(f.mean().item())
            self.wave += 1
            returns.append(float(ret.mean()))
            team_returns.append(float(team_ret.mean()))
            ent_curves.append(ents)
            f1_curves.append(f1s)
        mean = lambda rows: [sum(c) / len(c) for c in zip(*rows)]  # noqa: E731
        return {"episode_return": sum(returns) / len(returns), "team_return": sum(team_returns) / len(team_returns),
                "target_entropy": mean(ent_curves), "f1": mean(f1_curves)}

    def returns_on(self, episodes, policy: str = "actor") -> Dict[str, float]:
        """Mean return of ``policy`` over the FIXED ``episodes`` (E ids: same truth, start cells and sensor noise whoever flies them --
        every random stream is keyed by the episode number), the yardstick of the reference's own comparison (coma_test.py:84-97,
        random_baseline.py:91-96, IG_baseline.py:127-148):
          "actor"   the current actor, greedy (argmax of probs * mask: ActorNetwork in "eval" mode, actor/network.py:63-66)
          "random"  uniform over the valid actions
          "ig"      the greedy expected-information-gain planner on the agents' local maps (one team size per context)
        Does not touch the training buffer, the wave counter or epsilon.
        -> mean relative return ("episode_return": what COMA's reward is made of, utils/reward.py:25-40), mean absolute return, and
        the final global maps' mean target-region entropy and F1."""
        if policy not in ("actor", "random", "ig"):
            raise ValueError(f"unknown policy {policy!r}")
        env = self.env
        env.reset(torch.as_tensor(episodes, dtype=torch.int64).reshape(self.E))
        ret = torch.zeros(self.E, device=self.device)
        abs_ret = torch.zeros(self.E, device=self.device)
        for t in range(self.T):
            reward = self._fly(t, policy, self.eps_dev if self.graphs else self.eps)
            ret += reward[:, 0]
            abs_ret += reward[:, 1]
        ent, f1 = self.map_metrics(self.global_map_with_pending())
        return {"episode_return": float(ret.mean()), "absolute_return": float(abs_ret.mean()), "return_std": float(ret.std()),
                "final_target_entropy": float(ent.mean()), "final_f1": float(f1.mean()), "faults": int(env.fault.ne(0).sum())}

    def curves_on(self, episodes, policy: str = "actor", actions=None) -> Dict[str, torch.Tensor]:
        """The per-step curves every comparison script of the reference reports (coma_test.py:84-97,150-196, IG_baseline.py:84-97,
        random_baseline.py, lawn_mower.py), per env, for ``policy`` flown on the FIXED ``episodes`` (E ids): the policies of returns_on
        plus "explicit", which flies ``actions`` (int [T,E,N]).  Like returns_on it does not touch the training buffer, the wave counter
        or epsilon.
          target_entropy [E,T+1], f1 [E,T+1], f1_counts [E,T+1,3,3] ((tp, fp, fn) at log-odds > +1e-5, 0, -1e-5): index 0 = the prior map,
            index t+1 = the map holding every measurement up to the sensing after the move of step t (evaluate()'s convention);
          episode_return [E], absolute_return [E]; actions [T,E,N], what was flown; faults [E] (the steps' fault words, or-ed).
        No map is cloned per step: the env's own global fusion lags the sensing by one step, so the map of index t >= 1 IS ``env.glob``
        right after build_observations(t) has launched step t's fusion -- it is scored there (VecEnv.score_maps), before steps(t) --
        and only the last index needs the pending measurements fused into a copy (global_map_with_pending).  One host
        synchronisation, at the end."""
        if policy not in ("actor", "random", "ig", "explicit"):
            raise ValueError(f"unknown policy {policy!r}")
        env, T, E, N = self.env, self.T, self.E, self.N
        if policy == "explicit":
            if actions is None:
                raise ValueError('curves_on(policy="explicit") needs actions [T,E,N]')
            actions = torch.as_tensor(actions).to(self.device, torch.int32).reshape(T, E, N)
        env.reset(torch.as_tensor(episodes, dtype=torch.int64).reshape(E))
        ret = torch.zeros(E, device=self.device)
        abs_ret = torch.zeros(E, device=self.device)
        faults = torch.zeros(E, dtype=torch.int32, device=self.device)
        flown = torch.empty(T, E, N, dtype=torch.int32, device=self.device)
        scores = [env.score_maps()]            # the prior map
        for t in range(T):
            # (the map of index t is scored between step t's fusion launch and its move)
            reward = self._fly(t, policy, self.eps_dev if self.graphs else self.eps, actions=None if actions is None else actions[t],
                               observed=(lambda: scores.append(env.score_maps())) if t > 0 else None)
            ret += reward[:, 0]
            abs_ret += reward[:, 1]
            faults |= env.fault
            flown[t].copy_(env.action)
        scores.append(env.score_maps(self.global_map_with_pending()))
        out = {"target_entropy": torch.stack([s.target_entropy for s in scores], 1), "f1": torch.stack([s.f1 for s in scores], 1),
               "f1_counts": torch.stack([s.counts for s in scores], 1), "episode_return": ret, "absolute_return": abs_ret,
               "actions": flown, "faults": faults}
        torch.cuda.current_stream(self.device).synchronize()
        return out

    def save_actor(self, path: str):
        """Whole-module pickle of the actor, the reference's checkpoint format (coma_mission.py:425-451)."""
        from .checkpoint import save_actor
        save_actor(self.actor, path)

    # ---- trainer state: stop a run between two rounds, continue it bit for bit ------------------------------------------------------------
    STATE_FORMAT = 1
    SWITCHES = tuple(switches.TABLE)

    def _state_modules(self):
        return {"actor": self.actor, "critic": self.critic, "target_critic": self.critic_learner.target_critic,
                "frozen_target": self.frozen_target}

    def _state_optimizers(self):
        return {"actor": self.actor_learner.optimizer, "critic": self.critic_learner.optimizer}

    def fingerprint(self) -> Dict[str, object]:
        """What a saved state must agree on with the trainer that loads it: the sizes, what numbers the episodes, and the two switches
        whose state does not carry over (``adam``: the optimizer implementation; ``graphs``: the capturable Adam's arithmetic)."""
        n_active = self.env.n_active
        return {"n_envs": self.E, "n_agents": self.N, "n_actions": self.A, "T": self.T, "waves_per_update": self.waves_per_update,
                "quirks": self.quirks, "philox_seed": self.philox_seed, "first_episode": self.first_episode, "rank": self.rank,
                "world": self.world, "mission_type": str(self.params["experiment"]["missions"].get("type")),
                "team_sizes": None if n_active is None else [int(v) for v in n_active.tolist()],
                "adam": self.adam, "graphs": self.graphs}

    def state_dict(self) -> Dict[str, object]:
        """Everything a later round reads, as CPU tensors, numbers and strings (synchronises): the parameters of the actor, the critic,
        the learner's target network and the construction-time target copy; both optimizers' ``state_dict()`` (torch.optim.Adam's
        format from either implementation); the counters; the device generator's state (what shuffle="torch" draws from; shuffle="native"
        has none to keep, its round counter is ``train_step``); the fingerprint and the switch values."""
        cpu = lambda x: _map_tensors(x, lambda t: t.detach().to("cpu", copy=True))  # noqa: E731
        return {"format": self.STATE_FORMAT, "fingerprint": self.fingerprint(),
                "switches": {k: getattr(self, k) for k in self.SWITCHES},
                "modules": {k: cpu(dict(m.state_dict())) for k, m in self._state_modules().items()},
                "optimizers": {k: cpu(o.state_dict()) for k, o in self._state_optimizers().items()},
                "counters": {"train_step": int(self.train_step), "wave": int(self.wave), "eval_wave": int(self.eval_wave),
                             "step_replays": int(self.step_replays), "eps": float(self.eps),
                             "shuffle_round": int(self.train_step)},
                "rng": torch.cuda.get_rng_state(self.device).clone()}

    def load_state_dict(self, state: Dict[str, object]):
        """Continue from ``state`` (of ``state_dict()``): between rounds only, on a trainer whose fingerprint agrees.  Everything is written
        IN PLACE (``copy_`` into the parameters, the optimizers' existing state tensors and the native Adam's blob), so graphs captured
        before the load stay valid; modules and optimizer states are checked before the first write, so a state that does not fit leaves
        the trainer as it was.  The device generator's state is restored for shuffle="torch" only.  Afterwards ``eps_dev`` is refilled, every inference pack is repacked (the parameters' version counters
        have advanced) and the device round counter of shuffle="native" is set."""
        if self.filled != 0:
            raise _ffi.IppmError(f"load_state_dict: the buffer holds {self.filled} wave(s): a state is loaded between rounds (filled == 0)")
        if state.get("format") != self.STATE_FORMAT:
            raise _ffi.IppmError(f"load_state_dict: not a trainer state of format {self.STATE_FORMAT}")
        mine, theirs = self.fingerprint(), state["fingerprint"]
        for k, v in mine.items():
            if k not in theirs or theirs[k] != v:
                raise _ffi.IppmError(f"load_state_dict: the state's {k} is {theirs.get(k)!r}, this trainer's {v!r}")
        modules = self._state_modules()
        for name, module in modules.items():      # (checked first: nothing is written when a tensor does not fit)
            saved = state["modules"][name]
            own = module.state_dict()
            if set(saved) != set(own) or any(tuple(saved[k].shape) != tuple(own[k].shape) for k in own):
                raise _ffi.IppmError(f"load_state_dict: the state's {name} does not have this trainer's tensors")
        for name, opt in self._state_optimizers().items():
            _check_optimizer_state(name, opt, state["optimizers"][name])
        with torch.no_grad():
            for name, module in modules.items():
                saved = state["modules"][name]
                for k, t in list(module.named_parameters()) + list(module.named_buffers()):
                    t.copy_(saved[k])
        for name, opt in self._state_optimizers().items():
            _load_optimizer_in_place(opt, state["optimizers"][name])
        c = state["counters"]
        self.train_step, self.wave = int(c["train_step"]), int(c["wave"])
        self.eval_wave, self.step_replays = int(c["eval_wave"]), int(c["step_replays"])
        self.eps = float(c["eps"])
        self.eps_dev.fill_(self.eps)
        self._order.load(c, state.get("rng"))
        if self._native is not None and self._native.module is self.actor:
            self._native.sync()
        if self.critic_inference == "native":
            self._native_critic.sync()
            self.native_target().sync()

    def save_state(self, path: str):
        """``state_dict()`` as a plain ``torch.save`` (loads under ``torch.load(weights_only=True)``); between rounds only."""
        if self.filled != 0:
            raise _ffi.IppmError(f"save_state: the buffer holds {self.filled} wave(s): a state is saved between rounds (filled == 0)")
        torch.save(self.state_dict(), path)

    def load_state(self, path: str):
        """``load_state_dict`` of a file written by ``save_state``."""
        self.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))


def _map_tensors(x, fn):
    """``x`` with ``fn`` applied to every tensor inside its dicts, lists and tuples (the containers become plain dicts, lists, tuples)."""
    if isinstance(x, torch.Tensor):
        return fn(x)
    if isinstance(x, dict):
        return {k: _map_tensors(v, fn) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_map_tensors(v, fn) for v in x)
    return x


def _saved_entries(opt, saved):
    """{id(parameter): its entry of ``saved["state"]`` or None} for the parameters of ``opt``'s one group."""
    params = opt.param_groups[0]["params"]
    return {id(p): saved["state"].get(k) for p, k in zip(params, saved["param_groups"][0]["params"])}


def _check_optimizer_state(name, opt, saved):
    """Raises unless ``saved`` (torch.optim.Adam's format) fits ``opt``: one group over as many parameters, moments of the parameters'
    shapes, and -- for a torch optimizer that has stepped, which is written in place -- entries for exactly the parameters it has stepped."""
    params = opt.param_groups[0]["params"]
    groups = saved["param_groups"]
    if len(groups) != 1 or len(groups[0]["params"]) != len(params):
        raise _ffi.IppmError(f"load_state_dict: the {name} optimizer's state is over another parameter list")
    entries = _saved_entries(opt, saved)
    for p in params:
        e = entries[id(p)]
        if e is not None and any(k not in e or tuple(e[k].shape) != tuple(p.shape) for k in ("exp_avg", "exp_avg_sq")):
            raise _ffi.IppmError(f"load_state_dict: the {name} optimizer's moments do not have the parameters' shapes")
    if not isinstance(opt, optim_native.NativeAdam) and opt.state:
        want = {i for i, e in entries.items() if e is not None}
        if want and want != {id(p) for p in opt.state}:
            raise _ffi.IppmError(f"load_state_dict: the {name} optimizer's state steps other parameters than this trainer's has stepped")


def _load_optimizer_in_place(opt, saved):
    """``saved`` (checked by ``_check_optimizer_state``) into ``opt`` without replacing a tensor that a captured graph may hold: NativeAdam
    writes views of its blob; a torch optimizer that has stepped gets ``copy_`` into its state tensors; one that never stepped has no state
    tensor anybody could hold, and takes ``load_state_dict``."""
    if isinstance(opt, optim_native.NativeAdam) or not opt.state:
        opt.load_state_dict(saved)
        return
    entries = _saved_entries(opt, saved)
    with torch.no_grad():
        for p, st in opt.state.items():
            e = entries[id(p)]
            for k, v in st.items():
                if torch.is_tensor(v):
                    if e is None:
                        v.zero_()           # (a state saved before the first step: zero moments at step 0 are Adam's initial state)
                    else:
                        v.copy_(e[k])
