"""GPU tests of the DeepQ per-agent information-gain rewards (ippm_agent_rewards; coma_wrapper.py:113-171): the drop-in wrapper
against episodes recorded from the reference, the batched VecEnv / SplitVecEnv against the exact oracle under the production
randomness, and the launch's effect on everything else (none)."""
import numpy as np
import pytest

import ipp_oracle as O
from configs import make_params
from conftest import unpack_correctness
from test_deepq_golden import agent_rewards, deepq_params

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
RTOL = 1e-5


@pytest.mark.parametrize("tag", ["episode_deepq_small_e5", "episode_deepq_small27_e6"])
def test_dropin_deepq_replays_reference_episode(golden, tag, monkeypatch):
    """EpisodeGenerator.execute(...) with mission type DeepQ and the recorded randomness: every agent's transition carries ITS
    reward, the generator sums the last agent's."""
    from ippmarl.batch_memory import BatchMemory
    from ippmarl.coma_wrapper import COMAWrapper, ReplayHooks
    from ippmarl.mapping.grid_maps import GridMap
    from ippmarl.missions.episode_generator import EpisodeGenerator
    from ippmarl.sensors import Sensor
    from ippmarl.sensors.models import SensorModel
    fx = golden(tag)
    params = deepq_params(tag)
    n = params["experiment"]["missions"]["n_agents"]
    T = params["experiment"]["constraints"]["budget"] + 1
    corr = unpack_correctness(fx)
    draws = iter(fx["comm_draws"])
    monkeypatch.setattr(np.random, "random_sample", lambda *a, **k: next(draws))
    wrapper = COMAWrapper(params, None)
    wrapper.replay = ReplayHooks(correctness=lambda agent_id, stage: corr[stage * n + agent_id],
                                 action=lambda agent_id, t: int(fx["actions"][t, agent_id]))
    memory = BatchMemory(params, wrapper)
    grid_map = GridMap(params)
    generator = EpisodeGenerator(params, None, grid_map, Sensor(SensorModel(), grid_map))
    (episode_return, episode_rewards, absolute_return, simulated_map, memory, agent_positions, t_last, eps, agent_actions,
     agent_altitudes) = generator.execute(int(fx["episode"]), memory, wrapper, "train")
    assert np.array_equal(simulated_map.astype(np.uint8), fx["truth"])
    assert np.array_equal(np.array(agent_positions), fx["positions"])           # [T+1, n, 3], bit-exact
    assert np.array_equal(np.array(agent_actions), fx["actions"])
    assert t_last == T - 1 and memory.size() == T * n
    got = np.array([[memory.transitions[a][t].reward for a in range(n)] for t in range(T)])
    np.testing.assert_allclose(got, fx["rewards"], rtol=RTOL, atol=1e-6)
    assert all(memory.transitions[a][t].done == bool(fx["done"][t, a]) for a in range(n) for t in range(T))
    np.testing.assert_allclose(episode_rewards, fx["episode_rewards"], rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(episode_return, fx["episode_return"], rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(absolute_return, fx["abs_return"], rtol=RTOL, atol=1e-6)


def oracle_deepq_episode(params, episode, seed):
    """The exact oracle under the production randomness (Philox flips / uniform valid actions / comm draws), with every step's
    DeepQ rewards and sums: [(rec, rewards [n, 2], sums [n, 2])]."""
    holder = {}

    def correctness(i, s, shape):
        ag_pos = holder["ep"].agents[i]["position"]
        _, fc = O.project_field_of_view(holder["ep"].d, ag_pos)
        return O.philox_correctness(seed, episode, i, s, fc, holder["ep"].d.gy, O.noise_of_altitude(ag_pos[2]))

    ep = O.OracleEpisode(params, episode, correctness,
                         lambda i, t, mask, obs: O.uniform_valid_action(O.philox_action_word(seed, episode, i, t), mask),
                         comm_draw=lambda i, j, t: O.philox_comm_draw(seed, episode, i, j, t), build_features=False, exact=True)
    holder["ep"] = ep
    out = []
    for t in range(ep.d.budget + 1):
        rec = ep.step(t)
        r, s = agent_rewards(ep, rec)
        out.append((rec, r, s))
    return out


def _world(x, y, **over):
    return dict(environment__x_dim=x, environment__y_dim=y, **over)


NOISE_FREE = dict(experiment__constraints__min_altitude=15, experiment__constraints__max_altitude=20,
                  experiment__constraints__num_actions=27, experiment__uav__communication_range=10)
# name, overrides, envs, map layouts
CASES = {
    "small": ("small", {}, 4, ("rows", "tiles")),
    "failures6": ("small", dict(experiment__uav__failure_rate=0.35, experiment__uav__fix_range=False, experiment__missions__n_agents=6), 3,
                  ("rows", "tiles")),
    "actions27": ("small", dict(experiment__missions__n_agents=3, experiment__constraints__num_actions=27), 3, ("rows", "tiles")),
    "prior03": ("small", dict(mapping__prior=0.3), 3, ("rows",)),            # every cell shifts: the whole-grid walk
    "noise_free": ("small", NOISE_FREE, 2, ("rows",)),                      # 20 m: +-inf measurement log-odds
    "rect128x256": ("small", _world(50, 100), 3, ("rows", "tiles")),
    "c2": ("c2", {}, 3, ("rows", "tiles")),
    "narrow34": ("default", dict(sensor__pixel__number_x=4, sensor__pixel__number_y=4, experiment__missions__n_agents=3), 3, ("rows",)),
    # one cell per lane (grid_y < 44) with the whole-grid walk of prior != 0.5
    "narrow34_prior03": ("default", dict(sensor__pixel__number_x=4, sensor__pixel__number_y=4, experiment__missions__n_agents=3,
                                         mapping__prior=0.3), 3, ("rows",)),
    # 16-byte groups on rows that are not a multiple of 4 wide (51 cells): groups straddle rows, the map's last group runs past its end
    "odd51": ("default", dict(sensor__pixel__number_x=6, sensor__pixel__number_y=6, experiment__missions__n_agents=3), 3, ("rows",)),
    "odd51_prior03": ("default", dict(sensor__pixel__number_x=6, sensor__pixel__number_y=6, experiment__missions__n_agents=3,
                                      mapping__prior=0.3), 2, ("rows",)),
}
PARAMS = [(k, layout) for k, case in CASES.items() for layout in case[3]]


def check_deepq_batch(name, over, n_envs, map_layout="rows", team_sizes=None, parts=0, tracked=False, seed=0x5EED0DEE, first_episode=13):
    """Every step of a batch under the production randomness against the exact oracle: agent_reward [E,N,2] at the reward tolerances
    of the COMA reward, agent_sums (S1_i, S2_i) against the oracle's reward_sums, and T = sums[e][2] at the call point against a fresh
    ippm_weighted_entropy of K."""
    from ippmarl.vec_env import POLICY_UNIFORM, SplitVecEnv, VecEnv
    params = make_params(name, **over)
    if parts:
        env = SplitVecEnv(params, n_envs, parts=parts, philox_seed=seed, map_layout=map_layout, team_sizes=team_sizes, agent_rewards=True)
    else:
        env = VecEnv(params, n_envs, philox_seed=seed, track_area=tracked, map_layout=map_layout, team_sizes=team_sizes,
                     agent_rewards=True)
    assert env.tiled == (map_layout == "tiles")
    eps = [first_episode + 5 * k for k in range(n_envs)]
    env.reset(eps)
    N = env.d.n_agents
    teams = [N] * n_envs if team_sizes is None else list(team_sizes)
    oracles = [oracle_deepq_episode(make_params(name, **dict(over, experiment__missions__n_agents=teams[e])), ep, seed)
               for e, ep in enumerate(eps)]
    noise_free = any(z not in (5, 10, 15) for z in env.d.altitudes)
    s_scale = 1e-6 if env.d.prior != 0.5 else (2e-7 if noise_free else 2e-8)
    for t in range(env.d.budget + 1):
        if parts:
            env.steps(t, policy=POLICY_UNIFORM)
        elif tracked:
            env.build_observations(t)
            env.steps(t, policy=POLICY_UNIFORM)
        else:
            env.steps(t, policy=POLICY_UNIFORM, features=False)
        got = env.agent_reward.cpu().numpy()
        got_s = env.agent_sums.cpu().numpy()
        sums = env.sums.cpu().numpy()
        pos = env.pos.cpu().numpy()
        if not parts:   # T at the call point is the weighted entropy of K (a fresh float32-per-cell sum: 1e-5 when every cell counts)
            fresh = torch.zeros(n_envs, dtype=torch.float64, device=env.device)
            env.ctx.call("ippm_weighted_entropy", env._p(env.glob), None, 1, env._p(fresh), n_envs, env.stream)
            np.testing.assert_allclose(sums[:, 2], fresh.cpu().numpy(), rtol=2e-6 if env.d.prior == 0.5 else 2e-5, err_msg=f"T t={t}")
        for e, orc in enumerate(oracles):
            rec, want, want_s = orc[t]
            n = teams[e]
            t_exact = O.reward_sums(O.Derived(params), rec["global_map"], rec["global_map"])[1]   # sum w(K) H(K) of the exact oracle
            np.testing.assert_allclose(sums[e, 2], t_exact, rtol=RTOL, atol=1e-6 + s_scale * abs(t_exact), err_msg=f"T t={t} e={e}")
            assert np.array_equal(pos[e, :n], rec["next_positions"]), (t, e)
            np.testing.assert_allclose(got[e, :n, 0], want[:, 0], rtol=RTOL, atol=1e-6 + RTOL * 0.5, err_msg=f"relative t={t} e={e}")
            np.testing.assert_allclose(got[e, :n, 1], want[:, 1], rtol=RTOL, atol=1e-6 + RTOL * 0.17, err_msg=f"absolute t={t} e={e}")
            for i in range(n):
                np.testing.assert_allclose(got_s[e, i], want_s[i], rtol=RTOL, atol=1e-6 + s_scale * abs(want_s[i, 1]),
                                           err_msg=f"sums t={t} e={e} i={i}")
            assert not got[e, n:].any() and not got_s[e, n:].any(), (t, e)   # agents that do not fly: 0


@pytest.mark.parametrize("case,layout", PARAMS)
def test_agent_rewards_match_oracle(case, layout):
    name, over, n_envs, _ = CASES[case]
    check_deepq_batch(name, over, n_envs, map_layout=layout)


@pytest.mark.parametrize("layout", ["rows", "tiles"])
def test_agent_rewards_mixed_teams_match_oracle(layout):
    check_deepq_batch("small", dict(experiment__missions__n_agents=6), 6, map_layout=layout, team_sizes=[1, 2, 3, 6, 4, 5])


def test_agent_rewards_split_env_match_oracle():
    check_deepq_batch("small", {}, 5, parts=2)


def test_agent_rewards_tracked_step_match_oracle():
    """With the network inputs built (build_observations + steps(features=True)): the same rewards."""
    check_deepq_batch("small", {}, 3, tracked=True)


def test_agent_rewards_follow_the_mission_type():
    from ippmarl.vec_env import VecEnv
    assert VecEnv(make_params("small", experiment__missions__type="DeepQ"), 1).agent_reward is not None
    coma = VecEnv(make_params("small"), 1)
    assert coma.agent_rewards is False and coma.agent_reward is None
    assert VecEnv(make_params("small"), 1, agent_rewards=True).agent_reward.shape == (1, 4, 2)


@pytest.mark.parametrize("layout", ["rows", "tiles"])
def test_agent_rewards_change_nothing_else(layout):
    """Same seeds with agent rewards on and off at BASELINE config 2's shape (1024 envs): every other output is identical."""
    from ippmarl.vec_env import POLICY_UNIFORM, VecEnv
    params = make_params("c2")
    E = 1024
    envs = [VecEnv(params, E, philox_seed=0xD11, track_area=True, map_layout=layout, agent_rewards=on) for on in (False, True)]
    for env in envs:
        assert env.tiled == (layout == "tiles")
        env.reset(list(range(40, 40 + E)))
    off, on = envs
    assert off.agent_reward is None
    for t in range(params["experiment"]["constraints"]["budget"] + 1):
        outs = []
        for env in envs:
            obs = env.build_observations(t).clone()
            reward, _, state = env.steps(t, policy=POLICY_UNIFORM)
            outs.append((obs, state.clone(), reward.clone()))
        for a, b in zip(*outs):
            assert torch.equal(a, b), t
        # (not the area sums: float64 atomics of several workgroups, whose order varies from run to run with or without the launch)
        for k in ("local", "glob", "pos", "mask", "action", "sums", "comm", "rect", "code"):
            assert torch.equal(getattr(off, k), getattr(on, k)), (t, k)
        assert torch.isfinite(on.agent_reward).all(), t


# ---- COMATrainer with mission type DeepQ ---------------------------------------------------------------------------------------

def _step_round(tr):
    """One training wave stepped by hand (what rollout("train") does), checking after every step that the buffer row is the env's
    per-agent reward and that the returns follow the reference: the last flying agent's reward, the team reward beside it."""
    from ippmarl.parallel import episode_ids
    from ippmarl.vec_env import POLICY_SAMPLE
    env = tr.env
    env.reset(episode_ids(tr.first_episode, tr.wave, tr.E, tr.rank, tr.world))
    tr.ret.zero_(), tr.abs_ret.zero_(), tr.team_ret.zero_()
    teams = [tr.N] * tr.E if env.n_active is None else env.n_active.tolist()
    ret = np.zeros(tr.E)
    team = np.zeros(tr.E)
    for t in range(tr.T):
        tr._rollout_step(t, 0, POLICY_SAMPLE, True, tr.eps)
        ar = env.agent_reward.cpu().numpy()
        assert torch.equal(tr.buf_reward[0, t], env.agent_reward[..., 0]), t
        ret += np.array([ar[e, teams[e] - 1, 0] for e in range(tr.E)], dtype=np.float32)
        team += env.reward[:, 0].cpu().numpy()
    np.testing.assert_allclose(tr.ret.cpu().numpy(), ret, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(tr.team_ret.cpu().numpy(), team, rtol=1e-5, atol=1e-5)
    tr.wave += 1
    tr.filled = 1
    return teams


def _check_td_chains(tr, params, chains):
    T = tr.T
    td, _ = tr.td_targets()
    td = td.view(1, T, tr.E, tr.N).cpu().numpy()
    rew = tr.buf_reward[:1].cpu().numpy()                 # [1, T, E, N]: each agent's own rewards
    g, lam = params["networks"]["gamma"], params["networks"]["lambda"]
    dones = np.zeros(T, dtype=bool)
    dones[T - 1] = True
    for e, i in chains:
        with torch.no_grad():
            q, _ = tr.frozen_target(tr.buf_state[0, :, e, i].reshape(T, 11, 11, 12).contiguous())
        q_sel = q.gather(1, tr.buf_action[0, :, e, i].reshape(-1, 1).long()).view(-1).cpu().numpy()
        want, _ = O.td_lambda_targets(rew[0, :, e, i], dones, q_sel, g, lam)
        np.testing.assert_allclose(td[0, :, e, i], want, rtol=1e-5, atol=2e-6, err_msg=f"chain e={e} i={i}")


def test_trainer_deepq_buffer_and_td_chains():
    """COMATrainer with mission type DeepQ: the reward buffer [W,T,E,N] is env.agent_reward, TD(lambda) runs on each (env, agent)
    chain's own rewards (against the oracle's restatement), the return is the last agent's reward summed, and a round updates."""
    from ippmarl.trainer import COMATrainer
    params = make_params("small", experiment__missions__type="DeepQ")
    torch.manual_seed(3)
    tr = COMATrainer(params, n_envs=5, first_episode=3)
    assert tr.deepq and tuple(tr.buf_reward.shape) == (1, tr.T, 5, tr.N)
    _step_round(tr)
    rew = tr.buf_reward[0].cpu().numpy()
    assert (np.ptp(rew, axis=2) > 0).any()                # the agents' chains really differ
    _check_td_chains(tr, params, [(0, 0), (0, 3), (2, 1), (4, 2), (4, 3)])
    stats = tr.update()
    assert stats["transitions"] == tr.T * 5 * tr.N and np.isfinite(stats["critic_loss"]) and np.isfinite(stats["actor_loss"])
    s = tr.rollout("train")
    assert s["faults"] == 0 and np.isfinite(s["episode_return"]) and s["episode_return"] != s["team_return"]
    ev = tr.evaluate(1)
    assert np.isfinite(ev["episode_return"]) and np.isfinite(ev["team_return"])


def test_trainer_deepq_mixed_team_sizes():
    """DeepQ with team sizes 1 .. 4 of 4 UAVs: flying agents' rows are their own rewards, the others' are 0 and stay out of every
    minibatch; the return sums each env's LAST FLYING agent's reward."""
    from ippmarl.trainer import COMATrainer
    params = make_params("small", experiment__missions__type="DeepQ")
    teams = [1, 2, 3, 4, 4, 2]
    torch.manual_seed(5)
    tr = COMATrainer(params, n_envs=len(teams), first_episode=3, team_sizes=teams)
    _step_round(tr)
    rew = tr.buf_reward[0].cpu().numpy()
    for e, n_e in enumerate(teams):
        assert not rew[:, e, n_e:].any()
    assert len(tr.valid_transitions(1)) == sum(teams) * tr.T
    _check_td_chains(tr, params, [(0, 0), (1, 1), (2, 2), (3, 3), (5, 1)])
    out = tr.update()
    assert out["transitions"] == sum(teams) * tr.T and np.isfinite(out["critic_loss"]) and np.isfinite(out["actor_loss"])


def test_trainer_deepq_recorded_round_equals_eager_round():
    """COMATrainer(graphs=True).capture_graphs() with DeepQ: the recorded rollout steps include the per-agent reward launch, so a
    replayed wave fills the [W,T,E,N] buffer and the returns as the eager wave does (same weights, same seeds)."""
    from ippmarl.trainer import COMATrainer
    params = make_params("small", experiment__missions__type="DeepQ")

    def trainer():
        torch.manual_seed(11)
        return COMATrainer(params, n_envs=4, first_episode=3, graphs=True)

    eager, rec = trainer(), trainer()
    for tr in (eager, rec):
        torch.manual_seed(12)
        tr.rollout("train")
        tr.update()
    with torch.no_grad():   # identical training state (weights, Adam moments, target net) before the compared round
        for net in ("actor", "critic"):
            for p_dst, p_src in zip(getattr(rec, net).parameters(), getattr(eager, net).parameters()):
                p_dst.copy_(p_src)
        for learner in ("actor_learner", "critic_learner"):
            src_opt, dst_opt = getattr(eager, learner).optimizer, getattr(rec, learner).optimizer
            for g_src, g_dst in zip(src_opt.param_groups, dst_opt.param_groups):
                for p_src, p_dst in zip(g_src["params"], g_dst["params"]):
                    for k, v in src_opt.state.get(p_src, {}).items():
                        dst_opt.state[p_dst][k].copy_(v)
        for p_dst, p_src in zip(rec.critic_learner.target_critic.parameters(), eager.critic_learner.target_critic.parameters()):
            p_dst.copy_(p_src)
    rec.capture_graphs()
    stats = []
    for tr in (eager, rec):
        torch.manual_seed(20)
        stats.append(tr.rollout("train"))
    assert torch.equal(eager.buf_action, rec.buf_action) and torch.equal(eager.buf_mask, rec.buf_mask)
    assert torch.equal(eager.env.glob, rec.env.glob)
    torch.testing.assert_close(eager.buf_reward, rec.buf_reward, rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(eager.env.agent_reward, rec.env.agent_reward, rtol=1e-5, atol=2e-6)
    for k in ("episode_return", "absolute_return", "team_return"):
        np.testing.assert_allclose(stats[0][k], stats[1][k], rtol=1e-5, atol=1e-5, err_msg=k)
    for tr in (eager, rec):
        out = tr.update()
        assert np.isfinite(out["critic_loss"]) and np.isfinite(out["actor_loss"])
