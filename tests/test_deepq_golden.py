"""DeepQ mission type (coma_wrapper.py:113-171): the oracle composition the per-agent reward kernel is held to, against episodes
recorded from the reference itself (tools/make_golden_deepq.py).  CPU only.

Agent i's reward at step t is get_global_reward(K, fuse_map(K, [m_i])) with K the step's global map (after its global fusion) and m_i
agent i's measurement at its new position; the wrapper returns the LAST agent's pair, which EpisodeGenerator sums into the return."""
import numpy as np
import pytest

import ipp_oracle as O
from configs import make_params
from conftest import unpack_correctness

RTOL = 1e-5

DEEPQ_EPISODES = {
    # 4 UAVs on the small grid, prior 0.5
    "episode_deepq_small_e5": dict(name="small", over={}),
    # 3 UAVs, 27 actions, link failures, per-episode comm range
    "episode_deepq_small27_e6": dict(name="small", over=dict(experiment__missions__n_agents=3, experiment__uav__fix_range=False,
                                                             experiment__uav__failure_rate=0.3, experiment__constraints__num_actions=27)),
    # mapping.prior 0.3: fusing m_i shifts every cell of K
    "episode_deepq_prior03_e4": dict(name="small", over=dict(mapping__prior=0.3, experiment__missions__n_agents=3)),
}


def deepq_params(tag):
    case = DEEPQ_EPISODES[tag]
    return make_params(case["name"], experiment__missions__type="DeepQ", **case["over"])


def agent_rewards(ep, rec):
    """[n, 2] DeepQ rewards (relative, absolute) and [n, 2] sums (S1, S2) of the step just taken by ``ep`` (right after ep.step(t))."""
    d, K = ep.d, rec["global_map"]
    out, sums = [], []
    for i in range(d.n_agents):
        after = O.fuse_map(d, K, [ep.agents[i]["map2communicate"]], i, "global")
        _, rel, ab = O.global_reward(d, K, after, ep.truth)
        out.append((rel, ab))
        sums.append(O.reward_sums(d, K, after))
    return np.array(out), np.array(sums)


def replay_deepq(fx, params, exact=False):
    """The oracle driven with the randomness the reference consumed: (log, per-agent rewards [T, n, 2])."""
    d = O.Derived(params)
    n, T = d.n_agents, d.budget + 1
    corr = unpack_correctness(fx)
    comm = fx["comm_draws"]
    ep = O.OracleEpisode(params, int(fx["episode"]), correctness=lambda i, s, shape: corr[s * n + i].reshape(shape),
                         choose_action=lambda i, t, mask, obs: fx["actions"][t, i],
                         comm_draw=lambda i, j, t: comm[(t * n + i) * n + j], build_features=False, exact=exact)
    log, rewards = [], []
    for t in range(T):
        rec = ep.step(t)
        log.append(rec)
        rewards.append(agent_rewards(ep, rec)[0])
    return log, np.array(rewards)


@pytest.mark.parametrize("tag", list(DEEPQ_EPISODES))
def test_deepq_fixture_replays_in_reference_mode(golden, tag):
    fx = golden(tag)
    log, rewards = replay_deepq(fx, deepq_params(tag))
    for t, rec in enumerate(log):
        assert np.array_equal(rec["positions"], fx["positions"][t]), t
        assert np.array_equal(rec["next_positions"], fx["positions"][t + 1]), t
    np.testing.assert_array_equal(rewards[..., 0], fx["rewards"])            # the reference's own dtype flow: identical
    np.testing.assert_allclose(rewards[:, -1, 0].sum(), fx["episode_return"], rtol=1e-12)
    np.testing.assert_allclose(rewards[:, -1, 1].sum(), fx["abs_return"], rtol=1e-12)


@pytest.mark.parametrize("tag", list(DEEPQ_EPISODES))
def test_deepq_fixture_bookkeeping(golden, tag):
    """The wrapper hands the LAST agent's reward to EpisodeGenerator, and the agents' rewards really differ."""
    fx = golden(tag)
    np.testing.assert_array_equal(fx["episode_rewards"], fx["rewards"][:, -1])
    np.testing.assert_allclose(fx["rewards"][:, -1].sum(), fx["episode_return"], rtol=1e-12)
    assert (np.ptp(fx["rewards"], axis=1) > 0).all()    # (under COMA every agent of a step gets the team reward)
    assert fx["done"][-1].all() and not fx["done"][:-1].any()


@pytest.mark.parametrize("tag", ["episode_deepq_small_e5", "episode_deepq_small27_e6"])
def test_deepq_fixture_exact_mode(golden, tag):
    """The exact-float64 oracle (what the device is held to) against the recording at prior 0.5: 1e-5."""
    fx = golden(tag)
    _, rewards = replay_deepq(fx, deepq_params(tag), exact=True)
    np.testing.assert_allclose(rewards[..., 0], fx["rewards"], rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(rewards[:, -1, 0].sum(), fx["episode_return"], rtol=RTOL)
