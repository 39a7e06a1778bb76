"""Deferred clamp-only fusion ops (ippm_set_clamp_backlog / IPPM_STEP_DEFER_CLAMPS / ippm_settle_clamps): a VecEnv that defers and its
eager twin (defer_clamps=False) fly the same scripted episodes; whenever somebody looks, the maps must be the twin's bit for bit.

The scenario (tests/deferred_clamp_scenario.py; 3 envs x 3 UAVs on 128 x 128, the smallest grid the tile form takes) saturates cells at low
altitude and mixes envs in which everybody hears everybody, nobody hears anybody for a while, and some do; that it leaves owed
out-of-range cells at the looks is checked on the CPU (tests/test_deferred_clamp_cpu.py) and, here, from the counters."""
import numpy as np
import pytest
import torch

from conftest import assert_posteriors
from deferred_clamp_scenario import SEED, STARTS, comm_ranges, oracle_episodes, read_points, scenario_params as _params

pytestmark = pytest.mark.gpu


def make_pair(params=None, **kw):
    from ippmarl.vec_env import VecEnv
    params = _params() if params is None else params
    return (VecEnv(params, 3, philox_seed=SEED, **kw), VecEnv(params, 3, philox_seed=SEED, defer_clamps=False, **kw))


def fly(envs, episodes, reads, build_obs=False):
    """Flies the scripted episode on every env of `envs` in lock step; positions, masks, actions and the deferred clamp's ws state are compared at
    every step (they are never allowed to differ), the maps at the steps in `reads`.  -> rewards [env][T, E, 2]"""
    from ippmarl.vec_env import POLICY_EXPLICIT
    ora = oracle_episodes(tuple(episodes))
    T = envs[0].d.budget + 1
    for env in envs:
        env.reset(list(episodes), start_positions=torch.tensor(STARTS, dtype=torch.int32))
    rewards = [[] for _ in envs]
    for t in range(T):
        acts = torch.tensor(np.array([ora[e]["log"][t]["actions"] for e in range(3)]), dtype=torch.int32)
        for k, env in enumerate(envs):
            env.comm_range.copy_(torch.tensor(comm_ranges(t), dtype=torch.float32))
            if build_obs:
                env.build_observations(t)
            r, _, _ = env.steps(t, policy=POLICY_EXPLICIT, actions=acts, features=build_obs)
            rewards[k].append(r.clone())
        a, b = envs[0], envs[-1]
        for e in range(3):
            assert np.array_equal(a.pos[e].cpu().numpy(), ora[e]["log"][t]["next_positions"]), (t, e)
        assert torch.equal(a.pos, b.pos) and torch.equal(a.mask, b.mask) and torch.equal(a.action, b.action), t
        assert torch.equal(a.ws[..., :6], b.ws[..., :6]) and torch.equal(a.rect, b.rect), f"deferred-clamp state differs at t={t}"
        if t in reads:
            assert torch.equal(a.local, b.local), f"local maps differ at the look after step {t}"
            assert torch.equal(a.glob, b.glob), f"global maps differ at the look after step {t}"
    return [torch.stack(r).cpu().numpy() for r in rewards]


def check_not_vacuous(deferring, twin):
    cd, ce = deferring.counters(), twin.counters()
    fused_d = cd["fuse_local_cells"] + cd["fuse_global_cells"]
    fused_e = ce["fuse_local_cells"] + ce["fuse_global_cells"]
    print(f"fusion cells: deferring {fused_d}, twin {fused_e}; cells changed by the settles: {cd['settled_cells']}")
    assert fused_d < fused_e, "the deferring env's fusions touched no fewer cells: nothing was deferred"
    assert cd["settled_cells"] >= 1, "no settle changed a cell: the scenario leaves nothing owed at its looks"
    assert ce["settled_cells"] == 0 and cd["work_list_rejects"] == 0


@pytest.mark.parametrize("layout", ["rows", "tiles"])      # (a) and (d)
def test_whole_episode_unobserved_then_one_look(layout):
    episodes = (5, 6, 7)
    env, twin = make_pair(track_area=False, map_layout=layout)
    assert env.backlog is not None and twin.backlog is None and env.tiled == (layout == "tiles")
    T = env.d.budget + 1
    r_d, r_e = fly([env, twin], episodes, reads=read_points("end", T))
    np.testing.assert_allclose(r_d, r_e, rtol=0, atol=1e-5)
    check_not_vacuous(env, twin)
    ora = oracle_episodes(episodes)
    p_loc, p_glob = env.posterior_local().cpu().numpy(), env.posterior_global().cpu().numpy()
    for e in range(3):
        assert_posteriors(p_glob[e], ora[e]["global_map"], strict=True, msg=f"global map of env {e}")
        assert_posteriors(p_loc[e], ora[e]["local_maps"], strict=True, msg=f"local maps of env {e}")
        for t in range(T):
            np.testing.assert_allclose(float(r_d[t, e, 0]), ora[e]["log"][t]["relative_reward"], rtol=1e-5, atol=6e-6)


def test_a_look_every_four_steps():       # (b)
    env, twin = make_pair(track_area=False)
    T = env.d.budget + 1
    r_d, r_e = fly([env, twin], (5, 6, 7), reads=read_points("every4", T))
    np.testing.assert_allclose(r_d, r_e, rtol=0, atol=1e-5)
    check_not_vacuous(env, twin)


def test_second_episode_inherits_no_backlog():      # (c)
    env, twin = make_pair(track_area=False)
    T = env.d.budget + 1
    fly([env, twin], (5, 6, 7), reads=set())               # ends owing: nobody looked
    assert env._owing
    backlog = env.backlog.view(3, 4, -1)
    assert bool((backlog[..., 0] != 0).any()), "the first episode left nothing owed: the reset has nothing to forget"
    r_d, r_e = fly([env, twin], (8, 9, 10), reads={0, T - 1})
    np.testing.assert_allclose(r_d, r_e, rtol=0, atol=1e-5)
    env.reset([5, 6, 7], start_positions=torch.tensor(STARTS, dtype=torch.int32))
    assert not bool(env.backlog.view(3, 4, -1)[..., :3].any()) and not env._owing


@pytest.mark.parametrize("kw,over", [(dict(track_area=False), dict(mapping__prior=0.4)), (dict(track_area=True), dict())])    # (e)
def test_deferral_is_not_taken_where_it_does_not_apply(kw, over):
    from ippmarl.vec_env import VecEnv
    params = _params(**over)
    env = VecEnv(params, 3, philox_seed=SEED, **kw)
    twin = VecEnv(params, 3, philox_seed=SEED, defer_clamps=False, **kw)
    assert env.backlog is None and not env._defer
    # (the scripted actions come from the prior-0.5 oracle run: positions do not depend on the prior)
    fly([env, twin], (5, 6, 7), reads={env.d.budget}, build_obs=kw["track_area"])
    cd, ce = env.counters(), twin.counters()
    assert cd == ce and cd["settled_cells"] == 0 and cd["fuse_local_cells"] > 0
