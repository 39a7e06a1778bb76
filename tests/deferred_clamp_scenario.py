"""The scripted episodes that tests/test_hip_deferred_clamp.py flies (3 envs x 3 UAVs, 128 x 128), and their oracle runs.

As test_saturation_and_deferred_clamp arranges it: the agents descend to 5 m (noise 0.01: a cell is past the clip bound at its third look)
and shuttle between two lattice points, so that footprints are left out of range, left behind, and come back under later measurements.
Env 0: everybody hears everybody (agent 2 stays at 15 m: a global last op that sets no flag).  Env 1: nobody hears anybody for the first six
steps (the footprints an agent leaves behind pile up), then everybody.  Env 2: agents 0 and 1 hear each other, agent 2 nobody."""
import functools

import numpy as np

import ipp_oracle as O
from configs import make_params

SEED = 99
E, N = 3, 3
STARTS = [[[10, 10, 15], [15, 10, 15], [40, 40, 15]]] * E
SCRIPT = [5, 5] + [4, 1] * 7


def comm_ranges(t):
    return [100.0, 0.0 if t < 6 else 100.0, 7.0]


def choose(e, i, t):
    if e == 0 and i == 2:
        return 3 if t % 2 == 0 else 2
    return SCRIPT[t]


def scenario_params(**over):
    return make_params("small", experiment__missions__n_agents=N, experiment__uav__communication_range=100, **over)


def read_points(kind, T):
    """The steps after which somebody looks at the maps: (a) once, after the last step; (b) every four steps."""
    return {T - 1} if kind == "end" else set(range(3, T, 4)) | {T - 1}


@functools.lru_cache(maxsize=None)
def oracle_episodes(episodes):
    """The scripted episodes on the oracle, once per tuple of episode numbers: per env the step records and the final maps."""
    params = scenario_params()
    d = O.Derived(params)
    out = []
    for e, ep_no in enumerate(episodes):
        holder = {}

        def correctness(i, s, shape, ep_no=ep_no, holder=holder):
            pos = holder["ep"].agents[i]["position"]
            _, fc = O.project_field_of_view(d, pos)
            return O.philox_correctness(SEED, ep_no, i, s, fc, d.gy, O.noise_of_altitude(pos[2]))

        ep = O.OracleEpisode(params, ep_no, correctness, lambda i, t, m, o, e=e: choose(e, i, t), build_features=False,
                             start_positions=STARTS[e], exact=True)
        holder["ep"] = ep
        log = []
        for t in range(d.budget + 1):
            ep.comm_range = comm_ranges(t)[e]
            rec = ep.step(t)
            log.append({k: rec[k] for k in ("actions", "positions", "next_positions", "rects", "next_rects", "received", "relative_reward")})
        out.append(dict(log=log, global_map=ep.global_map.copy(), local_maps=np.array([a["local_map"] for a in ep.agents])))
    return out
