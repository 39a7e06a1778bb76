"""Records DeepQ episodes of the reference into tests/golden/ (mission type "DeepQ": every agent's transition carries the reward of
fusing only its own fresh measurement into the step's global map, coma_wrapper.py:113-133).

Runs only where the reference is installed: it imports oracle/make_golden.py and calls its ``run_reference_episode`` unchanged.

    python tools/make_golden_deepq.py            # the three fixtures of tests/test_deepq_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import make_golden as G  # noqa: E402
from configs import make_params  # noqa: E402

# tag -> (params name, overrides, episode); the same cases as the COMA fixtures of oracle/make_golden.py, flown as DeepQ
CASES = {
    "episode_deepq_small_e5": ("small", dict(), 5),
    "episode_deepq_small27_e6": ("small", dict(experiment__missions__n_agents=3, experiment__uav__fix_range=False,
                                               experiment__uav__failure_rate=0.3, experiment__constraints__num_actions=27), 6),
    "episode_deepq_prior03_e4": ("small", dict(mapping__prior=0.3, experiment__missions__n_agents=3), 4),
}


def main():
    for tag, (name, over, episode) in CASES.items():
        G.run_reference_episode(make_params(name, experiment__missions__type="DeepQ", **over), episode, tag)


if __name__ == "__main__":
    main()
