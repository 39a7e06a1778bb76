#!/usr/bin/env python
"""Randomised sweep of the Philox-mode parity check (tests/test_hip_env_parity.py::check_philox_episodes):
random team sizes, action sets, comm ranges, link-failure rates, seeds and episodes on the 128 x 128 and 256 x 256 grids; every
step of every episode against the oracle.  python tools/stress_parity.py [n_cases] [rng_seed]"""
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("tests", "oracle", "ipp-marl_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))
from test_hip_env_parity import check_philox_episodes as check  # noqa: E402
from test_hip_dropin import test_batched_ig_policy_matches_oracle as check_ig  # noqa: E402
from random_configs import random_case  # noqa: E402

def main():
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    t0 = time.time()
    ties = mixed = 0
    for k in range(n_cases):
        name, over, n_envs, seed, ep0, n, A = random_case(rng, even_batches=True)
        try:
            # every fourth case: the untracked kernels (tile-item fusion), half of those as steps() alone (bench.py's launch sequence)
            # (class-weight threshold ties are recognised by the comparison itself -- tests/conftest.py::assert_features_or_ties admits a
            #  whole-class-weight difference only where the oracle's deciding area average is within 32 ulp of 0.499 / 0.501 -- and counted)
            # every fifth case as a batch of MIXED team sizes (round 5): env e flies 1 .. N of the configured UAVs and is compared with an
            # oracle run of that team size
            teams = [rng.randint(1, n) for _ in range(n_envs)] if k % 5 == 2 else None
            mixed += teams is not None
            ties += check(name, over, n_envs, seed=seed, first_episode=ep0, track_area=k % 4 != 1, fused_step=k % 8 == 5, team_sizes=teams)
            # every third case also through the greedy planner (K9 + K10) -- not above 15 m: the reference's planner divides by the
            # sensor noise, which its sensor model sets to 0 there (ZeroDivisionError in IG_baseline.py, as in the oracle)
            if k % 3 == 0 and over.get("experiment__constraints__max_altitude", 15) <= 15:
                check_ig(name, over, seed=seed & 0xFFFFFFFF, first_episode=ep0, n_envs=n_envs)
        except Exception as exc:
            msg = str(exc)
            # (an agent boxed in by the others: the reference's torch.multinomial raises on the all-zero mask, the oracle with it; the
            #  device sets fault[e] -- tests/test_hip_env_parity.py::test_empty_mask_sets_fault_flag)
            if "footprint image smaller than 11 cells" in msg or "empty action mask" in msg:   # documented restrictions
                print(f"case {k}: skipped ({exc})", flush=True)
                continue
            raise
        print(f"case {k}: {name} px={over.get('sensor__pixel__number_x', '-')} prior={over.get('mapping__prior', 0.5)} N={n} A={A} range={over['experiment__uav__communication_range']} fail={over['experiment__uav__failure_rate']} "
              f"fix={over['experiment__uav__fix_range']} envs={n_envs}{' teams=' + str(teams) if teams else ''} ok ({time.time() - t0:.0f}s)", flush=True)
    print("all", n_cases, "cases match the oracle (", mixed, "of them batches of mixed team sizes );", ties, "feature elements sat on a proven class-weight threshold tie")


if __name__ == "__main__":   # (the oracle pool spawns workers that re-import this module)
    main()
