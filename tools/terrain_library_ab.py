#!/usr/bin/env python
"""What a reset costs over each terrain, at BASELINE config 2's shape (4 UAVs, 256 x 256, 1024 envs, env-only): ``split`` (the half-plane
of ippm_reset_episode), ``random_field`` (the synthesis passes) and ``library`` (ippm_terrain_library_draw out of 64 maps of 1024 x 1024,
once with library_augment="none" and once with "d4"), all in ONE process.

Per terrain: 10 warm-up resets, then 50 timed ones, each on fresh episode ids; of every timed reset the dispatch-bound kernel times
(VecEnv.profile: events on the launches themselves) summed per class -- ``terrain`` (synthesis passes / the library draw), ``reset``
(ippm_reset_episode) and ``reset_maps`` (prior fill + start sensing) -- and the wall time of ``reset()`` to its completion.  The medians
of the 50 are printed per terrain, for three such runs.  ``random_field`` is the yardstick: the same code as before the library existed.

    python tools/terrain_library_ab.py [--envs 1024] [--maps 64] [--side 1024] [--resets 50] [--warmup 10] [--runs 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ipp-marl_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

CLASSES = ("terrain", "reset", "reset_maps")
CASES = (("split", "split", None), ("random_field", "random_field", None), ("library_none", "library", "none"), ("library_d4", "library", "d4"))


def timed_resets(env, first, count):
    """-> per class the per-reset sums of kernel time (us) and the launches of one reset, and the wall times (us)."""
    sums = {c: [] for c in CLASSES}
    launches = {c: 0 for c in CLASSES}
    wall = []
    for k in range(count):
        ids = np.arange(first + k * env.E, first + (k + 1) * env.E)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.reset(ids)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
        times = env.event_times_us()
        for c in CLASSES:
            rec = times.get(c)
            sums[c].append(rec["avg_us"] * rec["launches"] if rec else 0.0)
            launches[c] = rec["launches"] if rec else 0
    return sums, launches, wall


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--maps", type=int, default=64)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--resets", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("terrain_library_ab.py measures on the GPU; there is nothing to report without one")
    from ippmarl.params import grid256_params
    from ippmarl.vec_env import VecEnv
    params = grid256_params(experiment__missions__n_agents=4)
    maps = np.random.RandomState(1).rand(args.maps, args.side, args.side) < 0.5
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    emit({"device": torch.cuda.get_device_name(), "envs": args.envs, "agents": 4, "grid": [256, 256], "library": [args.maps, args.side, args.side],
          "library_packed_bytes": args.maps * args.side * ((args.side + 31) // 32) * 4, "resets": args.resets, "warmup": args.warmup,
          "truth_bytes_per_reset": args.envs * 256 * 256 // 8})
    envs = {}
    for name, terrain, augment in CASES:
        kw = dict(terrain_library=maps, library_augment=augment) if terrain == "library" else {}
        envs[name] = VecEnv(params, args.envs, philox_seed=3, terrain=terrain, track_area=False, **kw)
        envs[name].profile = True
    for run in range(args.runs):
        for name, env in envs.items():
            first = 1 + run * (args.resets + args.warmup) * env.E
            timed_resets(env, first, args.warmup)
            sums, launches, wall = timed_resets(env, first + args.warmup * env.E, args.resets)
            rec = {"run": run, "terrain": name, "wall_us_median": round(statistics.median(wall), 2)}
            for c in CLASSES:
                rec[c + "_us_median"] = round(statistics.median(sums[c]), 2)
                rec[c + "_us_min"] = round(min(sums[c]), 2)
                rec[c + "_launches"] = launches[c]
            emit(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
