#!/usr/bin/env python
"""A/B of the COMA round -- ``rollout("train")`` + ``update()`` -- with the minibatch order from ``torch.randperm`` (shuffle="torch") and
from libippmarl's keyed permutation (shuffle="native"), in ONE process, the two forms alternating, on two shapes of the 256 x 256 grid with
4 UAVs: ``reference`` (5 envs, 300 transitions per update, graphs=True and capture_graphs(): the recorded round, whose permutation buffer
the torch form refills from the host before every replay) and ``large`` (1024 envs, 61 440 transitions per update, launch by launch).

Every other switch comes from the environment (IPPMARL_ADAM, IPPMARL_BUFFER, ...), as in bench.py; both trainers see the same.  Per form:
updates/s of ``--repeats`` windows of at least ``--window`` seconds each after ``--warmup`` rounds, with their run-to-run spread; and, from
one profiled round (torch.profiler), the host-side launch calls, device kernels and device copies of the round as timed.  No speed is
claimed for the switch: what it removes is a few small launches per round.  One JSON document per shape to ``--out-dir`` and to stdout.

    python tools/shuffle_ab.py [--shapes reference,large] [--window 1.5] [--repeats 5] [--warmup 3] [--out-dir profiles/r23]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ipp-marl_amd"))

import torch  # noqa: E402

SWITCHES = ("IPPMARL_ADAM", "IPPMARL_HEAD_UPDATE", "IPPMARL_TRUNK_UPDATE", "IPPMARL_CONV2_UPDATE", "IPPMARL_ACTOR_INFERENCE",
            "IPPMARL_CRITIC_INFERENCE", "IPPMARL_BUFFER", "IPPMARL_METRICS", "IPPMARL_ROLLOUT_LOG")
LAUNCH_CALLS = ("hipLaunchKernel", "hipExtLaunchKernel", "hipModuleLaunchKernel", "hipExtModuleLaunchKernel", "hipGraphLaunch",
                "hipLaunchCooperativeKernel")
FORMS = ("torch", "native")
SHAPES = {"reference": (5, True), "large": (1024, False)}        # envs, graphs


def one_round(tr):
    tr.rollout("train")
    tr.update()


def window(tr, seconds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rounds = 0
    while True:
        one_round(tr)
        rounds += 1
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return rounds / (time.perf_counter() - t0), rounds


def profile_round(tr):
    """Host-side launch calls, device kernels and device copies of ONE round (rollout + update)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        one_round(tr)
        torch.cuda.synchronize()
    kernels = copies = 0
    runtime = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                copies += 1
            else:
                kernels += 1
        elif e.name.startswith("hip"):
            runtime[e.name] = runtime.get(e.name, 0) + 1
    return {"host_launch_calls": sum(n for name, n in runtime.items() if name in LAUNCH_CALLS), "device_kernels": kernels,
            "device_copies": copies, "graph_launches": runtime.get("hipGraphLaunch", 0)}


def run_shape(name, args):
    from ippmarl.params import grid256_params
    from ippmarl.trainer import COMATrainer
    envs, graphs = SHAPES[name]
    params = grid256_params(experiment__missions__n_agents=4)
    trainers = {}
    for form in FORMS:
        torch.manual_seed(1)
        tr = COMATrainer(params, envs, philox_seed=3, graphs=graphs, shuffle=form)
        one_round(tr)
        torch.cuda.synchronize()
        if graphs:
            tr.capture_graphs()
        trainers[form] = tr
    for tr in trainers.values():
        for _ in range(args.warmup):
            one_round(tr)
    torch.cuda.synchronize()
    rates = {form: [] for form in FORMS}
    rounds = {form: [] for form in FORMS}
    for _ in range(args.repeats):
        for form, tr in trainers.items():
            r, n = window(tr, args.window)
            rates[form].append(r)
            rounds[form].append(n)
    tr = trainers["native"]
    result = {"shape": {"name": name, "envs": tr.E, "agents": tr.N, "steps": tr.T, "transitions_per_update": tr.T * tr.E * tr.N,
                        "batch_number": tr.batch_number, "data_passes": tr.data_passes, "hip_graphs": graphs},
              "switches": {v: os.environ.get(v, "unset") for v in SWITCHES}, "device": torch.cuda.get_device_name(),
              "window_s": args.window, "repeats": args.repeats, "warmup_rounds": args.warmup, "forms": {}}
    for form in FORMS:
        xs = rates[form]
        result["forms"][form] = {"shuffle": form, "updates_per_s": [round(x, 3) for x in xs], "median": round(statistics.median(xs), 3),
                                 "min": round(min(xs), 3), "max": round(max(xs), 3),
                                 "spread_percent": round(100.0 * (max(xs) - min(xs)) / statistics.median(xs), 2),
                                 "rounds_per_window": rounds[form], "round_as_timed": profile_round(trainers[form])}
    med = {k: v["median"] for k, v in result["forms"].items()}
    result["native_over_torch"] = round(med["native"] / med["torch"], 4)
    calls = {k: v["round_as_timed"]["host_launch_calls"] for k, v in result["forms"].items()}
    result["host_launch_calls_removed_per_round"] = calls["torch"] - calls["native"]
    text = json.dumps(result, indent=1)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, f"shuffle_ab_{name}{args.suffix}.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    del trainers
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="reference,large")
    ap.add_argument("--window", type=float, default=1.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r23"))
    ap.add_argument("--suffix", default="", help="appended to the file names")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shuffle_ab.py measures on the GPU; there is nothing to report without one")
    for name in args.shapes.split(","):
        run_shape(name, args)


if __name__ == "__main__":
    main()
