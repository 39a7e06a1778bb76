#!/usr/bin/env python
"""Three-way A/B of the recorded reference-sized COMA round (5 envs x 4 UAVs on the 256 x 256 grid, 300 transitions, 25 + 25 Adam steps on
60-sample minibatches, hipGraphs: the shape of profiles/r17/), in ONE process, the three forms alternating:

    (a) plain    metrics="torch",  update():                  the recorded round, no diagnostics -- a run that logs nothing
    (b) torch    metrics="torch",  update(diagnostics=True):  what a logging run did before the switch existed: the round leaves the graph and
                 every native path, runs launch by launch and reads ~45 scalars one by one -- the baseline
    (c) native   metrics="native", update(diagnostics=True):  the recorded round with the metric launches in it, one read of out[32]

Every other switch comes from the environment (IPPMARL_ADAM, IPPMARL_HEAD_UPDATE, ...), as in bench.py; all three trainers see the same.
Per form: updates/s of ``--repeats`` windows of at least ``--window`` seconds each (rollout + update per round, a device synchronise at the
end of the window; every update ends in a device-to-host read anyway), after ``--warmup`` rounds; and, from one profiled round
(torch.profiler), the device kernels, the host-side launch calls (kernel launches + graph launches) and the host synchronisations of the
update.  The profiler does not see inside a replayed graph, so the same update is also profiled launch by launch BEFORE the capture
(``as_recorded``): for (a) and (c) those are the operations the graph holds.  One JSON document to ``--out`` and to stdout.

    python tools/metrics_ab.py [--window 2.0] [--repeats 5] [--warmup 3] [--out profiles/r18/metrics_ab.json]"""
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
            "IPPMARL_CRITIC_INFERENCE", "IPPMARL_BUFFER")
LAUNCH_CALLS = ("hipLaunchKernel", "hipExtLaunchKernel", "hipModuleLaunchKernel", "hipExtModuleLaunchKernel", "hipGraphLaunch",
                "hipLaunchCooperativeKernel")


def window(tr, diagnostics, seconds):
    """Rounds of rollout + update for at least ``seconds`` -> (updates/s, rounds)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rounds = 0
    while True:
        tr.rollout("train")
        tr.update(diagnostics=diagnostics)
        rounds += 1
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return rounds / (time.perf_counter() - t0), rounds


def profile_update(tr, diagnostics):
    """Device kernels, host-side launch calls and host synchronisations of ONE update() (the rollout in front of it is not counted)."""
    from torch.profiler import ProfilerActivity, profile
    tr.rollout("train")
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        tr.update(diagnostics=diagnostics)
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
    launches = sum(n for name, n in runtime.items() if name in LAUNCH_CALLS)
    # what makes the host wait for the device: blocking copies (a .item() / .tolist() / float() read is one hipMemcpyWithStream) and
    # explicit synchronise calls, minus the device synchronise that closes the profile
    syncs = runtime.get("hipMemcpyWithStream", 0) + sum(n for name, n in runtime.items() if "Synchronize" in name) - 1
    return {"device_kernels": kernels, "device_copies": copies, "host_launch_calls": launches, "host_synchronisations": syncs,
            "runtime_calls": runtime}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "metrics_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_ab.py measures on the GPU; there is nothing to report without one")
    from ippmarl.params import grid256_params
    from ippmarl.trainer import COMATrainer
    params = grid256_params(experiment__missions__n_agents=4)
    forms = {"plain": ("torch", False), "torch": ("torch", True), "native": ("native", True)}
    trainers, recorded = {}, {}
    probe = COMATrainer(params, 1, philox_seed=3)
    # the reference's own round size, as bench.py's reference_sized_round: batch_size * batch_number transitions per update
    envs = max(1, -(-params["networks"]["batch_size"] * params["networks"]["batch_number"] // (probe.T * probe.N)))
    del probe
    for name, (mode, _) in forms.items():
        torch.manual_seed(1)
        tr = COMATrainer(params, envs, philox_seed=3, graphs=True, metrics=mode)
        tr.rollout("train")
        tr.update(diagnostics=forms[name][1])
        torch.cuda.synchronize()
        recorded[name] = profile_update(tr, forms[name][1])
        recorded[name].pop("runtime_calls")
        tr.capture_graphs()
        trainers[name] = tr
    for name, (_, diag) in forms.items():
        for _ in range(args.warmup):
            trainers[name].rollout("train")
            trainers[name].update(diagnostics=diag)
    torch.cuda.synchronize()
    rates = {name: [] for name in forms}
    rounds = {name: [] for name in forms}
    for _ in range(args.repeats):
        for name, (_, diag) in forms.items():
            r, n = window(trainers[name], diag, args.window)
            rates[name].append(r)
            rounds[name].append(n)
    tr = trainers["native"]
    result = {"shape": {"envs": tr.E, "agents": tr.N, "steps": tr.T, "transitions_per_update": tr.T * tr.E * tr.N,
                        "minibatch": tr.T * tr.E * tr.N // tr.batch_number, "batch_number": tr.batch_number, "data_passes": tr.data_passes,
                        "n_actions": tr.A},
              "switches": {v: os.environ.get(v, "unset") for v in SWITCHES}, "device": torch.cuda.get_device_name(),
              "window_s": args.window, "repeats": args.repeats, "warmup_rounds": args.warmup, "forms": {}}
    for name, (mode, diag) in forms.items():
        xs = rates[name]
        result["forms"][name] = {"metrics": mode, "diagnostics": diag, "updates_per_s": [round(x, 3) for x in xs],
                                 "median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
                                 "rounds_per_window": rounds[name], "one_update": profile_update(trainers[name], diag), "as_recorded": recorded[name]}
    med = {k: v["median"] for k, v in result["forms"].items()}
    result["native_over_torch"] = round(med["native"] / med["torch"], 3)
    result["native_cost_over_plain_percent"] = round(100.0 * (1.0 - med["native"] / med["plain"]), 2)
    result["plain_spread_percent"] = round(100.0 * (result["forms"]["plain"]["max"] - result["forms"]["plain"]["min"]) / med["plain"], 2)
    text = json.dumps(result, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
