#!/usr/bin/env python
"""A/B of the COMA round as ``COMAMission.execute`` drives it -- ``keep_rollout_log`` on, ``update(diagnostics=True)``, the
``add_to_tensorboard`` work with a writer that keeps every scalar -- with the rollout log on the torch path and on the native one, in ONE
process, the forms alternating:

    (a) plain         rollout_log="torch",  metrics="torch":  rollout(), update() -- a run that logs nothing
    (b) metrics_only  rollout_log="torch",  metrics="native": update(diagnostics=True), no rollout log kept -- what profiles/r18/ called a
                      logging run
    (c) torch_log     rollout_log="torch",  metrics="native": the mission's round before the switch existed: three clones per rollout step,
                      launch by launch even where the step graphs are recorded, five arrays to the host and ~20 host reductions per round
    (d) native_log    rollout_log="native", metrics="native": the mission's round with the log launch in every (recorded) step, one closing
                      launch and one device-to-host copy

on two shapes of the 256 x 256 grid with 4 UAVs: ``reference`` (5 envs, 300 transitions per update, graphs=True and capture_graphs(): the
shape of profiles/r18/) and ``large`` (1024 envs, 61 440 transitions per update, launch by launch).  Every other switch comes from the
environment (IPPMARL_ADAM, IPPMARL_HEAD_UPDATE, ...), as in bench.py; all trainers see the same.  Per form: updates/s of ``--repeats``
windows of at least ``--window`` seconds each after ``--warmup`` rounds; and, from one profiled rollout (torch.profiler), the device
operations and host-side launch calls per rollout step -- launch by launch before the capture (``as_recorded``: what a step graph holds)
and as timed.  One JSON document per shape to ``--out-dir`` and to stdout.

    python tools/rollout_log_ab.py [--shapes reference,large] [--window 1.5] [--repeats 5] [--warmup 3] [--out-dir profiles/r19]"""
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
#        rollout_log, metrics, the mission's logging
FORMS = {"plain": ("torch", "torch", False), "metrics_only": ("torch", "native", False), "torch_log": ("torch", "native", True),
         "native_log": ("native", "native", True)}
SHAPES = {"reference": (5, True), "large": (1024, False)}        # envs, graphs


class Recorder:
    """A writer that keeps the last value of every tag."""

    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, step):
        self.scalars[tag] = float(value)


def one_round(mission, form):
    """One pass of the body of COMAMission.execute (without the checkpoint and the evaluation), or its non-logging counterparts."""
    tr = mission.trainer
    if form == "plain":
        tr.rollout("train")
        tr.update()
        return
    wave = tr.rollout("train")
    stats = tr.update(diagnostics=True)
    mission.training_step_idx = tr.train_step
    mission.environment_step_idx += stats["transitions"]
    if form == "metrics_only":
        for tag, value in tr.last_diagnostics.items():
            mission.writer.add_scalar(tag, value, mission.training_step_idx)
        return
    mission.add_to_tensorboard([tr.last_rollout], tr.last_diagnostics)
    mission.episode_returns.append(wave["episode_return"])


def window(mission, form, seconds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rounds = 0
    while True:
        one_round(mission, form)
        rounds += 1
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return rounds / (time.perf_counter() - t0), rounds


def profile_rollout(tr):
    """Device operations, host-side launch calls and host synchronisations of ONE rollout("train"), per rollout step where that divides."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        tr.rollout("train")
        torch.cuda.synchronize()
    tr.update()
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
    return {"device_kernels": kernels, "device_copies": copies, "host_launch_calls": launches,
            "device_operations_per_step": round((kernels + copies) / tr.T, 2), "host_launch_calls_per_step": round(launches / tr.T, 2),
            "graph_launches": runtime.get("hipGraphLaunch", 0)}


def run_shape(name, args):
    from ippmarl.missions.coma_mission import COMAMission
    from ippmarl.params import grid256_params
    envs, graphs = SHAPES[name]
    params = grid256_params(experiment__missions__n_agents=4)
    missions, recorded = {}, {}
    for form, (log, metrics, keep) in FORMS.items():
        torch.manual_seed(1)
        m = COMAMission(params, Recorder(), n_envs=envs, eval_every=0, philox_seed=3, graphs=graphs, metrics=metrics, rollout_log=log)
        m.trainer.keep_rollout_log = keep
        one_round(m, form)
        torch.cuda.synchronize()
        recorded[form] = profile_rollout(m.trainer)
        if graphs:
            m.trainer.capture_graphs()
        missions[form] = m
    for form, m in missions.items():
        for _ in range(args.warmup):
            one_round(m, form)
    torch.cuda.synchronize()
    rates = {form: [] for form in FORMS}
    rounds = {form: [] for form in FORMS}
    for _ in range(args.repeats):
        for form, m in missions.items():
            r, n = window(m, form, args.window)
            rates[form].append(r)
            rounds[form].append(n)
    tr = missions["native_log"].trainer
    result = {"shape": {"name": name, "envs": tr.E, "agents": tr.N, "steps": tr.T, "transitions_per_update": tr.T * tr.E * tr.N,
                        "batch_number": tr.batch_number, "data_passes": tr.data_passes, "n_actions": tr.A, "hip_graphs": graphs},
              "switches": {v: os.environ.get(v, "unset") for v in SWITCHES}, "device": torch.cuda.get_device_name(),
              "window_s": args.window, "repeats": args.repeats, "warmup_rounds": args.warmup, "forms": {}}
    for form, (log, metrics, keep) in FORMS.items():
        xs = rates[form]
        t = missions[form].trainer
        before = t.step_replays
        timed = profile_rollout(t)
        result["forms"][form] = {"rollout_log": log, "metrics": metrics, "mission_log": keep, "updates_per_s": [round(x, 3) for x in xs],
                                 "median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
                                 "spread_percent": round(100.0 * (max(xs) - min(xs)) / statistics.median(xs), 2),
                                 "rounds_per_window": rounds[form], "rollout_as_timed": timed, "rollout_as_recorded": recorded[form],
                                 "steps_replayed_in_the_profiled_rollout": t.step_replays - before,
                                 "scalars_written": len(missions[form].writer.scalars)}
    med = {k: v["median"] for k, v in result["forms"].items()}
    result["native_log_over_torch_log"] = round(med["native_log"] / med["torch_log"], 3)
    result["native_log_below_metrics_only_percent"] = round(100.0 * (1.0 - med["native_log"] / med["metrics_only"]), 2)
    result["native_log_below_plain_percent"] = round(100.0 * (1.0 - med["native_log"] / med["plain"]), 2)
    result["torch_log_below_plain_percent"] = round(100.0 * (1.0 - med["torch_log"] / med["plain"]), 2)
    text = json.dumps(result, indent=1)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, f"rollout_log_ab_{name}{args.suffix}.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    del missions
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="reference,large")
    ap.add_argument("--window", type=float, default=1.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r19"))
    ap.add_argument("--suffix", default="", help="appended to the file names (e.g. _four_switches)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_log_ab.py measures on the GPU; there is nothing to report without one")
    for name in args.shapes.split(","):
        run_shape(name, args)


if __name__ == "__main__":
    main()
