"""Timing of the map scoring pass (ippm_score_maps) against the four passes it replaces -- one ippm_weighted_entropy and three
ippm_f1_counts, their memsets included -- on the same maps, and of COMATrainer.curves_on against returns_on on the same episodes.
Warm-up first, then the arms alternate in one process; every figure comes with its spread over the repeats.
    python tools/score_bench.py [--repeats 9] [--inner 20] [--episodes 1024] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("oracle", "ipp-marl_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))
from configs import make_params  # noqa: E402
from ippmarl import _ffi  # noqa: E402
from ippmarl.derived import DerivedConstants  # noqa: E402
from ippmarl.trainer import COMATrainer  # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s (MI355X)

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--inner", type=int, default=20, help="calls per timed window")
ap.add_argument("--episodes", type=int, default=1024)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "score_bench.py needs the MI355X"
dev = torch.device("cuda:0")
p = _ffi.ptr


def spread(us):
    return {"median_us": float(np.median(us)), "min_us": float(np.min(us)), "max_us": float(np.max(us)), "repeats": len(us)}


def pass_times(config, n_maps, tiled):
    d = DerivedConstants(make_params(config))
    ctx = _ffi.Context(d)
    ctx.call("ippm_set_map_layout", 1 if tiled else 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    gen = torch.Generator(device=dev).manual_seed(1)
    # maps as an episode leaves them: half the cells observed (log-odds up to the clip), half at the prior; a half-plane-like truth
    maps = torch.where(torch.rand(n_maps, d.grid_x, d.grid_y, device=dev, generator=gen) < 0.5,
                       torch.randn(n_maps, d.grid_x, d.grid_y, device=dev, generator=gen) * 4, torch.zeros((), device=dev)).contiguous()
    truth = torch.zeros(n_maps, d.truth_bytes, dtype=torch.uint8, device=dev)
    truth[:, : d.truth_bytes * 2 // 5] = 255
    words = np.zeros(1, dtype=np.int64)
    ctx.call("ippm_score_scratch", n_maps, words.ctypes.data)
    scratch = torch.empty(int(words[0]), dtype=torch.float64, device=dev)
    ent = torch.empty(n_maps, dtype=torch.float64, device=dev)
    counts = torch.empty(n_maps, 3, 3, dtype=torch.int64, device=dev)
    old_ent = torch.empty(n_maps, dtype=torch.float64, device=dev)
    old_counts = torch.empty(3, n_maps, 3, dtype=torch.int64, device=dev)

    def new():
        ctx.call("ippm_score_maps", p(maps), p(truth), 1, 1e-5, p(ent), p(counts), p(scratch), n_maps, stream)

    def old():
        ctx.call("ippm_weighted_entropy", p(maps), p(truth), 1, p(old_ent), n_maps, stream)
        for k, thr in enumerate((1e-5, 0.0, -1e-5)):
            ctx.call("ippm_f1_counts", p(maps), p(truth), 1, thr, p(old_counts[k]), n_maps, stream)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / args.inner

    for _ in range(3):
        new()
        old()
    torch.cuda.synchronize()
    assert torch.equal(counts, old_counts.permute(1, 0, 2)), "the single pass and the four passes count differently"
    rel = float(((ent - old_ent).abs() / old_ent.abs().clamp_min(1e-30)).max())
    t_new, t_old = [], []
    for _ in range(args.repeats):
        t_new.append(timed(new))
        t_old.append(timed(old))
    cells = n_maps * d.grid_x * d.grid_y
    need = cells * (4 + 1 / 8)
    rec = {"config": config, "grid": [d.grid_x, d.grid_y], "maps": n_maps, "layout": "tiles" if tiled else "rows", "bytes_needed": need,
           "score_maps": spread(t_new), "four_passes": spread(t_old), "entropy_rel_diff_to_weighted_entropy": rel}
    rec["score_maps"]["fraction_of_hbm_peak"] = need / HBM_PEAK / (1e-6 * rec["score_maps"]["median_us"])
    rec["four_passes"]["fraction_of_hbm_peak"] = need / HBM_PEAK / (1e-6 * rec["four_passes"]["median_us"])
    rec["speedup_median"] = rec["four_passes"]["median_us"] / rec["score_maps"]["median_us"]
    rec["faster_beyond_spread"] = rec["score_maps"]["max_us"] < rec["four_passes"]["min_us"]
    print(json.dumps(rec), flush=True)
    return rec


def curve_times(E):
    tr = COMATrainer(make_params("c2"), n_envs=E, philox_seed=3)
    episodes = list(range(100001, 100001 + E))

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for _ in range(2):
        tr.curves_on(episodes, "random")
        tr.returns_on(episodes, "random")
    t_curves, t_returns = [], []
    for _ in range(args.repeats):
        t_curves.append(wall(lambda: tr.curves_on(episodes, "random")))
        t_returns.append(wall(lambda: tr.returns_on(episodes, "random")))
    sp = lambda ms: {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "repeats": len(ms)}  # noqa: E731
    rec = {"config": "c2", "episodes": E, "policy": "random", "steps": tr.T, "curves_on": sp(t_curves), "returns_on": sp(t_returns)}
    print(json.dumps(rec), flush=True)
    return rec


out = {"passes": [pass_times("c2", 1024, False), pass_times("c2", 2048, True), pass_times("c5", 64, False)],
       "curves": curve_times(args.episodes)}
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
