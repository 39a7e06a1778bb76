"""The reference's comparison figure as numbers: per-step target-region entropy and target-class F1 of the global map (coma_test.py:
84-97,150-196, IG_baseline.py:84-97, random_baseline.py) for the random walk, the greedy information-gain planner and the (untrained,
unless --actor names a checkpoint) actor on the SAME fixed episodes -- COMATrainer.curves_on.  Mean and standard deviation over the
episodes per step, the returns, and the F1 bracket of the exactly-cancelled cells.
    python tools/policy_curves.py [--config c2] [--episodes 1024] [--first 100001] [--seed 0] [--actor best_model.pth] [--out FILE.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("oracle", "ipp-marl_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))
from configs import make_params  # noqa: E402
from ippmarl.trainer import COMATrainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c2")
ap.add_argument("--episodes", type=int, default=1024)
ap.add_argument("--first", type=int, default=100001)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--actor", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "policy_curves.py needs the MI355X"
params = make_params(args.config)
torch.manual_seed(args.seed)
tr = COMATrainer(params, n_envs=args.episodes, philox_seed=3)
if args.actor:
    from ippmarl.checkpoint import load_reference_actor
    tr.actor = load_reference_actor(args.actor, params).to(tr.device)
episodes = list(range(args.first, args.first + args.episodes))


def f1_of(c):      # (tp, fp, fn) int64 [..., 3] -> F1, 0 where nothing is predicted or true
    tp, fp, fn = (c[..., k].double() for k in range(3))
    den = 2 * tp + fp + fn
    return torch.where(den > 0, 2 * tp / den.clamp_min(1), torch.zeros_like(tp))


result = {"config": args.config, "grid": [tr.env.d.grid_x, tr.env.d.grid_y], "agents": tr.N, "episodes": [episodes[0], episodes[-1]],
          "steps": tr.T, "actor": args.actor or f"untrained (torch seed {args.seed})", "index": "0 = prior map, t + 1 = after the sensing of step t",
          "policies": {}}
for policy in ("random", "ig", "actor"):
    out = tr.curves_on(episodes, policy)
    c = out["f1_counts"]
    # the attainable range of F1 under the class of the exactly-cancelled cells
    worst = f1_of(torch.stack([c[..., 0, 0], c[..., 2, 1], c[..., 0, 2]], -1))
    best = f1_of(torch.stack([c[..., 2, 0], c[..., 0, 1], c[..., 2, 2]], -1))
    result["policies"][policy] = {
        "target_entropy_mean": out["target_entropy"].mean(0).tolist(), "target_entropy_std": out["target_entropy"].std(0).tolist(),
        "f1_mean": out["f1"].mean(0).tolist(), "f1_std": out["f1"].std(0).tolist(),
        "f1_worst_mean": worst.mean(0).tolist(), "f1_best_mean": best.mean(0).tolist(),
        "episode_return_mean": float(out["episode_return"].mean()), "episode_return_std": float(out["episode_return"].std()),
        "absolute_return_mean": float(out["absolute_return"].mean()), "faults": int(out["faults"].ne(0).sum()),
        "actions_histogram": torch.bincount(out["actions"].reshape(-1).long(), minlength=tr.A).tolist()}
    r = result["policies"][policy]
    print(f"{policy:7s} return {r['episode_return_mean']:.3f}  final target entropy {r['target_entropy_mean'][-1]:.4f}  final F1 {r['f1_mean'][-1]:.4f}",
          flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
