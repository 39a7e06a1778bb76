#!/usr/bin/env python
"""A/B of the critic's no-grad forward: the float32 PyTorch module (CriticNetwork, the default inference path) against libippmarl's
bf16 matrix-core forward (ippm_critic_forward, ``critic_inference="native"``), in one process, HIP events around every run, the median
of ``--runs`` runs after ``--warmup`` at each batch size.  Also times the repack (ippm_critic_pack) and prints how far the two paths'
Q values are apart.  One JSON line per batch size.

    python tools/critic_forward_ab.py [--batches 8 4096 16384] [--actions 6] [--runs 50] [--warmup 10]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("oracle", "ipp-marl_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import torch  # noqa: E402


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 4096, 16384])
    ap.add_argument("--actions", type=int, default=6)
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from configs import make_params
    from ippmarl.critic_native import NativeCritic
    from ippmarl.networks import CriticNetwork
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    critic = CriticNetwork(make_params("c2", experiment__constraints__num_actions=args.actions)).to(dev).eval()
    native = NativeCritic(critic, dev)
    pack_us, _ = timed(native.refresh, args.runs, args.warmup)
    flop = 2 * (49 * 256 * 300 + 16 * 256 * 4096 + 256 * 4096 + 256 * 256 + 256 * args.actions)
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        states = (torch.rand(B, 11, 11, 12, generator=g) * (torch.rand(B, 1, 1, 12, generator=g) < 0.7)).to(dev)
        actions = torch.randint(0, args.actions, (B,), generator=g, dtype=torch.int32).to(dev)
        native.reserve(B)

        def run_torch():
            with torch.no_grad():
                return critic(states)[0]

        def run_native():
            return native.forward(states)[0]

        def run_native_sel():     # what the TD targets use: the chosen action's Q only
            return native.forward(states, actions, want_q=False)[1]

        t_med, t_min = timed(run_torch, args.runs, args.warmup)
        n_med, n_min = timed(run_native, args.runs, args.warmup)
        s_med, _ = timed(run_native_sel, args.runs, args.warmup)
        diff = float((run_torch().view(B, -1) - run_native()).abs().max())
        print(json.dumps({"batch": B, "actions": args.actions, "torch_f32_us_median": round(t_med, 1), "torch_f32_us_min": round(t_min, 1),
                          "native_bf16_us_median": round(n_med, 1), "native_bf16_us_min": round(n_min, 1),
                          "native_bf16_q_sel_us_median": round(s_med, 1), "speedup_median": round(t_med / n_med, 2),
                          "native_tflops": round(flop * B / n_med / 1e6, 1), "pack_us_median": round(pack_us, 1),
                          "max_abs_q_difference": diff}), flush=True)


if __name__ == "__main__":
    main()
