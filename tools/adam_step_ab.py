#!/usr/bin/env python
"""A/B of the optimizer step of the COMA update: for each net (actor: 7 planes, critic: 12), the sequence "clear the gradients, step, refresh
the bf16 inference pack" in four forms --

    torch    torch.optim.Adam in its default form: zero_grad(set_to_none=False), step(), NativeNet.refresh()
    fused    torch.optim.Adam(capturable=True, fused=True), what graphs=True selects: the same three calls
    native   optim_native.NativeAdam without a pack: zero_grad() (launches nothing behind its own step), step(), NativeNet.refresh()
    packed   optim_native.NativeAdam with the pack attached: zero_grad(), step() -- the one launch also rewrites the pack

One process, HIP events around each call of the sequence, median and minimum of ``--runs`` calls after ``--warmup``; the device launches of
one call are counted with torch.profiler.  The gradients are rewritten outside the timed region before every call (the torch forms
then clear them in the sequence and step on zeros: the cost of a step does not depend on the values).  One JSON line per net.

    python tools/adam_step_ab.py [--runs 50] [--warmup 10]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ipp-marl_amd"))

import torch  # noqa: E402


def timed(fn, prepare, runs, warmup):
    for _ in range(warmup):
        prepare()
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out), min(out)


def launches(fn, prepare):
    """Device kernels of one call (None where the profiler cannot trace the device)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        prepare()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:
        return None


def main():
    from ippmarl.params import grid256_params
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from ippmarl import optim_native
    from ippmarl.actor_native import NativeActor
    from ippmarl.critic_native import NativeCritic
    from ippmarl.networks import ActorNetwork, CriticNetwork
    dev = torch.device("cuda:0")
    params = grid256_params()
    for name, net_cls, native_cls in (("actor", ActorNetwork, NativeActor), ("critic", CriticNetwork, NativeCritic)):
        row = {"net": name, "runs": args.runs, "warmup": args.warmup}
        for form in ("torch", "fused", "native", "packed"):
            torch.manual_seed(1)
            net = net_cls(params).to(dev)
            used = optim_native.used_parameters(net)
            row["parameters"] = sum(p.numel() for p in used)
            pack = native_cls(net, dev)
            lr = params["networks"][name]["learning_rate"]
            if form == "torch":
                opt = torch.optim.Adam(net.parameters(), lr=lr)
            elif form == "fused":
                opt = torch.optim.Adam(net.parameters(), lr=lr, capturable=True, fused=True)
            else:
                opt = optim_native.NativeAdam(net.parameters(), lr, managed=used)
                if form == "packed":
                    opt.attach_pack(pack)
            g = torch.Generator(device=dev).manual_seed(2)
            source = [torch.randn(p.shape, device=dev, generator=g) * 1e-3 for p in used]
            for p in used:
                p.grad = torch.zeros_like(p)

            def prepare(used=used, source=source):
                for p, s in zip(used, source):
                    p.grad.copy_(s)

            def sequence(opt=opt, pack=pack, form=form):
                # (in a round backward() sits between the first two calls; the cost of the three does not depend on the gradients' values)
                opt.zero_grad(set_to_none=False)
                opt.step()
                if form != "packed":
                    pack.refresh()

            med, low = timed(sequence, prepare, args.runs, args.warmup)
            row[form] = {"us_median": round(med, 1), "us_min": round(low, 1), "launches": launches(sequence, prepare)}
            fresh = native_cls(net, dev)
            row[form]["pack_current"] = bool(torch.equal(fresh.packed, pack.packed))
        for form in ("fused", "native", "packed"):
            row[form]["speedup_vs_torch"] = round(row["torch"]["us_median"] / max(row[form]["us_median"], 1e-9), 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
