#!/usr/bin/env python
"""A/B of conv1 and conv3 in the COMA update: each new operation of ``trunk_update="bf16"`` (libippmarl's ippm_conv5x5_bf16_forward with
the fused bias + ReLU store and ippm_conv5x5_bf16_grad_weight, as networks._Conv5x5Bf16 calls them; the 4x4 entry points at ih = iw = 4 as
networks._Conv3Bf16 calls them; scratch allocation included) against what the default path runs for it: the convolution library's float32
forward followed by networks._BiasReLU, ``aten.convolution_backward``'s weight gradient, and for conv3 ``F.linear`` on the permuted weight
and its two backward GEMMs.  One process, HIP events around every call, median and minimum of ``--runs`` calls after ``--warmup`` at each
batch size.  One JSON line per batch size; the default batch sizes are 8 and config 3's minibatch (61 440 transitions / batch_number).

    python tools/trunk_update_ab.py [--batches 8 12288] [--runs 50] [--warmup 10]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ipp-marl_amd"))

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


class Ctx:   # what the Functions' forward and backward passes use of their context
    saved_tensors = ()
    needs_input_grad = (False, False, False)

    def save_for_backward(self, *tensors):
        pass

    def mark_dirty(self, *tensors):
        pass


def main():
    from ippmarl.params import grid256_params
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 61440 // grid256_params()["networks"]["batch_number"]])
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from ippmarl import networks
    c5, c4, c3, br = networks._Conv5x5Bf16, networks._Conv4x4Bf16, networks._Conv3Bf16, networks._BiasReLU
    conv2d, linear = torch.nn.functional.conv2d, torch.nn.functional.linear
    dev = torch.device("cuda:0")
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        ops, flops = {}, {}
        gy1 = (torch.randn(B, 7, 7, 256, generator=g) / B ** 0.5).to(dev).permute(0, 3, 1, 2)
        for planes in (7, 12):
            x = (torch.rand(B, 11, 11, planes, generator=g) * (torch.rand(B, 1, 1, planes, generator=g) < 0.7)).to(dev).permute(0, 3, 1, 2)
            w = (torch.randn(256, planes, 5, 5, generator=g) * (2.0 / (25 * planes)) ** 0.5).to(dev)
            bias = (torch.randn(256, generator=g) * 0.1).to(dev)
            assert x.is_contiguous(memory_format=torch.channels_last) and c5.usable(x, w.requires_grad_(True), bias)
            w = w.detach()
            ops[f"conv1_p{planes}_forward_bias_relu"] = (lambda x=x, w=w, bias=bias: br.forward(Ctx(), conv2d(x, w), bias),
                                                         lambda x=x, w=w, bias=bias: c5.forward(Ctx(), x, w, bias))
            ops[f"conv1_p{planes}_grad_weight"] = (
                lambda x=x, w=w: torch.ops.aten.convolution_backward(gy1, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                                     [False, True, False])[1],
                lambda x=x: c5.grad_weight(gy1, x))
            flops[f"conv1_p{planes}_forward_bias_relu"] = flops[f"conv1_p{planes}_grad_weight"] = 2 * 49 * 256 * 25 * planes
        # conv3: one output position over the 4x4x256 activation
        h = (torch.relu(torch.randn(B, 4, 4, 256, generator=g)) * (torch.rand(B, 1, 1, 256, generator=g) < 0.7)).to(dev).permute(0, 3, 1, 2)
        w3 = (torch.randn(256, 256, 4, 4, generator=g) * (2.0 / 4096) ** 0.5).to(dev)
        g3 = (torch.randn(B, 256, generator=g) / B ** 0.5).to(dev)
        hf = h.permute(0, 2, 3, 1).reshape(B, -1)                       # (a view of the channels-last activation)
        flat = lambda: w3.permute(0, 2, 3, 1).reshape(256, -1)          # noqa: E731  (the copy the default path makes per forward)
        w3f = flat()
        ops["conv3_forward"] = (lambda: linear(hf, flat()), lambda: c4._call("ippm_conv4x4_bf16_forward", h, w3, torch.empty(B, 256, device=dev), B, 4, 4, False))
        ops["conv3_grad_weight"] = (lambda: (g3.t() @ hf).view(256, 4, 4, 256).permute(0, 3, 1, 2).contiguous(),
                                    lambda: c4._call("ippm_conv4x4_bf16_grad_weight", g3, h, torch.empty_like(w3), B, 4, 4, True))
        ops["conv3_grad_input"] = (lambda: g3 @ w3f,          # [B, (ty, tx, c)]: the native result is permuted to that order, a view
                                   lambda: c4._call("ippm_conv4x4_bf16_grad_input", g3, w3, torch.empty_like(h), B, 4, 4, False).permute(0, 2, 3, 1))
        for name in ("conv3_forward", "conv3_grad_weight", "conv3_grad_input"):
            flops[name] = 2 * 256 * 4096
        assert c3.usable(h, w3.requires_grad_(True))
        w3 = w3.detach()
        row = {"batch": B, "runs": args.runs, "warmup": args.warmup}
        with torch.no_grad():
            for name, (f32, b16) in ops.items():
                f_med, f_min = timed(f32, args.runs, args.warmup)
                b_med, b_min = timed(b16, args.runs, args.warmup)
                ref, got = f32(), b16()
                row[name] = {"float32_us_median": round(f_med, 1), "float32_us_min": round(f_min, 1), "bf16_us_median": round(b_med, 1),
                             "bf16_us_min": round(b_min, 1), "speedup_median": round(f_med / b_med, 2),
                             "float32_tflops": round(flops[name] * B / f_med / 1e6, 1), "bf16_tflops": round(flops[name] * B / b_med / 1e6, 1),
                             "max_abs_difference": float((ref.reshape(-1) - got.reshape(-1)).abs().max()),
                             "max_abs_float32": float(ref.abs().max())}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
