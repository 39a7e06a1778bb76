#!/usr/bin/env python
"""A/B of conv2 in the COMA update: each of the three operations of ``conv2_update="bf16"`` (libippmarl's ippm_conv4x4_bf16_forward /
_grad_weight / _grad_input, as networks._Conv4x4Bf16 calls them, scratch allocation included) against what the default path runs for it:
the convolution library's float32 forward, ``aten.convolution_backward``'s weight gradient, and the hipBLASLt GEMM + ippm_col2im_nhwc
input gradient of networks._ConvDataGradAsGemm.  One process, HIP events around every call, median and minimum of ``--runs`` calls after
``--warmup`` at each batch size.  One JSON line per batch size; the default batch sizes are 8 and config 3's minibatch
(61 440 transitions / batch_number).

    python tools/conv2_update_ab.py [--batches 8 12288] [--runs 50] [--warmup 10]"""
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


def main():
    from ippmarl.params import grid256_params
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 61440 // grid256_params()["networks"]["batch_number"]])
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from ippmarl import networks
    bf16, gemm = networks._Conv4x4Bf16, networks._ConvDataGradAsGemm
    dev = torch.device("cuda:0")
    flop = 2 * 16 * 256 * 4096      # per sample and operation
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        x = (torch.relu(torch.randn(B, 7, 7, 256, generator=g)) * (torch.rand(B, 1, 1, 256, generator=g) < 0.7)).to(dev).permute(0, 3, 1, 2)
        w = (torch.randn(256, 256, 4, 4, generator=g) * (2.0 / 4096) ** 0.5).to(dev)
        gy = (torch.randn(B, 4, 4, 256, generator=g) / B ** 0.5).to(dev).permute(0, 3, 1, 2)
        assert x.is_contiguous(memory_format=torch.channels_last) and gy.is_contiguous(memory_format=torch.channels_last)

        class Ctx:   # what the two Functions' backward passes read of their context
            saved_tensors = (x, w)
            needs_input_grad = (False, False, False)

            def save_for_backward(self, *tensors):
                pass

        def ctx(*needs):
            c = Ctx()
            c.needs_input_grad = needs
            return c

        ops = {
            "forward": (lambda: torch.nn.functional.conv2d(x, w), lambda: bf16.forward(ctx(), x, w)),
            "grad_weight": (lambda: gemm.backward(ctx(False, True, False), gy)[1], lambda: bf16.backward(ctx(False, True), gy)[1]),
            "grad_input": (lambda: gemm.backward(ctx(True, False, False), gy)[0], lambda: bf16.backward(ctx(True, False), gy)[0]),
        }
        row = {"batch": B, "runs": args.runs, "warmup": args.warmup}
        with torch.no_grad():
            for name, (f32, b16) in ops.items():
                f_med, f_min = timed(f32, args.runs, args.warmup)
                b_med, b_min = timed(b16, args.runs, args.warmup)
                ref = f32()
                row[name] = {"float32_us_median": round(f_med, 1), "float32_us_min": round(f_min, 1), "bf16_us_median": round(b_med, 1),
                             "bf16_us_min": round(b_min, 1), "speedup_median": round(f_med / b_med, 2),
                             "float32_tflops": round(flop * B / f_med / 1e6, 1), "bf16_tflops": round(flop * B / b_med / 1e6, 1),
                             "max_abs_difference": float((ref - b16()).abs().max()), "max_abs_float32": float(ref.abs().max())}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
