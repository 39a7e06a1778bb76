"""Shared by test_trunk_update_cpu.py and test_hip_trunk_update.py: the numerical contract of the bf16 conv1 of the COMA update
(csrc/conv5x5_train.hip, networks._Conv5x5Bf16) and of the whole trunk under ``trunk_update("bf16")`` restated in PyTorch on the CPU, and
the constructed inputs the tests run.  Nothing here calls the code under test.

Contract: every operand tensor (x, w, gy) is rounded to bf16 and promoted to the accumulation type; nothing else
is rounded.  ``float64`` is the reference; ``float32`` is a second legitimate accumulation order, and the spread between the two is the
unit the dense tolerances are stated in (``MARGIN`` spreads: the value of tests/actor_native_ref.py).

Tensors are channels-last, as the C entry points take them: x [B,11,11,planes], y and gy [B,7,7,256]; w and gw [256,planes,5,5]."""
import functools
import os
import re

import torch
import torch.nn.functional as F

from actor_native_ref import MARGIN  # noqa: F401

OUT = 256
PLANES = (7, 12)


def header_chunk():
    """IPPM_CONV5X5_WGRAD_CHUNK as include/ippmarl.h defines it (read as text: nothing is loaded)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ippmarl.h")
    with open(path) as f:
        return int(re.search(r"^#define IPPM_CONV5X5_WGRAD_CHUNK (\d+)$", f.read(), re.M).group(1))


CHUNK = header_chunk()
INT_MAX_BATCH = 2 * CHUNK + 3            # the largest batch of the small-integer cases
# |w| <= 3, 0 <= x <= 3, |gy| <= 2: a weight-gradient sum over B * 49 rows stays below 6 * 49 * B, a forward sum below 9 * 300
assert CHUNK <= 4096 and 6 * INT_MAX_BATCH * 49 < 2 ** 24


def w_shape(planes):
    return (OUT, planes, 5, 5)


def _bf16(t, dtype):
    return t.to(torch.bfloat16).to(dtype)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def forward(x, w, bias, dtype):
    """y = conv2d(bf16(x), bf16(w)); with a bias, relu(y + bias)"""
    y = F.conv2d(_nchw(_bf16(x, dtype)), _bf16(w, dtype))
    if bias is not None:
        y = torch.relu(y + bias.to(dtype).view(1, -1, 1, 1))
    return _nhwc(y)


def grad_weight(gy, x, dtype):
    """gw = the weight gradient of conv2d at (bf16(x), bf16(gy))"""
    return torch.nn.grad.conv2d_weight(_nchw(_bf16(x, dtype)).contiguous(), w_shape(x.shape[-1]), _nchw(_bf16(gy, dtype)).contiguous())


class RestatedConv(torch.autograd.Function):
    """A bias-free convolution of the contract as one differentiable step of a CPU network (logical NCHW in and out), in the dtype of
    its input: operands rounded to bf16 in the forward, the output gradient rounded to bf16 in both gradients.  ``bf16_gw`` False: the
    weight gradient is the plain one of the unrounded operands (a layer whose weight gradient stays a float32 GEMM)."""

    @staticmethod
    def forward(ctx, x, w, bf16_gw=True):
        ctx.save_for_backward(x, w)
        ctx.bf16_gw = bf16_gw
        return F.conv2d(_bf16(x, x.dtype), _bf16(w, x.dtype))

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        g = _bf16(gy, x.dtype)
        gx = F.conv_transpose2d(g, _bf16(w, x.dtype)) if ctx.needs_input_grad[0] else None
        gw = (torch.nn.grad.conv2d_weight(_bf16(x, x.dtype).contiguous(), w.shape, g.contiguous()) if ctx.bf16_gw
              else torch.nn.grad.conv2d_weight(x.contiguous(), w.shape, gy.contiguous()))
        return gx, gw, None


# The trunk's contract under trunk_update("bf16") ("conv1 and conv3 in the update"): every convolution's forward and
# input gradient and the weight gradients of conv1 and conv2 take bf16 operands; conv3's weight gradient stays the float32 GEMM on the
# unrounded activation and output gradient.
BF16_WEIGHT_GRADIENT = {"conv1": True, "conv2": True, "conv3": False}


def net_grads(net, inputs, loss_fn, dtype):
    """The gradients of ``loss_fn(fc3's output)`` with respect to the ten used parameters of a convnet of networks._ConvTrunk's shape, on the
    CPU in ``dtype``, with conv1, conv2 and conv3 restated (BF16_WEIGHT_GRADIENT).  net: {layer: (weight, bias)} float32; inputs float32 [B,11,11,planes]
    -> {"conv1.weight": grad, ...}."""
    p = {f"{n}.{k}": t.to(dtype).clone().requires_grad_(True) for n, (w, b) in net.items() for k, t in (("weight", w), ("bias", b))}
    h = _nchw(inputs.to(dtype))
    for name in ("conv1", "conv2", "conv3"):
        h = torch.relu(RestatedConv.apply(h, p[f"{name}.weight"], BF16_WEIGHT_GRADIENT[name]) + p[f"{name}.bias"].view(1, -1, 1, 1))
    h = torch.relu(F.linear(h.flatten(1), p["fc1.weight"], p["fc1.bias"]))
    loss_fn(F.linear(h, p["fc3.weight"], p["fc3.bias"])).backward()
    return {k: t.grad for k, t in p.items()}


# ---- the small-integer case: every partial sum is an integer below 2^24, so any accumulation order is exact ---------------------------
@functools.lru_cache(maxsize=None)
def int_w(planes, seed=1):
    return torch.randint(-3, 4, w_shape(planes), generator=torch.Generator().manual_seed(seed + planes)).float()


@functools.lru_cache(maxsize=None)
def int_bias(seed=4):
    return torch.randint(-40, 41, (OUT,), generator=torch.Generator().manual_seed(seed)).float()


@functools.lru_cache(maxsize=None)
def int_x(batch, planes, seed=2):
    return torch.randint(0, 4, (batch, 11, 11, planes), generator=torch.Generator().manual_seed(seed + 31 * batch + planes)).float()


@functools.lru_cache(maxsize=None)
def int_gy(batch, seed=3):
    return torch.randint(-2, 3, (batch, 7, 7, OUT), generator=torch.Generator().manual_seed(seed + 31 * batch)).float()


@functools.lru_cache(maxsize=None)
def int_forward(batch, planes, with_bias):
    return forward(int_x(batch, planes), int_w(planes), int_bias() if with_bias else None, torch.float64)


@functools.lru_cache(maxsize=None)
def int_grad_weight(batch, planes):
    assert batch <= INT_MAX_BATCH
    return grad_weight(int_gy(batch), int_x(batch, planes), torch.float64)


# ---- the dense real case ------------------------------------------------------------------------------------------------------------------
DENSE_SEEDS, DENSE_BATCH = (1, 2, 3), 300


@functools.lru_cache(maxsize=None)
def dense_inputs(seed, planes, batch=DENSE_BATCH):
    """w He-normal, bias N(0, 0.1), x = rand with 30 % of the planes zeroed per sample (the networks' inputs are in [0, 1]),
    gy = randn / sqrt(batch) -> (x, w, bias, gy)."""
    g = torch.Generator().manual_seed(100 * seed + planes)
    w = torch.randn(w_shape(planes), generator=g) * (2.0 / (planes * 25)) ** 0.5
    bias = torch.randn(OUT, generator=g) * 0.1
    x = torch.rand(batch, 11, 11, planes, generator=g) * (torch.rand(batch, 1, 1, planes, generator=g) < 0.7)
    gy = torch.randn(batch, 7, 7, OUT, generator=g) / batch ** 0.5
    return x, w, bias, gy


@functools.lru_cache(maxsize=None)
def dense_case(seed, planes, dtype):
    x, w, bias, gy = dense_inputs(seed, planes)
    return {"y": forward(x, w, None, dtype), "yb": forward(x, w, bias, dtype), "gw": grad_weight(gy, x, dtype)}


def dense_spreads(seed, planes):
    """{op: (max |restatement(float32) - restatement(float64)|, restatement(float64))}"""
    r32, r64 = dense_case(seed, planes, torch.float32), dense_case(seed, planes, torch.float64)
    return {k: (float((r32[k].double() - r64[k]).abs().max()), r64[k]) for k in r64}
