"""Shared by test_conv2_train_cpu.py and test_hip_conv2_train.py: the numerical contract of the bf16 conv2 of the COMA update
(csrc/conv4x4_train.hip, networks._Conv4x4Bf16) restated in PyTorch on the CPU, and the constructed inputs the tests run.  Nothing here
calls the code under test.

Contract: every operand tensor (x, w, gy) is rounded to bf16 and promoted to the accumulation type; nothing else
is rounded.  ``float64`` is the reference; ``float32`` is a second legitimate accumulation order, and the spread between the two is the
unit the dense tolerances are stated in (``MARGIN`` spreads: the value of tests/actor_native_ref.py).

Tensors are channels-last, as the C entry points take them: x [B,ih,iw,256], y and gy [B,ih-3,iw-3,256]; w and gw [256,256,4,4]."""
import functools

import torch
import torch.nn.functional as F

from actor_native_ref import MARGIN, _dense_layer  # noqa: F401

CH = 256
W_SHAPE = (CH, CH, 4, 4)


def _bf16(t, dtype):
    return t.to(torch.bfloat16).to(dtype)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def forward(x, w, dtype):
    """y = conv2d(bf16(x), bf16(w))"""
    return _nhwc(F.conv2d(_nchw(_bf16(x, dtype)), _bf16(w, dtype)))


def grad_input(gy, w, dtype):
    """gx = conv_transpose2d(bf16(gy), bf16(w))"""
    return _nhwc(F.conv_transpose2d(_nchw(_bf16(gy, dtype)), _bf16(w, dtype)))


def grad_weight(gy, x, dtype):
    """gw = the weight gradient of conv2d at (bf16(x), bf16(gy))"""
    return torch.nn.grad.conv2d_weight(_nchw(_bf16(x, dtype)).contiguous(), W_SHAPE, _nchw(_bf16(gy, dtype)).contiguous())


class RestatedConv2(torch.autograd.Function):
    """The three formulas as one differentiable step of a CPU network (logical NCHW in and out), in the dtype of its input."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return F.conv2d(_bf16(x, x.dtype), _bf16(w, x.dtype))

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        g = _bf16(gy, x.dtype)
        return (F.conv_transpose2d(g, _bf16(w, x.dtype)),
                torch.nn.grad.conv2d_weight(_bf16(x, x.dtype).contiguous(), W_SHAPE, g.contiguous()))


def net_grads(net, inputs, loss_fn, dtype):
    """The gradients of ``loss_fn(fc3's output)`` with respect to the ten used parameters of a convnet of networks._ConvTrunk's shape, on the
    CPU in ``dtype``, with conv2 restated.  net: {layer: (weight, bias)} float32; inputs float32 [B,11,11,planes]
    -> {"conv1.weight": grad, ...}."""
    p = {f"{n}.{k}": t.to(dtype).clone().requires_grad_(True) for n, (w, b) in net.items() for k, t in (("weight", w), ("bias", b))}
    h = torch.relu(F.conv2d(_nchw(inputs.to(dtype)), p["conv1.weight"], p["conv1.bias"]))
    h = torch.relu(RestatedConv2.apply(h, p["conv2.weight"]) + p["conv2.bias"].view(1, -1, 1, 1))
    h = torch.relu(F.conv2d(h, p["conv3.weight"], p["conv3.bias"])).flatten(1)
    h = torch.relu(F.linear(h, p["fc1.weight"], p["fc1.bias"]))
    loss_fn(F.linear(h, p["fc3.weight"], p["fc3.bias"])).backward()
    return {k: t.grad for k, t in p.items()}


# ---- the small-integer case: every partial sum is an integer below 2^24, so any accumulation order is exact ---------------------------
@functools.lru_cache(maxsize=None)
def int_w(seed=1):
    return torch.randint(-3, 4, W_SHAPE, generator=torch.Generator().manual_seed(seed)).float()


@functools.lru_cache(maxsize=None)
def int_x(batch, ih, iw, seed=2):
    return torch.randint(0, 4, (batch, ih, iw, CH), generator=torch.Generator().manual_seed(seed + 31 * batch + ih * 11 + iw)).float()


@functools.lru_cache(maxsize=None)
def int_gy(batch, ih, iw, seed=3):
    return torch.randint(-2, 3, (batch, ih - 3, iw - 3, CH), generator=torch.Generator().manual_seed(seed + 31 * batch + ih * 11 + iw)).float()


@functools.lru_cache(maxsize=None)
def int_case(batch, ih, iw, ops=("y", "gx", "gw")):
    """{"y" | "gx" | "gw": the float64 restatement} of the integer inputs of this shape."""
    x, w, gy = int_x(batch, ih, iw), int_w(), int_gy(batch, ih, iw)
    out = {}
    if "y" in ops:
        out["y"] = forward(x, w, torch.float64)
    if "gx" in ops:
        out["gx"] = grad_input(gy, w, torch.float64)
    if "gw" in ops:
        out["gw"] = grad_weight(gy, x, torch.float64)
    return out


# ---- the dense real case ------------------------------------------------------------------------------------------------------------------
DENSE_SEEDS, DENSE_BATCH = (1, 2, 3), 300


@functools.lru_cache(maxsize=None)
def dense_inputs(seed, batch=DENSE_BATCH, ih=7, iw=7):
    """w He-normal, x = relu(randn) with 30 % of the channels zeroed per sample, gy = randn / sqrt(batch)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(W_SHAPE, generator=g) * (2.0 / (CH * 16)) ** 0.5
    x = torch.relu(torch.randn(batch, ih, iw, CH, generator=g)) * (torch.rand(batch, 1, 1, CH, generator=g) < 0.7)
    gy = torch.randn(batch, ih - 3, iw - 3, CH, generator=g) / batch ** 0.5
    return x, w, gy


@functools.lru_cache(maxsize=None)
def dense_case(seed, dtype):
    x, w, gy = dense_inputs(seed)
    return {"y": forward(x, w, dtype), "gx": grad_input(gy, w, dtype), "gw": grad_weight(gy, x, dtype)}


def dense_spreads(seed):
    """{op: (max |restatement(float32) - restatement(float64)|, restatement(float64))}"""
    r32, r64 = dense_case(seed, torch.float32), dense_case(seed, torch.float64)
    return {k: (float((r32[k].double() - r64[k]).abs().max()), r64[k]) for k in r64}
