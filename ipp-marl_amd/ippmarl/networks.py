"""Actor / critic convnets (PyTorch-ROCm; the only place MFMA is used on this path).

Same architecture, layer names and initialisation order as the reference (actor/network.py:10-96,
critic/network.py:12-47) so that a reference ``state_dict`` / ``best_model.pth`` loads unchanged: conv 5x5 -> 4x4 -> 4x4
(11 -> 7 -> 4 -> 1), fc1, (fc2: present but unused, exactly like the reference), fc3.  Inputs are channels-last
[B,11,11,C] as produced by the feature kernels.  The reference's global ``torch.autograd.set_detect_anomaly(True)``
(critic/network.py:9) is deliberately not reproduced.
"""
from __future__ import annotations

import contextlib
import contextvars
import ctypes
import os
from typing import Dict, Optional

import torch
from torch import nn

from . import switches

# MIOpen's exhaustive solver search (needed: its fast mode picks kernels that make a COMA update 6x slower) also times the
# naive reference convolutions, which take 0.3-0.5 s per run on the 12k-sample minibatches: 40 s of warm-up per process
# for nothing.  Leave them out of the search unless the user says otherwise.
for _v in ("FWD", "BWD", "WRW"):
    os.environ.setdefault(f"MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_{_v}", "0")


# conv3 as a GEMM (see _ConvTrunk.trunk); IPPMARL_CONV3_GEMM=0 keeps the convolution call
CONV3_AS_GEMM = os.environ.get("IPPMARL_CONV3_GEMM", "1") != "0"
# bias + ReLU after conv1 / conv2 as one pass (see _BiasReLU); IPPMARL_FUSED_BIAS_RELU=0 keeps PyTorch's separate passes
FUSED_BIAS_RELU = os.environ.get("IPPMARL_FUSED_BIAS_RELU", "1") != "0"
# conv2's input gradient as GEMM + col2im (see _ConvDataGradAsGemm); IPPMARL_CONV2_BWD_GEMM=0 keeps the library's kernel
CONV2_BWD_DATA_AS_GEMM = os.environ.get("IPPMARL_CONV2_BWD_GEMM", "1") != "0"


# conv2 of a forward-with-gradient pass: "float32" (the library's convolution, the default) or "bf16" (libippmarl's matrix-core kernels,
# see _Conv4x4Bf16).  The mode belongs to the CALLER of the forward -- a learner enters conv2_update(mode) around it -- and is neither
# process-global nor stored in the module: whole-module pickles are the checkpoint format.
CONV2_UPDATE_ENV, CONV2_UPDATE_MODES = switches.TABLE["conv2_update"][:2]
_CONV2_UPDATE: "contextvars.ContextVar[str]" = contextvars.ContextVar("ippmarl_conv2_update", default="float32")


def resolve_conv2_update(conv2_update: Optional[str] = None) -> str:
    """The update's conv2 path: the argument, else IPPMARL_CONV2_UPDATE, else "float32"; anything but "float32" / "bf16" raises."""
    return switches.resolve("conv2_update", conv2_update)


@contextlib.contextmanager
def conv2_update(mode: str):
    """Forwards with gradients run inside this block take ``mode`` for conv2 ("bf16" only where _Conv4x4Bf16.usable says so: device
    float32 channels-last tensors under grad mode; everything else silently keeps the float32 path)."""
    if mode not in CONV2_UPDATE_MODES:
        raise ValueError(f"conv2 update must be one of {CONV2_UPDATE_MODES}, got {mode!r}")
    token = _CONV2_UPDATE.set(mode)
    try:
        yield
    finally:
        _CONV2_UPDATE.reset(token)


# conv1, conv2 and conv3 of a forward-with-gradient pass: "float32" (the default: whatever conv2_update says for conv2, the float32
# library for the rest) or "bf16" (conv1 through _Conv5x5Bf16, conv2 through _Conv4x4Bf16 whatever conv2_update says, conv3 through
# _Conv3Bf16).  The rules of the conv2 switch: the mode belongs to the caller of the forward and is never stored in the module.
TRUNK_UPDATE_ENV, TRUNK_UPDATE_MODES = switches.TABLE["trunk_update"][:2]
_TRUNK_UPDATE: "contextvars.ContextVar[str]" = contextvars.ContextVar("ippmarl_trunk_update", default="float32")


def resolve_trunk_update(trunk_update: Optional[str] = None) -> str:
    """The update's trunk path: the argument, else IPPMARL_TRUNK_UPDATE, else "float32"; anything but "float32" / "bf16" raises."""
    return switches.resolve("trunk_update", trunk_update)


@contextlib.contextmanager
def trunk_update(mode: str):
    """Forwards with gradients run inside this block take ``mode`` for conv1, conv2 and conv3 ("bf16" only where the three Functions'
    ``usable`` say so: device float32 channels-last tensors under grad mode; everything else silently keeps the float32 path)."""
    if mode not in TRUNK_UPDATE_MODES:
        raise ValueError(f"trunk update must be one of {TRUNK_UPDATE_MODES}, got {mode!r}")
    token = _TRUNK_UPDATE.set(mode)
    try:
        yield
    finally:
        _TRUNK_UPDATE.reset(token)


# Everything behind conv3 of a forward-with-gradient pass -- fc1, ReLU, fc3 (and, in the learners, the loss): "float32" (the default:
# PyTorch's GEMMs and elementwise passes) or "bf16" (libippmarl's head kernels, see _HeadBf16).  The rules of the other two switches:
# the mode belongs to the caller of the forward and is never stored in the module.  Independent of conv2_update and trunk_update.
HEAD_UPDATE_ENV, HEAD_UPDATE_MODES = switches.TABLE["head_update"][:2]
_HEAD_UPDATE: "contextvars.ContextVar[str]" = contextvars.ContextVar("ippmarl_head_update", default="float32")


def resolve_head_update(head_update: Optional[str] = None) -> str:
    """The update's head path: the argument, else IPPMARL_HEAD_UPDATE, else "float32"; anything but "float32" / "bf16" raises."""
    return switches.resolve("head_update", head_update)


@contextlib.contextmanager
def head_update(mode: str):
    """Forwards with gradients run inside this block take ``mode`` for fc1, ReLU and fc3 ("bf16" only where _HeadBf16.usable says so:
    device float32 contiguous tensors under grad mode; everything else silently keeps the float32 path)."""
    if mode not in HEAD_UPDATE_MODES:
        raise ValueError(f"head update must be one of {HEAD_UPDATE_MODES}, got {mode!r}")
    token = _HEAD_UPDATE.set(mode)
    try:
        yield
    finally:
        _HEAD_UPDATE.reset(token)


def epsilon_schedule(params: Dict, num_episode: int) -> float:
    """Linear anneal eps_max -> eps_min over eps_anneal_phase episodes (actor/network.py:53-58)."""
    m = params["experiment"]["missions"]
    if num_episode > m["eps_anneal_phase"]:
        return m["eps_min"]
    return m["eps_max"] - num_episode / m["eps_anneal_phase"] * (m["eps_max"] - m["eps_min"])


# ActorNetwork.get_action_index: the team's action probabilities of the sweep in progress, per network object (kept out of the
# module's __dict__: whole-module pickles are the reference's checkpoint format)
import weakref  # noqa: E402

_TEAM_PROBS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


class _ConvDataGradAsGemm(torch.autograd.Function):
    """conv2d whose INPUT gradient is a GEMM + col2im instead of the library's implicit-GEMM backward-data kernel.

    Measured on MI355X (profiles/r02/coma_update_flops.json): MIOpen's float32 forward and weight-gradient kernels run this
    4x4 convolution at 132 / 136 TFLOP/s (84-87 % of the float32 matrix peak), its backward-data kernel at 48 -- 44 % of a
    COMA update's kernel time.  The input gradient of a stride-1 convolution is  fold(grad_out[B*L, O] x W[O, C*kh*kw])  (L =
    output positions): one hipBLASLt GEMM at the forward's rate plus a memory-bound scatter.  Forward, weight and bias
    gradients stay with the library."""

    COLS_LIMIT = 3 << 30   # bytes of the column matrix of one slice (below the 4 GB at which 32-bit byte offsets wrap)

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return torch.nn.functional.conv2d(x, weight, bias)

    @staticmethod
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        grad_x = grad_w = grad_b = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            _, grad_w, grad_b = torch.ops.aten.convolution_backward(
                grad_out, x, weight, [weight.shape[0]], [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                [False, True, bool(ctx.needs_input_grad[2])])
            if not ctx.needs_input_grad[2]:
                grad_b = None
        if ctx.needs_input_grad[0]:
            B, O, Ho, Wo = grad_out.shape
            C, K = weight.shape[1], weight.shape[2]
            g = grad_out.permute(0, 2, 3, 1).reshape(B * Ho * Wo, O)                  # [B*L, O] (a view for channels-last)
            if grad_out.is_cuda and C % 4 == 0 and weight.shape[2] == weight.shape[3]:
                # tap-major, channel-minor columns: the gather kernel of libippmarl reads and writes channels-last rows.
                # The column matrix is K*K times the size of grad_out (3.2 GB for a 12 288-sample minibatch of conv2): batches
                # whose columns would pass COLS_LIMIT bytes go through in slices of the batch
                from . import _ffi
                lib, stream = _ffi.load_library(), torch.cuda.current_stream(grad_out.device).cuda_stream
                w2 = weight.permute(0, 2, 3, 1).reshape(O, -1)                        # [O, K*K*C]
                grad_x = torch.empty(B, Ho + K - 1, Wo + K - 1, C, dtype=grad_out.dtype, device=grad_out.device)
                g = g.contiguous()
                per_sample = Ho * Wo * K * K * C * g.element_size()
                step = max(1, min(B, _ConvDataGradAsGemm.COLS_LIMIT // per_sample))
                for lo in range(0, B, step):
                    nb = min(step, B - lo)
                    cols = g[lo * Ho * Wo:(lo + nb) * Ho * Wo] @ w2                   # [nb*L, K*K*C]
                    _ffi.check(lib.ippm_col2im_nhwc(_ffi.ptr(cols), grad_x[lo:lo + nb].data_ptr(), nb, Ho, Wo, K, C, stream), "ippm_col2im_nhwc")
                grad_x = grad_x.permute(0, 3, 1, 2)                                   # logical NCHW, channels-last strides
            else:
                cols = g @ weight.reshape(O, -1)                                       # [B*L, C*kh*kw]
                cols = cols.view(B, Ho * Wo, -1).transpose(1, 2)                       # [B, C*kh*kw, L]
                grad_x = torch.nn.functional.fold(cols, x.shape[-2:], weight.shape[-2:])
        return grad_x, grad_w, grad_b


def _scratch(bytes_entry: str, args: tuple, device) -> torch.Tensor:
    """The scratch tensor of a bf16 entry point family: the library's ``bytes_entry(*args, &bytes)`` is asked for the size."""
    from . import _ffi
    nbytes = ctypes.c_int64(0)
    _ffi.check(getattr(_ffi.load_library(), bytes_entry)(*args, ctypes.addressof(nbytes)), bytes_entry)
    return torch.empty(nbytes.value, dtype=torch.uint8, device=device)


class _Conv4x4Bf16(torch.autograd.Function):
    """Bias-free conv2 (4x4, 256 -> 256 channels, stride 1, no padding) whose forward, input gradient and weight gradient run on the
    bf16 matrix cores (libippmarl's ippm_conv4x4_bf16_*, csrc/conv4x4_train.hip) instead of the library's float32 convolution.
    Contract: x, weight and grad_out are rounded to bf16 on their way in, products accumulate in float32, outputs
    are float32; deterministic, no atomics.  Tensors are logical NCHW over channels-last storage, as everywhere in the trunk.  No host
    synchronisation; the scratch is allocated per call, so the calls record into a hipGraph like the rest of the round."""

    @staticmethod
    def usable(x: torch.Tensor, weight: torch.Tensor) -> bool:
        return (torch.is_grad_enabled() and weight.requires_grad and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
                and x.shape[0] >= 1 and tuple(weight.shape) == (256, 256, 4, 4) and x.shape[1] == 256 and weight.dtype == torch.float32
                and weight.device == x.device and 4 <= x.shape[2] <= 11 and 4 <= x.shape[3] <= 11 and not x.is_sparse
                and x.is_contiguous(memory_format=torch.channels_last))

    @staticmethod
    def _call(name: str, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, batch: int, ih: int, iw: int, partials: bool):
        from . import _ffi
        lib = _ffi.load_library()
        # (forward and input gradient use the weight packs at the head of the scratch only: the size of a one-sample call)
        scratch = _scratch("ippm_conv4x4_bf16_scratch_bytes", (batch if partials else 1, ih, iw), out.device)
        _ffi.check(getattr(lib, name)(a.data_ptr(), b.data_ptr(), batch, ih, iw, scratch.data_ptr(), out.data_ptr(),
                                      torch.cuda.current_stream(out.device).cuda_stream), name)
        return out

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        xs, w = x.contiguous(memory_format=torch.channels_last), weight.contiguous()
        B, _, ih, iw = xs.shape
        y = torch.empty((B, 256, ih - 3, iw - 3), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        return _Conv4x4Bf16._call("ippm_conv4x4_bf16_forward", xs, w, y, B, ih, iw, False)

    @staticmethod
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        xs, w = x.contiguous(memory_format=torch.channels_last), weight.contiguous()
        g = grad_out.contiguous(memory_format=torch.channels_last)
        B, _, ih, iw = xs.shape
        grad_x = grad_w = None
        if ctx.needs_input_grad[1]:
            grad_w = _Conv4x4Bf16._call("ippm_conv4x4_bf16_grad_weight", g, xs, torch.empty_like(w), B, ih, iw, True)
        if ctx.needs_input_grad[0]:
            grad_x = _Conv4x4Bf16._call("ippm_conv4x4_bf16_grad_input", g, w, torch.empty_like(xs), B, ih, iw, False)
        return grad_x, grad_w


class _Conv3Bf16(torch.autograd.Function):
    """Bias-free conv3 under trunk_update("bf16"): a 4x4 kernel over a 4x4 map, one output position.  x is logical [B,256,4,4] over
    channels-last storage, the result [B,256].  Forward and input gradient go through the 4x4 entry points of _Conv4x4Bf16 (ih = iw = 4),
    which tools/trunk_update_ab.py measured 1.6 x and 2.3 x ahead of the default path's float32 GEMMs at config 3's minibatch; the weight
    gradient (K = 256 rows per partial sum, 4 MiB of partial sums per 256 samples) only ties there and stays the float32 GEMM on the
    unrounded operands (profiles/r12/README.md)."""

    @staticmethod
    def usable(x: torch.Tensor, weight: torch.Tensor) -> bool:
        return _Conv4x4Bf16.usable(x, weight) and tuple(x.shape[2:]) == (4, 4)

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        xs, w = x.contiguous(memory_format=torch.channels_last), weight.contiguous()
        B = xs.shape[0]
        return _Conv4x4Bf16._call("ippm_conv4x4_bf16_forward", xs, w, torch.empty((B, 256), dtype=x.dtype, device=x.device), B, 4, 4, False)

    @staticmethod
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        xs, w = x.contiguous(memory_format=torch.channels_last), weight.contiguous()
        g = grad_out.contiguous()                                                       # [B,256]
        B = xs.shape[0]
        grad_x = grad_w = None
        if ctx.needs_input_grad[1]:
            # [256, (ty, tx, c)] from the channels-last activation flattened as a view, then PyTorch's [256,256,4,4]
            grad_w = (g.t() @ xs.permute(0, 2, 3, 1).reshape(B, -1)).view(256, 4, 4, 256).permute(0, 3, 1, 2).contiguous()
        if ctx.needs_input_grad[0]:
            grad_x = _Conv4x4Bf16._call("ippm_conv4x4_bf16_grad_input", g, w, torch.empty_like(xs), B, 4, 4, False)
        return grad_x, grad_w


class _Conv5x5Bf16(torch.autograd.Function):
    """relu(conv1(x) + bias) (5x5, 7 or 12 planes -> 256 channels, 11x11 -> 7x7) whose forward -- bias and ReLU fused into its store -- and
    weight gradient run on the bf16 matrix cores (libippmarl's ippm_conv5x5_bf16_*, csrc/conv5x5_train.hip).  Contract (DESIGN.md section
    7): x, weight and the gradient behind the ReLU are rounded to bf16 on their way in, products accumulate in float32, outputs are
    float32; deterministic, no atomics.  The backward is ippm_bias_relu_backward_nhwc on the saved output (the gradient through the ReLU,
    the bias gradient), then the weight gradient; the input is data and gets none.  No host synchronisation; the scratch is allocated per
    call, so the calls record into a hipGraph like the rest of the round."""

    @staticmethod
    def usable(x: torch.Tensor, weight: torch.Tensor, bias) -> bool:
        return (FUSED_BIAS_RELU and torch.is_grad_enabled() and weight.requires_grad and bias is not None and x.is_cuda
                and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] >= 1 and x.shape[1] in (7, 12)
                and tuple(x.shape[2:]) == (11, 11) and tuple(weight.shape) == (256, x.shape[1], 5, 5) and weight.dtype == torch.float32
                and bias.dtype == torch.float32 and weight.device == x.device and bias.device == x.device and not x.is_sparse
                and not x.requires_grad and x.is_contiguous(memory_format=torch.channels_last))

    @staticmethod
    def forward(ctx, x, weight, bias):
        from . import _ffi
        lib = _ffi.load_library()
        xs, w, b = x.contiguous(memory_format=torch.channels_last), weight.detach().contiguous(), bias.detach().contiguous()
        if xs.data_ptr() % 16:                            # (a view into a larger buffer: a sample is 847 or 1452 floats)
            xs = xs.clone(memory_format=torch.channels_last)
        B, planes = xs.shape[0], xs.shape[1]
        y = torch.empty((B, 256, 7, 7), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        # (the forward uses the weight pack at the head of the scratch only: the size of a one-sample call minus its partial sums)
        scratch = _scratch("ippm_conv5x5_bf16_scratch_bytes", (1, planes), x.device)
        _ffi.check(lib.ippm_conv5x5_bf16_forward(xs.data_ptr(), w.data_ptr(), b.data_ptr(), B, planes, scratch.data_ptr(), y.data_ptr(),
                                                 torch.cuda.current_stream(x.device).cuda_stream), "ippm_conv5x5_bf16_forward")
        ctx.save_for_backward(xs, y)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        from . import _ffi
        xs, y = ctx.saved_tensors
        lib, stream = _ffi.load_library(), torch.cuda.current_stream(y.device).cuda_stream
        B, planes = xs.shape[0], xs.shape[1]
        g = grad_y.contiguous(memory_format=torch.channels_last)
        grad_pre = torch.empty_like(y)                    # channels-last like y
        grad_b = torch.zeros(256, dtype=y.dtype, device=y.device)
        _ffi.check(lib.ippm_bias_relu_backward_nhwc(g.data_ptr(), y.data_ptr(), grad_pre.data_ptr(), _ffi.ptr(grad_b), B * 49, 256, stream),
                   "ippm_bias_relu_backward_nhwc")
        grad_w = _Conv5x5Bf16.grad_weight(grad_pre, xs) if ctx.needs_input_grad[1] else None
        return None, grad_w, (grad_b if ctx.needs_input_grad[2] else None)

    @staticmethod
    def grad_weight(grad_pre: torch.Tensor, xs: torch.Tensor) -> torch.Tensor:
        """The weight gradient [256,planes,5,5] of the bias-free convolution at the channels-last input ``xs`` for the output gradient
        ``grad_pre`` (channels-last, 16-byte aligned both)."""
        from . import _ffi
        lib = _ffi.load_library()
        B, planes = xs.shape[0], xs.shape[1]
        grad_w = torch.empty((256, planes, 5, 5), dtype=xs.dtype, device=xs.device)
        scratch = _scratch("ippm_conv5x5_bf16_scratch_bytes", (B, planes), xs.device)
        _ffi.check(lib.ippm_conv5x5_bf16_grad_weight(grad_pre.data_ptr(), xs.data_ptr(), B, planes, scratch.data_ptr(), grad_w.data_ptr(),
                                                     torch.cuda.current_stream(xs.device).cuda_stream), "ippm_conv5x5_bf16_grad_weight")
        return grad_w


def _loss_scratch(batch: int, device) -> torch.Tensor:
    """The first part of the head entry points' scratch for ``batch``, all that the two losses use (ippmarl.h)."""
    from . import _ffi
    chunks = (batch + _ffi.HEAD_WGRAD_CHUNK - 1) // _ffi.HEAD_WGRAD_CHUNK
    return torch.empty((chunks + 1) // 2 * 16, dtype=torch.uint8, device=device)


class _HeadBf16(torch.autograd.Function):
    """fc3(relu(fc1(h))) -> logits [B,A] whose forward is ONE kernel and whose backward is four (libippmarl's ippm_head_forward /
    ippm_head_backward, csrc/head_train.hip) instead of three library GEMMs forward and four backward with bias, threshold and reduction
    passes between them.  Contract: both operands of every product are rounded to bf16 on their way in, products
    accumulate in float32, everything else is float32; deterministic, no atomics.  No host synchronisation; the scratch is allocated per
    call, so the calls record into a hipGraph like the rest of the round."""

    @staticmethod
    def usable(h: torch.Tensor, fc1: nn.Linear, fc3: nn.Linear) -> bool:
        tensors = (h, fc1.weight, fc1.bias, fc3.weight, fc3.bias)
        return (torch.is_grad_enabled() and fc1.bias is not None and fc3.bias is not None and h.is_cuda and h.dim() == 2
                and h.shape[0] >= 1 and h.shape[1] == 256 and tuple(fc1.weight.shape) == (256, 256) and fc3.weight.dim() == 2
                and fc3.weight.shape[1] == 256 and 1 <= fc3.weight.shape[0] <= 32
                and all(t.dtype == torch.float32 and t.device == h.device and not t.is_sparse and t.is_contiguous() for t in tensors)
                and all(t.requires_grad for t in tensors[1:]))

    @staticmethod
    def forward(ctx, h, w1, b1, w3, b3):
        from . import _ffi
        lib = _ffi.load_library()
        hs, w1, b1, w3, b3 = (t.detach().contiguous() for t in (h, w1, b1, w3, b3))
        B, A = hs.shape[0], w3.shape[0]
        a1 = torch.empty((B, 256), dtype=h.dtype, device=h.device)
        logits = torch.empty((B, A), dtype=h.dtype, device=h.device)
        _ffi.check(lib.ippm_head_forward(hs.data_ptr(), w1.data_ptr(), b1.data_ptr(), w3.data_ptr(), b3.data_ptr(), B, A, None, a1.data_ptr(),
                                         logits.data_ptr(), torch.cuda.current_stream(h.device).cuda_stream), "ippm_head_forward")
        ctx.save_for_backward(hs, w1, w3, a1)
        return logits

    @staticmethod
    def backward(ctx, grad_logits):
        from . import _ffi
        hs, w1, w3, a1 = ctx.saved_tensors
        lib = _ffi.load_library()
        B, A = hs.shape[0], w3.shape[0]
        g = grad_logits.contiguous()
        gh, gw1, gw3 = torch.empty_like(hs), torch.empty_like(w1), torch.empty_like(w3)
        gb1 = torch.empty(256, dtype=hs.dtype, device=hs.device)
        gb3 = torch.empty(A, dtype=hs.dtype, device=hs.device)
        scratch = _scratch("ippm_head_scratch_bytes", (B, A), hs.device)
        _ffi.check(lib.ippm_head_backward(g.data_ptr(), None, a1.data_ptr(), hs.data_ptr(), w1.data_ptr(), w3.data_ptr(), B, A, scratch.data_ptr(),
                                          gh.data_ptr(), gw1.data_ptr(), gb1.data_ptr(), gw3.data_ptr(), gb3.data_ptr(),
                                          torch.cuda.current_stream(hs.device).cuda_stream), "ippm_head_backward")
        return (gh if ctx.needs_input_grad[0] else None), gw1, gb1, gw3, gb3


class _CriticLossBf16(torch.autograd.Function):
    """(q [B,A], action [B], td [B]) -> (loss = mean (q[b,a_b] - td_b)^2, q_chosen [B]) through ippm_critic_loss, which also writes the
    gradient of the loss with respect to q; the backward scales it, on the device, by the incoming gradient."""

    @staticmethod
    def forward(ctx, q, action, td):
        from . import _ffi
        lib = _ffi.load_library()
        qs, a32, t32 = q.detach().contiguous(), action.to(torch.int32).contiguous(), td.detach().float().contiguous().view(-1)
        B, A = qs.shape
        loss = torch.empty((), dtype=q.dtype, device=q.device)
        q_chosen = torch.empty(B, dtype=q.dtype, device=q.device)
        dq = torch.empty_like(qs)
        scratch = _loss_scratch(B, q.device)
        _ffi.check(lib.ippm_critic_loss(qs.data_ptr(), a32.data_ptr(), t32.data_ptr(), B, A, scratch.data_ptr(), loss.data_ptr(),
                                        q_chosen.data_ptr(), dq.data_ptr(), torch.cuda.current_stream(q.device).cuda_stream), "ippm_critic_loss")
        ctx.save_for_backward(dq)
        ctx.mark_non_differentiable(q_chosen)
        return loss, q_chosen

    @staticmethod
    def backward(ctx, grad_loss, _grad_q_chosen):
        (dq,) = ctx.saved_tensors
        return dq * grad_loss, None, None


class _ActorLossBf16(torch.autograd.Function):
    """(logits [B,A], q_values, mask, action, eps) -> (loss, adv [B]) of actor/learner.py:52-97 through ippm_actor_loss: softmax, the
    epsilon mix, K7's advantage, the mask-weighted mean, and the gradient of the loss with respect to the logits in one kernel; the
    backward scales that gradient, on the device, by the incoming one.  ``eps``: a float, or a device scalar (recorded rounds).
    ``probs_out`` (optional, float32 [B,A], contiguous): receives the epsilon-mixed probabilities the loss was formed from (the native
    metrics' pre-step policy)."""

    @staticmethod
    def forward(ctx, logits, q_values, mask, action, eps, probs_out=None):
        from . import _ffi
        lib = _ffi.load_library()
        ls, q32 = logits.detach().contiguous(), q_values.detach().float().contiguous()
        m8, a32 = mask.to(torch.uint8).contiguous(), action.to(torch.int32).contiguous()
        B, A = ls.shape
        loss = torch.empty((), dtype=ls.dtype, device=ls.device)
        adv = torch.empty(B, dtype=ls.dtype, device=ls.device)
        dlogits = torch.empty_like(ls)
        eps_dev = eps if isinstance(eps, torch.Tensor) else None
        scratch = _loss_scratch(B, ls.device)
        if probs_out is not None and (probs_out.dtype != ls.dtype or probs_out.numel() != B * A or not probs_out.is_contiguous()
                                      or probs_out.device != ls.device):
            raise _ffi.IppmError("_ActorLossBf16: probs_out must be a contiguous float32 [B,A] tensor on the logits' device")
        _ffi.check(lib.ippm_actor_loss(ls.data_ptr(), q32.data_ptr(), m8.data_ptr(), a32.data_ptr(), B, A, 0.0 if eps_dev is not None else float(eps),
                                       None if eps_dev is None else eps_dev.data_ptr(), scratch.data_ptr(), loss.data_ptr(), adv.data_ptr(),
                                       None if probs_out is None else probs_out.data_ptr(),
                                       dlogits.data_ptr(), torch.cuda.current_stream(ls.device).cuda_stream), "ippm_actor_loss")
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(adv)
        return loss, adv

    @staticmethod
    def backward(ctx, grad_loss, _grad_adv):
        (dlogits,) = ctx.saved_tensors
        return dlogits * grad_loss, None, None, None, None, None


class _BiasReLU(torch.autograd.Function):
    """relu(x + bias) for a channels-last activation tensor as ONE pass in each direction (libippmarl's ippm_bias_relu_nhwc
    / ippm_bias_relu_backward_nhwc) instead of the bias pass + ReLU pass (and threshold pass + column reduction) PyTorch runs
    around a MIOpen convolution.  ``x`` is the bias-free convolution output and is overwritten."""

    @staticmethod
    def usable(x: torch.Tensor, bias) -> bool:
        c = x.shape[1]
        return (FUSED_BIAS_RELU and bias is not None and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and c % 4 == 0
                and 256 % (c // 4) == 0 and x.is_contiguous(memory_format=torch.channels_last))

    @staticmethod
    def _lib():
        from . import _ffi
        return _ffi, _ffi.load_library()

    @staticmethod
    def forward(ctx, x, bias):
        ffi, lib = _BiasReLU._lib()
        b = bias.detach().contiguous()
        # (channels-last storage: dense [rows, C]; `usable` has checked that)
        ffi.check(lib.ippm_bias_relu_nhwc(x.data_ptr(), ffi.ptr(b), x.numel() // x.shape[1], x.shape[1],
                                          torch.cuda.current_stream(x.device).cuda_stream), "ippm_bias_relu_nhwc")
        ctx.mark_dirty(x)
        ctx.save_for_backward(x)
        return x

    @staticmethod
    def backward(ctx, grad_y):
        (y,) = ctx.saved_tensors
        ffi, lib = _BiasReLU._lib()
        g = grad_y.contiguous(memory_format=torch.channels_last)
        grad_x = torch.empty_like(y)                      # channels-last like y
        grad_b = torch.zeros(y.shape[1], dtype=y.dtype, device=y.device)
        ffi.check(lib.ippm_bias_relu_backward_nhwc(g.data_ptr(), y.data_ptr(), grad_x.data_ptr(), ffi.ptr(grad_b),
                                                   y.numel() // y.shape[1], y.shape[1],
                                                   torch.cuda.current_stream(y.device).cuda_stream), "ippm_bias_relu_backward_nhwc")
        return grad_x, grad_b


class _ConvTrunk(nn.Module):
    def __init__(self, in_planes: int, n_actions: int):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, 256, (5, 5))
        self.conv2 = nn.Conv2d(256, 256, (4, 4))
        self.conv3 = nn.Conv2d(256, 256, (4, 4))
        self.activation = nn.ReLU()
        self.flatten = nn.Flatten()
        self.fc1 = nn.Linear(256, 256)
        self.fc2 = nn.Linear(256, 256)  # never used in forward (reference: commented out) -> never gets a gradient
        self.fc3 = nn.Linear(256, n_actions)

    def _conv_relu(self, conv: nn.Conv2d, x: torch.Tensor, data_grad_as_gemm: bool, bf16_update: bool = False):
        """activation(conv(x)); on the device the convolution runs bias-free and bias + ReLU are one in-place pass.  ``bf16_update``:
        the bias-free convolution of a forward with gradients goes to _Conv4x4Bf16 where that is usable."""
        # (both paths below, and _ConvDataGradAsGemm's backward, are written for the unpadded stride-1 layers of the reference)
        assert tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (0, 0) and tuple(conv.dilation) == (1, 1) and conv.groups == 1
        conv2d = _ConvDataGradAsGemm.apply if data_grad_as_gemm else torch.nn.functional.conv2d
        if x.is_cuda and FUSED_BIAS_RELU:
            if bf16_update and conv.bias is not None and _Conv4x4Bf16.usable(x, conv.weight):
                out = _Conv4x4Bf16.apply(x, conv.weight)
            else:
                out = conv2d(x, conv.weight, None)
            if _BiasReLU.usable(out, conv.bias):
                return _BiasReLU.apply(out, conv.bias)
            return self.activation(out + conv.bias.view(1, -1, 1, 1))
        return self.activation(conv2d(x, conv.weight, conv.bias))

    # conv1's activation [B, 256, 7, 7] float32 is 50 176 bytes per sample: 2^31 bytes at 42 799 samples, 2^32 at 85 598, and
    # the library's convolution kernels address their tensors with 32-bit byte offsets (measured: one forward pass over 131 072
    # critic states returns the results of samples 85 598.. wrapped onto samples 0..: wrong Q values, no error).  Larger batches go
    # through in slices.
    MAX_SAMPLES = 32768

    def trunk(self, x: torch.Tensor):
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if x.shape[0] > self.MAX_SAMPLES:
            parts = [self.trunk(x[lo:lo + self.MAX_SAMPLES]) for lo in range(0, x.shape[0], self.MAX_SAMPLES)]
            return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        x = x.permute(0, 3, 1, 2)  # NHWC storage -> logical NCHW (channels_last strides, no copy)
        bf16_trunk = _TRUNK_UPDATE.get() == "bf16"
        if bf16_trunk and _Conv5x5Bf16.usable(x, self.conv1.weight, self.conv1.bias):
            h = _Conv5x5Bf16.apply(x, self.conv1.weight, self.conv1.bias)
        else:
            h = self._conv_relu(self.conv1, x, False)
        h = self._conv_relu(self.conv2, h, CONV2_BWD_DATA_AS_GEMM and h.requires_grad, bf16_trunk or _CONV2_UPDATE.get() == "bf16")
        if bf16_trunk and h.is_cuda and FUSED_BIAS_RELU and self.conv3.bias is not None and _Conv3Bf16.usable(h, self.conv3.weight):
            h = self.activation(_Conv3Bf16.apply(h, self.conv3.weight) + self.conv3.bias)
        elif CONV3_AS_GEMM and h.shape[-2:] == self.conv3.kernel_size:
            # conv3 sees a 4x4 map with a 4x4 kernel: ONE output position, i.e. a plain [B, 4096] x [4096, 256] product.
            # As a GEMM it goes to hipBLASLt instead of an implicit-GEMM convolution with a degenerate output tile.
            # (h is channels-last: flattening it in (H, W, C) order is a view; the weight is permuted to match.)
            w3 = self.conv3.weight.permute(0, 2, 3, 1).reshape(self.conv3.out_channels, -1)
            h = self.activation(torch.nn.functional.linear(h.permute(0, 2, 3, 1).reshape(h.shape[0], -1), w3, self.conv3.bias))
        else:
            h = self.flatten(self.activation(self.conv3(h)))
        if _HEAD_UPDATE.get() == "bf16" and _HeadBf16.usable(h, self.fc1, self.fc3):
            return _HeadBf16.apply(h, self.fc1.weight, self.fc1.bias, self.fc3.weight, self.fc3.bias), h
        return self.fc3(self.activation(self.fc1(h))), h


class ActorNetwork(_ConvTrunk):
    def __init__(self, params: Dict):
        self.params = params
        self.n_agents = params["experiment"]["missions"]["n_agents"]
        self.n_actions = params["experiment"]["constraints"]["num_actions"]
        super().__init__(7, self.n_actions)
        self.softmax = nn.Softmax(dim=1)
        # The plain attributes of the reference's class (actor/network.py:13-39).  A whole-module pickle of this object is
        # unpickled by the reference WITHOUT running its __init__ (checkpoint.save_actor), so everything its methods read --
        # get_action_index uses device and the epsilon schedule -- has to travel in our __dict__.
        m = params["experiment"]["missions"]
        self.mission_type = m["type"]
        self.hidden_dim = params["networks"]["actor"]["hidden_dim"]
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.log_softmax = nn.LogSoftmax(dim=1)
        self.hidden_states = [[]] * self.n_agents
        self.eps_max, self.eps_min, self.eps_anneal_phase, self.use_eps = m["eps_max"], m["eps_min"], m["eps_anneal_phase"], m["use_eps"]
        self.network_type = params["networks"]["type"]
        self.baseline = "no"

    def forward(self, input_state: torch.Tensor, eps: float):
        """-> ((1-eps) * softmax + eps / n_actions, hidden) (actor/network.py:70-88)."""
        logits, h = self.trunk(input_state)
        probs = self.softmax(logits)
        return (1 - eps) * probs + eps / self.n_actions, h

    def eps(self, num_episode: int) -> float:
        return epsilon_schedule(self.params, num_episode)

    def get_action_index(self, batch_memory, action_mask_1d, agent_id, t, num_episode: int, mode: str):
        """Single-agent action choice of the drop-in Agent.step (actor/network.py:41-68,90-96): masked eps-softmax,
        torch.multinomial in training, argmax in evaluation.
        The agents of a team are served one after the other within a step (coma_wrapper.py:97-104) and their observations are all
        in the memory before the first one acts (coma_wrapper.py:37-71), so the first call of a sweep runs ONE forward pass for the
        whole team and the following agents take their row of it (a batch-1 pass per agent was a quarter of the seam's step)."""
        device = self.conv1.weight.device
        eps = epsilon_schedule(self.params, num_episode)
        team = _TEAM_PROBS.get(self)
        key = (id(batch_memory), t, eps)
        if team is None or team[0] != key or agent_id <= team[1] or agent_id >= team[2].shape[0]:
            lens = {len(batch_memory.transitions[j]) for j in range(self.n_agents)} if hasattr(batch_memory, "transitions") else set()
            if len(lens) == 1 and agent_id == 0:       # every agent holds an observation of this step: the whole team at once
                obs = torch.stack([batch_memory.get(-1, j, "observation") for j in range(self.n_agents)]).to(device).float()
            else:
                obs = batch_memory.get(-1, agent_id, "observation").unsqueeze(0).to(device).float()
            with torch.no_grad():
                probs_all, _ = self.forward(obs, eps)
            team = [key, agent_id, probs_all if obs.shape[0] > 1 else None]
            row = probs_all[agent_id if obs.shape[0] > 1 else 0]
            if team[2] is None:
                team = None
        else:
            row = team[2][agent_id]
        if team is not None:
            team[1] = agent_id
        _TEAM_PROBS[self] = team
        mask = torch.as_tensor(action_mask_1d).to(device)
        probs = row * mask
        chosen = torch.argmax(probs) if mode == "eval" else torch.multinomial(probs, 1, replacement=True)
        return probs, chosen, mask, eps


class CriticNetwork(_ConvTrunk):
    def __init__(self, params: Dict):
        self.params = params
        self.n_agents = params["experiment"]["missions"]["n_agents"]
        self.n_actions = params["experiment"]["constraints"]["num_actions"]
        super().__init__(12, self.n_actions)

    def forward(self, input_state: torch.Tensor):
        """-> (Q [B,A], log_softmax over dim 0 (a metric the reference logs; critic/network.py:43-47))."""
        q, _ = self.trunk(input_state)
        q = q.squeeze()
        with torch.no_grad():
            log_probs = torch.log_softmax(q, dim=0)
        return q, log_probs
