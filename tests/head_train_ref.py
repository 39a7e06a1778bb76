"""Shared by test_head_update_cpu.py and test_hip_head_update.py: the numerical contract of the native heads of the COMA update
(csrc/head_train.hip; networks._HeadBf16, _CriticLossBf16, _ActorLossBf16) restated in PyTorch on the CPU, and the constructed inputs the
tests run.  Nothing here calls the code under test.

Contract: both operands of the six products (z1 = h W1^T, logits = a1 W3^T, ga1 = d W3, gh = gz1 W1, gW1 = gz1^T h,
gW3 = d^T a1, d = dlogits * scale) are rounded to bf16 and promoted to the accumulation type; everything else (bias adds, ReLU, the ReLU's
mask, the bias gradients, the losses) is plain arithmetic of that type on unrounded values.  ``float64`` is the reference; ``float32`` is a
second legitimate accumulation order, and the spread between the two is the unit the dense tolerances are stated in (``MARGIN`` spreads:
the value of tests/actor_native_ref.py)."""
import functools
import os
import re

import torch

from actor_native_ref import MARGIN  # noqa: F401

HID = 256
ACTION_SETS = (4, 6, 9, 27)              # the reference's action sets


def header_chunk():
    """IPPM_HEAD_WGRAD_CHUNK as include/ippmarl.h defines it (read as text: nothing is loaded)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ippmarl.h")
    with open(path) as f:
        return int(re.search(r"^#define IPPM_HEAD_WGRAD_CHUNK (\d+)$", f.read(), re.M).group(1))


CHUNK = header_chunk()
INT_MAX_BATCH = 2 * CHUNK + 3            # the largest batch of the small-integer gradient cases


def _bf16(t, dtype):
    return t.to(torch.bfloat16).to(dtype)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def forward(h, w1, b1, w3, b3, dtype):
    """-> (a1 [B,256], logits [B,A]) in ``dtype``"""
    a1 = torch.relu(_bf16(h, dtype) @ _bf16(w1, dtype).t() + b1.to(dtype))
    return a1, fc3(a1, w3, b3, dtype)


def fc3(a1, w3, b3, dtype):
    """logits = bf16(a1) bf16(W3)^T + b3 in ``dtype``"""
    return _bf16(a1, dtype) @ _bf16(w3, dtype).t() + b3.to(dtype)


def backward(dlogits, scale, a1, h, w1, w3, dtype):
    """-> {gh, gw1, gb1, gw3, gb3} in ``dtype`` for d = dlogits * scale; a1 is the forward's (its sign is the ReLU's mask)."""
    d = dlogits.to(dtype) * scale
    gz1 = (_bf16(d, dtype) @ _bf16(w3, dtype)) * (a1 > 0).to(dtype)
    return {"gh": _bf16(gz1, dtype) @ _bf16(w1, dtype), "gw1": _bf16(gz1, dtype).t() @ _bf16(h, dtype), "gb1": gz1.sum(0),
            "gw3": _bf16(d, dtype).t() @ _bf16(a1.to(dtype), dtype), "gb3": d.sum(0)}


def critic_loss(q, action, td, dtype):
    """critic/learner.py:76-92 -> {loss, q_chosen [B], dq [B,A]}"""
    q, td = q.to(dtype), td.to(dtype)
    idx = action.long().view(-1, 1)
    qc = q.gather(1, idx).squeeze(1)
    d = qc - td
    return {"loss": d.square().mean(), "q_chosen": qc, "dq": torch.zeros_like(q).scatter_(1, idx, (2 * d / q.shape[0]).view(-1, 1))}


def coma_advantage(p, q, mask, action):
    """K7 (actor/learner.py:55-83): pi~ = p mask / max(sum, 1e-5), floored at 1e-5; adv = q[a] - sum pi~ q mask"""
    m = mask.to(p.dtype)
    pm = p * m
    pn = (pm / pm.sum(1, keepdim=True).clamp_min(1e-5)).clamp_min(1e-5)
    return q.gather(1, action.long().view(-1, 1)).squeeze(1) - (pn * q * m).sum(1)


def actor_loss(logits, q, mask, action, eps, dtype):
    """actor/learner.py:52-97 -> {loss, adv [B], probs [B,A], dlogits [B,A]}; adv is not differentiated."""
    logits, q = logits.to(dtype), q.to(dtype)
    B, A = logits.shape
    idx = action.long().view(-1, 1)
    s = torch.softmax(logits, dim=1)
    p = (1 - eps) * s + eps / A
    adv = coma_advantage(p, q, mask, action)
    w = mask.to(dtype).sum(1) / A
    pc, sc = p.gather(1, idx).squeeze(1), s.gather(1, idx)
    onehot = torch.zeros_like(s).scatter_(1, idx, 1.0)
    coef = -(adv * w / B) * (1 - eps) * sc.squeeze(1) / pc
    return {"loss": -(adv * torch.log(pc) * w).mean(), "adv": adv, "probs": p, "dlogits": coef.view(-1, 1) * (onehot - s)}


# ---- the small-integer case: every partial sum is an integer below 2^24, so any accumulation order is exact ---------------------------
# 0 <= h <= 15, |w| <= 3, |b1| <= 40: |z1| <= 11520 and a1 <= 11560 (well past 256: rounded to bf16 by both sides, still an integer);
# |logits| <= 256 * 11560 * 3; |dlogits| <= 2: |gz1| <= 27 * 6 = 162 (exact in bf16), and the sums over INT_MAX_BATCH rows stay below
# 11560 * 2 * INT_MAX_BATCH (gW3) and 162 * 15 * INT_MAX_BATCH (gW1)
assert 256 * 11560 * 3 + 5 < 2 ** 24 and 11560 * 2 * INT_MAX_BATCH < 2 ** 24 and 162 * 3 * 256 < 2 ** 24 and CHUNK <= 256


def _ints(lo, hi, shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


@functools.lru_cache(maxsize=None)
def int_weights(A):
    """-> (w1, b1, w3, b3)"""
    return _ints(-3, 3, (HID, HID), 1), _ints(-40, 40, (HID,), 2), _ints(-3, 3, (A, HID), 3 + A), _ints(-5, 5, (A,), 40 + A)


@functools.lru_cache(maxsize=None)
def int_h(batch):
    return _ints(0, 15, (batch, HID), 100 + batch)


@functools.lru_cache(maxsize=None)
def int_dlogits(batch, A):
    return _ints(-2, 2, (batch, A), 200 + 31 * batch + A)


@functools.lru_cache(maxsize=None)
def int_forward(batch, A):
    return forward(int_h(batch), *int_weights(A), torch.float64)


@functools.lru_cache(maxsize=None)
def int_backward(batch, A, scale=1.0):
    assert batch <= INT_MAX_BATCH
    w1, _, w3, _ = int_weights(A)
    return backward(int_dlogits(batch, A), scale, int_forward(batch, A)[0], int_h(batch), w1, w3, torch.float64)


@functools.lru_cache(maxsize=None)
def int_critic(batch, A):
    """-> (q, action, td), |q|, |td| <= 8: the squared errors are integers <= 256 and the batch is a power of two"""
    assert batch & (batch - 1) == 0
    g = torch.Generator().manual_seed(300 + batch + A)
    return _ints(-8, 8, (batch, A), 301 + batch + A), torch.randint(0, A, (batch,), generator=g).int(), _ints(-8, 8, (batch,), 302 + batch + A)


# ---- the dense real case ---------------------------------------------------------------------------------------------------------------------
DENSE_SEEDS, DENSE_BATCH, DENSE_ACTIONS, DENSE_EPS = (1, 2, 3), 300, 6, 0.25


@functools.lru_cache(maxsize=None)
def dense_inputs(seed, A=DENSE_ACTIONS, batch=DENSE_BATCH):
    """He-normal weights, N(0, 0.1) biases (as trunk_train_ref.dense_inputs), h = relu(randn) (conv3's activation), td and the actor's Q
    N(0, 1), masks with 70 % valid actions and the chosen action always valid."""
    g = torch.Generator().manual_seed(1000 * seed + A)
    w1, b1 = torch.randn(HID, HID, generator=g) * (2.0 / HID) ** 0.5, torch.randn(HID, generator=g) * 0.1
    w3, b3 = torch.randn(A, HID, generator=g) * (2.0 / HID) ** 0.5, torch.randn(A, generator=g) * 0.1
    h = torch.relu(torch.randn(batch, HID, generator=g))
    action = torch.randint(0, A, (batch,), generator=g).int()
    mask = (torch.rand(batch, A, generator=g) < 0.7).to(torch.uint8)
    mask.scatter_(1, action.long().view(-1, 1), 1)
    return dict(h=h, w1=w1, b1=b1, w3=w3, b3=b3, action=action, mask=mask, td=torch.randn(batch, generator=g),
                q_values=torch.randn(batch, A, generator=g))


def spreads(fn):
    """fn(dtype) -> {output: tensor}; -> {output: (max |fn(float32) - fn(float64)|, fn(float64))}"""
    r32, r64 = fn(torch.float32), fn(torch.float64)
    return {k: (float((r32[k].double() - r64[k]).abs().max()), r64[k]) for k in r64}


# ---- the seam: a CPU network whose head is the restatement ---------------------------------------------------------------------------------
class RestatedHead(torch.autograd.Function):
    """(h, w1, b1, w3, b3) -> logits as one differentiable step of a CPU network, in the dtype of its input."""

    @staticmethod
    def forward(ctx, h, w1, b1, w3, b3):
        a1, logits = forward(h, w1, b1, w3, b3, h.dtype)
        ctx.save_for_backward(h, w1, w3, a1)
        return logits

    @staticmethod
    def backward(ctx, g):
        h, w1, w3, a1 = ctx.saved_tensors
        r = backward(g, 1.0, a1, h, w1, w3, h.dtype)
        return r["gh"], r["gw1"], r["gb1"], r["gw3"], r["gb3"]


class RestatedLoss(torch.autograd.Function):
    """The learners' loss on the head's output with the restated gradient (adv is not differentiated): ``spec`` is ("critic", action, td)
    or ("actor", q_values, mask, action, eps).  -> (loss, q_chosen or adv)"""

    @staticmethod
    def forward(ctx, logits, spec):
        r = critic_loss(logits, spec[1], spec[2], logits.dtype) if spec[0] == "critic" else actor_loss(logits, *spec[1:], logits.dtype)
        ctx.save_for_backward(r["dq" if spec[0] == "critic" else "dlogits"])
        return r["loss"], r["q_chosen" if spec[0] == "critic" else "adv"].clone()

    @staticmethod
    def backward(ctx, g, _):
        return ctx.saved_tensors[0] * g, None


def net_grads(net, inputs, spec, dtype, bf16_trunk=False):
    """The loss, its by-product and the gradients of the ten used parameters of a convnet of networks._ConvTrunk's shape on the CPU in
    ``dtype``: plain convolutions (or trunk_train_ref's restated ones), the restated head and loss.  net: {layer: (weight, bias)} float32
    -> (loss, q_chosen or adv, {"conv1.weight": grad, ...})"""
    import torch.nn.functional as F
    import trunk_train_ref as T
    p = {f"{n}.{k}": t.to(dtype).clone().requires_grad_(True) for n, (w, b) in net.items() for k, t in (("weight", w), ("bias", b))}
    h = inputs.to(dtype).permute(0, 3, 1, 2)
    for name in ("conv1", "conv2", "conv3"):
        conv = T.RestatedConv.apply(h, p[f"{name}.weight"], T.BF16_WEIGHT_GRADIENT[name]) if bf16_trunk else F.conv2d(h, p[f"{name}.weight"])
        h = torch.relu(conv + p[f"{name}.bias"].view(1, -1, 1, 1))
    logits = RestatedHead.apply(h.flatten(1), p["fc1.weight"], p["fc1.bias"], p["fc3.weight"], p["fc3.bias"])
    loss, side = RestatedLoss.apply(logits, spec)
    loss.backward()
    return loss.detach(), side.detach(), {k: t.grad for k, t in p.items()}
