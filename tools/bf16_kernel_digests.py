#!/usr/bin/env python
"""Digests of everything the bf16 matrix-core entry points compute, for comparing two builds of the library bit for bit: the existing
tests bound the error on dense inputs, so a reordered sum would pass them; two libraries whose digests agree computed the same bits.

Every entry point (ippm_actor_forward, ippm_critic_forward, ippm_conv4x4_bf16_*, ippm_conv5x5_bf16_*, ippm_head_forward,
ippm_head_backward, ippm_critic_loss, ippm_actor_loss) is called through _ffi on seeded dense inputs at the smallest shapes that reach
every branch of the tile (partial row tiles, chunk edges of the weight gradients, every tap set of the input gradient), twice: "finite"
-- normal draws with rounding ties, the smallest normal and subnormals from tests/bf16_operand_classes_ref.py's lists cycled through
every 97th element -- and "salted" -- the same plus NaNs of three payloads, +Inf and -Inf in the last sample.  One JSON line per case
with the sha256 of each output tensor and the number of its non-finite elements.  The library is the one IPPMARL_LIB names (default: lib/libippmarl.so):

    IPPMARL_LIB=/path/to/libippmarl_parent.so python tools/bf16_kernel_digests.py > parent.jsonl
    python tools/bf16_kernel_digests.py > new.jsonl && cmp parent.jsonl new.jsonl"""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ipp-marl_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bf16_operand_classes_ref as OC  # noqa: E402
from ippmarl import _ffi  # noqa: E402

DEV = torch.device("cuda:0")
# finite values that keep a sum of thousands of products finite: the lists' patterns below 4 in magnitude, and subnormals
_MILD = [v for v in OC.pattern_values("signed-finite").tolist() if abs(v) < 4.0] + [1e-40, -1e-40, 1.4e-45]
_SALT = np.array([0x7FC00000, 0x7FC12345, 0xFF812345, 0x7F800000, 0xFF800000], dtype=np.uint32).view(np.float32)


def dense(gen, shape, scale, salted, start):
    """Normal draws * scale; every 97th element one of the mild patterns; salted: the five non-finite values in the last sample."""
    t = torch.randn(shape, generator=gen) * scale
    flat = t.view(-1)
    idx = torch.arange(min(start % 97, flat.numel()), flat.numel(), 97)
    flat[idx] = torch.tensor(_MILD, dtype=torch.float32)[(idx // 97 + start) % len(_MILD)]
    if salted:
        per = flat.numel() // shape[0]
        where = (shape[0] - 1) * per + (torch.arange(len(_SALT)) * 1009 + start) % per
        flat[where] = torch.from_numpy(_SALT.copy())
    return t.to(DEV)


TAG = {False: "finite", True: "salted"}


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def scratch(lib, name, *args):
    nbytes = ctypes.c_int64(0)
    _ffi.check(getattr(lib, name)(*args, ctypes.addressof(nbytes)), name)
    return torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)


def call(lib, name, *args):
    _ffi.check(getattr(lib, name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], None), name)


def emit(case, **outs):
    torch.cuda.synchronize()
    print(json.dumps({"case": case, **{k: digest(v) for k, v in outs.items()},
                      "nonfinite": {k: int((~torch.isfinite(v)).sum()) for k, v in outs.items()}}), flush=True)


def inference(lib, gen, kind, A, B, salted):
    planes = OC.PLANES[kind]
    shapes = [(256, planes, 5, 5), (256,), (256, 256, 4, 4), (256,), (256, 256, 4, 4), (256,), (256, 256), (256,), (A, 256), (A,)]
    params = [dense(gen, s, (2.0 / max(1, int(np.prod(s[1:])))) ** 0.5 if len(s) > 1 else 0.1, False, i) for i, s in enumerate(shapes)]
    packed = scratch(lib, f"ippm_{kind}_pack_bytes", A)
    call(lib, f"ippm_{kind}_pack", *params, A, packed)
    x = dense(gen, (B, 11, 11, planes), 1.0, salted, 3)
    sc = scratch(lib, f"ippm_{kind}_scratch_bytes", B)
    out = torch.empty((B, A), device=DEV)
    if kind == "actor":
        logits = torch.empty((B, A), device=DEV)
        call(lib, "ippm_actor_forward", packed, x, B, A, 0.3, None, sc, out, logits)
        emit(f"actor_forward/A{A}/B{B}/{TAG[salted]}", probs=out, logits=logits)
    else:
        action = torch.randint(0, A, (B,), generator=gen).int().to(DEV)
        q_sel = torch.empty(B, device=DEV)
        call(lib, "ippm_critic_forward", packed, x, B, A, action, sc, out, q_sel)
        emit(f"critic_forward/A{A}/B{B}/{TAG[salted]}", q=out, q_sel=q_sel)


def conv4x4(lib, gen, salted):
    w = dense(gen, (256, 256, 4, 4), (2.0 / 4096) ** 0.5, False, 1)
    for ih, iw in ((4, 4), (7, 7), (5, 6)):
        for B in (1, 9, 129):
            x = dense(gen, (B, ih, iw, 256), 1.0, salted, 2)
            gy = dense(gen, (B, ih - 3, iw - 3, 256), 1.0, salted, 5)
            sc = scratch(lib, "ippm_conv4x4_bf16_scratch_bytes", B, ih, iw)
            y, gx = torch.empty_like(gy), torch.empty_like(x)
            call(lib, "ippm_conv4x4_bf16_forward", x, w, B, ih, iw, sc, y)
            call(lib, "ippm_conv4x4_bf16_grad_input", gy, w, B, ih, iw, sc, gx)
            emit(f"conv4x4/{ih}x{iw}/B{B}/{TAG[salted]}", y=y, gx=gx)
    for (ih, iw), B in [((7, 7), b) for b in (1, 255, 256, 257)] + [((4, 4), 1)]:
        x = dense(gen, (B, ih, iw, 256), 1.0, salted, 2)
        gy = dense(gen, (B, ih - 3, iw - 3, 256), 1.0, salted, 5)
        sc = scratch(lib, "ippm_conv4x4_bf16_scratch_bytes", B, ih, iw)
        gw = torch.empty_like(w)
        call(lib, "ippm_conv4x4_bf16_grad_weight", gy, x, B, ih, iw, sc, gw)
        emit(f"conv4x4_grad_weight/{ih}x{iw}/B{B}/{TAG[salted]}", gw=gw)


def conv5x5(lib, gen, salted):
    for planes in (7, 12):
        w = dense(gen, (256, planes, 5, 5), (2.0 / (25 * planes)) ** 0.5, False, 1)
        bias = dense(gen, (256,), 0.1, False, 4)
        for B in (1, 3):
            x = dense(gen, (B, 11, 11, planes), 1.0, salted, 2)
            sc = scratch(lib, "ippm_conv5x5_bf16_scratch_bytes", B, planes)
            y, yb = torch.empty((B, 7, 7, 256), device=DEV), torch.empty((B, 7, 7, 256), device=DEV)
            call(lib, "ippm_conv5x5_bf16_forward", x, w, None, B, planes, sc, y)
            call(lib, "ippm_conv5x5_bf16_forward", x, w, bias, B, planes, sc, yb)
            emit(f"conv5x5_forward/P{planes}/B{B}/{TAG[salted]}", y=y, y_bias_relu=yb)
        for B in (1, 63, 64, 65):
            x = dense(gen, (B, 11, 11, planes), 1.0, salted, 2)
            gy = dense(gen, (B, 7, 7, 256), 1.0, salted, 5)
            sc = scratch(lib, "ippm_conv5x5_bf16_scratch_bytes", B, planes)
            gw = torch.empty_like(w)
            call(lib, "ippm_conv5x5_bf16_grad_weight", gy, x, B, planes, sc, gw)
            emit(f"conv5x5_grad_weight/P{planes}/B{B}/{TAG[salted]}", gw=gw)


def head(lib, gen, salted):
    for A in (1, 6, 32):
        w1, b1 = dense(gen, (256, 256), (2.0 / 256) ** 0.5, False, 1), dense(gen, (256,), 0.1, False, 2)
        w3, b3 = dense(gen, (A, 256), (2.0 / 256) ** 0.5, False, 3), dense(gen, (A,), 0.1, False, 4)
        for B in (1, 63, 64, 65):
            h = dense(gen, (B, 256), 1.0, salted, 5)
            sc = scratch(lib, "ippm_head_scratch_bytes", B, A)
            a1, logits = torch.empty((B, 256), device=DEV), torch.empty((B, A), device=DEV)
            call(lib, "ippm_head_forward", h, w1, b1, w3, b3, B, A, sc, a1, logits)
            action = torch.randint(0, A, (B,), generator=gen).int().to(DEV)
            td, qv = dense(gen, (B,), 1.0, salted, 6), dense(gen, (B, A), 1.0, False, 7)
            mask = (torch.rand(B, A, generator=gen) < 0.7).to(torch.uint8).to(DEV)
            mask.scatter_(1, action.long().view(-1, 1), 1)
            loss_c, loss_a = torch.empty((), device=DEV), torch.empty((), device=DEV)
            q_chosen, adv = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
            dq, dlogits, probs = torch.empty_like(logits), torch.empty_like(logits), torch.empty_like(logits)
            call(lib, "ippm_critic_loss", logits, action, td, B, A, sc, loss_c, q_chosen, dq)
            call(lib, "ippm_actor_loss", logits, qv, mask, action, B, A, 0.3, None, sc, loss_a, adv, probs, dlogits)
            outs = {"a1": a1, "logits": logits, "critic_loss": loss_c, "q_chosen": q_chosen, "dq": dq, "actor_loss": loss_a, "adv": adv,
                    "probs": probs, "dlogits": dlogits}
            for which, d in (("critic", dq), ("actor", dlogits)):
                g = [torch.empty_like(t) for t in (h, w1, b1, w3, b3)]
                call(lib, "ippm_head_backward", d, None, a1, h, w1, w3, B, A, sc, *g)
                outs.update({f"{which}_{n}": t for n, t in zip(("gh", "gw1", "gb1", "gw3", "gb3"), g)})
            emit(f"head/A{A}/B{B}/{TAG[salted]}", **outs)


def main():
    lib = _ffi.load_library()
    for salted in ("finite", "salted"):
        gen = torch.Generator().manual_seed(20)
        for kind in ("actor", "critic"):
            for A in (1, 6, 32):
                for B in (1, 3, 129):
                    inference(lib, gen, kind, A, B, salted == "salted")
        conv4x4(lib, gen, salted == "salted")
        conv5x5(lib, gen, salted == "salted")
        head(lib, gen, salted == "salted")


if __name__ == "__main__":
    main()
