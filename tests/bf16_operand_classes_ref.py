"""Shared by test_bf16_operand_classes_cpu.py and test_hip_bf16_operand_classes.py: operands that NEED rounding in an interesting way, and
operands that are not finite, for every bf16 matrix-core entry point (the native actor and critic forwards, conv4x4_train.hip,
conv5x5_train.hip, head_train.hip).  Nothing here calls the code under test; every expected value is the restatement of the entry
point's module (conv2_train_ref, trunk_train_ref, head_train_ref, actor_native_ref / critic_native_ref) under ``restate``.

Contract: float32 -> bf16 is round to nearest even, NaN stays NaN, a magnitude from 0x7F7F8000 on gives Inf; NaN and
Inf then propagate as in the IEEE arithmetic of the definition (Inf * 0 = NaN, Inf - Inf = NaN, relu(NaN) = NaN); padding contributes nothing.

Part A, rounding classes.  One operand of an entry point is filled with a cycled list of float32 bit patterns (``PATTERNS``); every other
operand is a SELECTOR, a 0/1 tensor that picks at most one product per output sum, so that an output is bf16(one pattern) -- or, for
the operands the contract does not round (biases, the returned a1, gb3), the pattern itself -- and every accumulation order gives the
same bits.  Every case comes with two lists: the ``-finite`` one (no pattern rounds to Inf: every output is finite and is compared bit
for bit) and the ``-all`` one (with the patterns that round to Inf: they meet the selector's zeros and give NaN, compared by class).
Float32 SUBNORMALS are left out on purpose: whether the matrix cores flush them is a hardware property nobody here has measured.

Part B, one poisoned element.  A dense case is run clean and with one element replaced by NaN, +Inf or -Inf (``POISONS``); ``depends``
writes out, from the definition, which output elements that element reaches: everything else must keep the clean run's bits, and the
class (finite, +Inf, -Inf, NaN) of every output element is the restatement's."""
import collections
import functools

import numpy as np
import torch

import actor_native_ref as AR
import conv2_train_ref as C2
import critic_native_ref as CR
import head_train_ref as HR
import trunk_train_ref as TR

CH = 256
PLANES = {"actor": 7, "critic": 12}
TILE_ROWS = 128               # LT_M of ippm_bf16_net.h: rows of a workgroup tile of the layer kernel, conv4x4's and conv5x5's forward
HEAD_TILE = HR.CHUNK          # head_train.hip: HT_M == IPPM_HEAD_WGRAD_CHUNK (a static_assert there)


def _header(name):
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ippmarl.h")
    with open(path) as f:
        return int(re.search(rf"^#define {name} (\d+)$", f.read(), re.M).group(1))


C4_CHUNK, C5_CHUNK = _header("IPPM_CONV4X4_WGRAD_CHUNK"), TR.CHUNK

# ---- the patterns -------------------------------------------------------------------------------------------------------------------------
NAMED = {                      # float32 bits -> the bf16 bits round-to-nearest-even gives (test_bf16_operand_classes_cpu.py checks torch's too)
    0x00000000: 0x0000,        # 0.0
    0x3F800000: 0x3F80,        # 1.0: exact
    0x40490000: 0x4049,        # 3.140625: exact
    0x3F808000: 0x3F80,        # a tie whose even neighbour is below
    0x3F818000: 0x3F82,        # a tie whose even neighbour is above
    0x3F807FFF: 0x3F80,        # one ulp below a tie
    0x3F808001: 0x3F81,        # one ulp above a tie
    0x3FFF8000: 0x4000,        # a tie that carries into the exponent
    0x7F7F7FFF: 0x7F7F,        # the largest float32 that still rounds to the largest bf16
    0x00800000: 0x0080,        # the smallest normal
    0x00FF8000: 0x0100,        # a tie between the two smallest exponents
    0x7E967699: 0x7E96,        # 1e38: a large one, rounded down
    0x3DCCCCCD: 0x3DCD,        # 0.1f: rounded up
    0x7F7F8000: 0x7F80,        # the smallest that rounds to Inf
    0x7F7FFFFF: 0x7F80,        # FLT_MAX
    0x3E000000: 0x3E00,        # 0.125: exact (makes the signed lists odd)
}
_FINITE = tuple(NAMED)[:13]
_OVERFLOW = (0x7F7F8000, 0x7F7FFFFF)


def _signed(bits):
    return bits + tuple(b | 0x80000000 for b in bits) + (0x3E000000,)


# the lengths are odd and share no factor with the 2-wide (packed hardware conversion) and 8-wide (one 16-byte LDS store) groups, so
# cycling a list over a tensor's flat index puts every pattern into every slot of both
PATTERNS = {"nonneg-finite": _FINITE, "nonneg-all": _FINITE + _OVERFLOW, "signed-finite": _signed(_FINITE), "signed-all": _signed(_FINITE + _OVERFLOW)}
LISTS = ("finite", "all")


def pattern_values(which):
    return torch.from_numpy(np.array(PATTERNS[which], dtype=np.uint32).view(np.float32).copy())


def cycled(shape, which, start=0):
    p = pattern_values(which)
    n = int(np.prod(shape))
    return p[(torch.arange(n) + start) % len(p)].view(shape).clone()


# ---- comparing ----------------------------------------------------------------------------------------------------------------------------
FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3
BY_CLASS_ONLY = ("probs",)    # softmax: expf, not a rounding of the operands -- its finite values are the dense tests' business


def classes(t):
    c = torch.zeros(t.shape, dtype=torch.int8)
    c[t == float("inf")] = POS_INF
    c[t == float("-inf")] = NEG_INF
    c[torch.isnan(t)] = NAN
    return c


def disagreements(got, want, exact=True):
    """Elements of the float32 ``got`` whose class is not that of ``want`` cast to float32, plus (``exact``) the finite ones whose value
    differs: bit for bit, +0 and -0 counting as equal."""
    want = want.to(torch.float32)
    cg, cw = classes(got), classes(want)
    bad = cg != cw
    if exact:
        bad |= (cw == FINITE) & (cg == FINITE) & (got != want)
    return int(bad.sum())


def same_bits(a, b):
    return a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)


# ---- the restatements, by entry point -------------------------------------------------------------------------------------------------
def restate(entry, a, dtype):
    """entry, its arguments {name: tensor} -> {output: tensor in ``dtype``}"""
    if entry == "conv4x4.y":
        return {"y": C2.forward(a["x"], a["w"], dtype)}
    if entry == "conv4x4.gx":
        return {"gx": C2.grad_input(a["gy"], a["w"], dtype)}
    if entry == "conv4x4.gw":
        return {"gw": C2.grad_weight(a["gy"], a["x"], dtype)}
    if entry == "conv5x5.y":
        return {"y": TR.forward(a["x"], a["w"], a.get("bias"), dtype)}
    if entry == "conv5x5.gw":
        return {"gw": TR.grad_weight(a["gy"], a["x"], dtype)}
    if entry == "head.forward":
        a1, logits = HR.forward(a["h"], a["w1"], a["b1"], a["w3"], a["b3"], dtype)
        return {"a1": a1, "logits": logits}
    if entry == "head.backward":
        return HR.backward(a["dlogits"], a["scale"], a["a1"].to(dtype), a["h"], a["w1"], a["w3"], dtype)
    if entry == "critic_loss":
        return HR.critic_loss(a["q"], a["action"], a["td"], dtype)
    if entry == "actor_loss":
        return HR.actor_loss(a["logits"], a["q_values"], a["mask"], a["action"], a["eps"], dtype)
    if entry == "actor":
        logits = AR.emulate(a["net"], a["x"], dtype)
        return {"logits": logits, "probs": AR.mix(logits, 0.0)}
    if entry == "critic":
        return {"q": CR.emulate(a["net"], a["x"], dtype)}
    raise KeyError(entry)


def get(args, path):
    """path: "x", or "conv2.weight" / "fc3.bias" of args["net"]"""
    if "." in path:
        layer, what = path.split(".")
        return args["net"][layer][what == "bias"]
    return args[path]


def replaced(args, path, value):
    out = dict(args)
    if "." in path:
        layer, what = path.split(".")
        pair = list(args["net"][layer])
        pair[what == "bias"] = value
        out["net"] = dict(args["net"])
        out["net"][layer] = tuple(pair)
    else:
        out[path] = value
    return out


# ---- Part A: selectors ------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "entry args operand support")    # support: where the patterned operand is filled (None: everywhere)


def _tap_identity(out_ch, in_ch, k, tap_of):
    """w[o,c,ty,tx] = [c == o % in_ch][(ty, tx) == tap_of(o)] (None: tap (0, 0))"""
    w = torch.zeros(out_ch, in_ch, k, k)
    o = torch.arange(out_ch)
    tap = torch.zeros(out_ch, dtype=torch.long) if tap_of is None else tap_of(o)
    w[o, o % in_ch, tap // k, tap % k] = 1
    return w


def _one_per_channel(B, H, W, C, step=1009):
    """t[b,y,x,c] = [(b,y,x) == site(c)]: channel C-1 sits in the last pixel of the last sample, the others ``step`` positions apart"""
    P = B * H * W
    t = torch.zeros(P, C)
    c = torch.arange(C)
    t[(P - 1 - (C - 1 - c) * step) % P, c] = 1
    return t.view(B, H, W, C)


def _one_per_sample(B, H, W, C, sites=None):
    """t[b] is one-hot at sites[b] = (y, x, c) (default: seeded by b, both parities of c)"""
    t = torch.zeros(B, H, W, C)
    for b in range(B):
        y, x, c = sites[b] if sites else ((b * 3 + 1) % H, (b * 5 + 2) % W, (b * 37 + 6) % C)
        t[b, y, x, c] = 1
    return t


def _rows_one_hot(B, width=CH):
    """h[m,k] = [k == (37 m + 5) % width]"""
    h = torch.zeros(B, width)
    m = torch.arange(B)
    h[m, (m * 37 + 5) % width] = 1
    return h


def _conv4x4_case(entry, operand, shape, tap, which):
    B, ih, iw = shape
    oh, ow = ih - 3, iw - 3
    eye = _tap_identity(CH, CH, 4, lambda o: torch.full_like(o, tap[0] * 4 + tap[1]))
    if entry == "conv4x4.y":
        args = dict(x=cycled((B, ih, iw, CH), which), w=eye) if operand == "x" else dict(x=_one_per_sample(B, ih, iw, CH), w=cycled(C2.W_SHAPE, which))
    elif entry == "conv4x4.gx":
        args = dict(gy=cycled((B, oh, ow, CH), which), w=eye) if operand == "gy" else dict(gy=_one_per_sample(B, oh, ow, CH), w=cycled(C2.W_SHAPE, which))
    elif operand == "gy":
        args = dict(gy=cycled((B, oh, ow, CH), which), x=_one_per_channel(B, ih, iw, CH))
    else:
        args = dict(gy=_one_per_channel(B, oh, ow, CH), x=cycled((B, ih, iw, CH), which))
    return Case(entry, args, operand, None)


def _conv5x5_case(entry, operand, planes, which):
    if entry == "conv5x5.y":
        B = 3
        if operand == "x":       # output channel o reads plane o % planes at tap (24 - o // planes) % 25: every tap, the last real k included
            args = dict(x=cycled((B, 11, 11, planes), which), w=_tap_identity(CH, planes, 5, lambda o: (24 - o // planes) % 25))
        elif operand == "w":     # (5, 5): every tap meets an output position; plane planes-1 at tap 24 is the last real k
            args = dict(x=_one_per_sample(B, 11, 11, planes, [(5, 5, planes - 1), (4, 6, 0), (6, 4, planes // 2)]), w=cycled(TR.w_shape(planes), which))
        else:                    # x = 0: y = relu(bias), not rounded
            args = dict(x=torch.zeros(B, 11, 11, planes), w=TR.int_w(planes), bias=cycled((CH,), which))
    else:
        B = C5_CHUNK + 1
        if operand == "gy":
            args = dict(gy=cycled((B, 7, 7, CH), which), x=_one_per_channel(B, 11, 11, planes, step=617))
        else:
            args = dict(gy=_one_per_channel(B, 7, 7, CH), x=cycled((B, 11, 11, planes), which))
    return Case(entry, args, operand, None)


def _fc3_selector(A):
    w3 = torch.zeros(A, CH)
    w3[torch.arange(A), torch.arange(A)] = 1
    return w3


def _head_forward_case(operand, B, A, which):
    args = dict(h=_rows_one_hot(B), w1=torch.eye(CH), b1=torch.zeros(CH), w3=_fc3_selector(A), b3=torch.zeros(A))
    if operand == "b1":          # a1 on its way into fc3: a1 = relu(b1) is returned unrounded, logits = bf16(a1)
        args.update(h=torch.zeros(B, CH), b1=cycled((CH,), which))
    else:
        args[operand] = cycled(tuple(args[operand].shape), which)
    return Case("head.forward", args, operand, None)


def _head_backward_case(operand, B, A, which, start=0):
    """d = dlogits * scale is one-hot per action a at row r_a (row B-1 for a = 0) and fc3 sends action a to unit n_a, so gz1 has one
    non-zero per used row and column and every sum over the batch has one term."""
    assert B > A
    a = torch.arange(A)
    r, n = (B - 1 - 7 * a) % B, (9 * a + 2) % CH
    assert len(set(r.tolist())) == A
    d = torch.zeros(B, A)
    d[r, a] = 1
    w3 = torch.zeros(A, CH)
    w3[a, n] = 1
    args = dict(dlogits=d, scale=1.0, a1=torch.ones(B, CH), h=_rows_one_hot(B), w1=torch.eye(CH), w3=w3)
    support = None
    if operand == "dlogits":     # scaled on the device, then rounded: dlogits = pattern / 2 (exact), scale = 2; gb3 gets d unrounded.
        p = torch.zeros(B, A)    # (only A elements are non-zero, so the list is cycled over them, from ``start`` on)
        p[r, a] = cycled((A,), which, start)
        args.update(dlogits=torch.where(p.abs() >= 2.0 ** -125, p * 0.5, p), scale=2.0)
        support = d
    elif operand == "w3":        # row a < A carries action a, and the ReLU's mask opens unit n for row n % A only
        d = torch.zeros(B, A)
        d[a, a] = 1
        a1 = torch.zeros(B, CH)
        a1[torch.arange(CH) % A, torch.arange(CH)] = 1
        args.update(dlogits=d, a1=a1, w3=cycled((A, CH), which))
    else:
        args[operand] = cycled(tuple(args[operand].shape), which)
    return Case("head.backward", args, operand, support)


NET_BATCH = 17


def selector_net(planes, A):
    """identity at tap (0,0) through conv1 to conv3, identity fc1, fc3[a,n] = [a == n]; no bias"""
    zero = torch.zeros(CH)
    return {"conv1": (_tap_identity(CH, planes, 5, None) * (torch.arange(CH) < planes).view(-1, 1, 1, 1), zero),
            "conv2": (_tap_identity(CH, CH, 4, None), zero), "conv3": (_tap_identity(CH, CH, 4, None), zero),
            "fc1": (torch.eye(CH), zero), "fc3": (_fc3_selector(A), torch.zeros(A))}


def _net_case(kind, operand, A, which):
    """The batch of NET_BATCH; batch 1 is its first sample.  A patterned weight is met by a one-hot sample whose 1 sits at the tap the
    sample reads of it (sample 0: the last real k of conv1, plane planes-1 at tap 24)."""
    planes, B = PLANES[kind], NET_BATCH
    layer = operand.split(".")[0]
    side = {"conv1": 5, "conv2": 4, "conv3": 4}.get(layer, 1)
    sites = [(side - 1 - b % side, side - 1 - (b // side) % side, (planes - 1 - b) % planes) for b in range(B)]
    args = dict(net=selector_net(planes, A), x=_one_per_sample(B, 11, 11, planes, sites), A=A)
    if operand == "x":
        args["x"] = cycled((B, 11, 11, planes), which)
    elif operand == "fc3.bias":
        args = replaced(dict(args, x=torch.zeros(B, 11, 11, planes)), operand, cycled((A,), which))
    else:
        args = replaced(args, operand, cycled(tuple(get(args, operand).shape), which))
    return Case(kind, args, operand, None)


def _rounding_cases():
    cases = {}
    for lst in LISTS:
        for shape in ((2, 5, 6), (1, 4, 4)):       # (the second is the conv3 use)
            s = "x".join(map(str, shape))
            for entry, operands in (("conv4x4.y", ("x", "w")), ("conv4x4.gx", ("gy", "w")), ("conv4x4.gw", ("gy", "x"))):
                for operand in operands:
                    for tap in ((0, 0), (3, 3)) if operand != "w" and entry != "conv4x4.gw" else ((0, 0),):
                        cases[f"{entry}/{operand}/{s}/tap{tap[0]}{tap[1]}/{lst}"] = functools.partial(_conv4x4_case, entry, operand, shape, tap, f"signed-{lst}")
        for planes in TR.PLANES:
            for operand in ("x", "w", "bias"):
                cases[f"conv5x5.y/{operand}/planes{planes}/{lst}"] = functools.partial(_conv5x5_case, "conv5x5.y", operand, planes, f"signed-{lst}")
            for operand in ("gy", "x"):
                cases[f"conv5x5.gw/{operand}/planes{planes}/{lst}"] = functools.partial(_conv5x5_case, "conv5x5.gw", operand, planes, f"signed-{lst}")
        for B, A in ((17, 4), (129, 27)):
            for operand in ("h", "w1", "w3", "b1"):
                cases[f"head.forward/{operand}/B{B}-A{A}/{lst}"] = functools.partial(_head_forward_case, operand, B, A, f"signed-{lst}")
        for B, A in ((17, 4), (HR.CHUNK + 1, 27)):
            for operand in ("a1", "h", "w1", "w3"):
                cases[f"head.backward/{operand}/B{B}-A{A}/{lst}"] = functools.partial(_head_backward_case, operand, B, A, f"signed-{lst}")
            for start in range(0, len(PATTERNS[f"signed-{lst}"]), A):
                cases[f"head.backward/dlogits/B{B}-A{A}/from{start}/{lst}"] = functools.partial(_head_backward_case, "dlogits", B, A, f"signed-{lst}", start)
        for kind in PLANES:
            for A in (4, 27):
                for operand in ("x", "conv1.weight", "conv2.weight", "conv3.weight", "fc1.weight", "fc3.weight", "fc3.bias"):
                    sign = "signed" if operand.startswith("fc3") else "nonneg"      # (non-negative in front of a ReLU)
                    cases[f"{kind}/{operand}/A{A}/{lst}"] = functools.partial(_net_case, kind, operand, A, f"{sign}-{lst}")
    return cases


ROUNDING_CASES = _rounding_cases()


@functools.lru_cache(maxsize=None)
def rounding_case(case_id):
    return ROUNDING_CASES[case_id]()


@functools.lru_cache(maxsize=None)
def rounding_expected(case_id, dtype=torch.float64):
    case = rounding_case(case_id)
    return restate(case.entry, case.args, dtype)


def selected_counts(case):
    """How many products each output sum picks: the restatement with the patterned operand replaced by ones on its support."""
    t = get(case.args, case.operand)
    ones = torch.ones_like(t) if case.support is None else case.support.clone()
    args = replaced(case.args, case.operand, ones)
    if case.operand == "dlogits":
        args["scale"] = 1.0
    return restate(case.entry, args, torch.float64)


# ---- Part B: one poisoned element ------------------------------------------------------------------------------------------------------
POISONS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
POISON_SEED = 1
LOSS_EPS = HR.DENSE_EPS


@functools.lru_cache(maxsize=None)
def poison_base(base):
    """The dense inputs of the existing tests at the small batches of the poison cases -> (entry, args)."""
    kind, _, rest = base.partition("@")
    if kind.startswith("conv4x4"):
        B, ih, iw = map(int, rest.split("x"))
        x, w, gy = C2.dense_inputs(POISON_SEED, B, ih, iw)
        return kind, {"conv4x4.y": dict(x=x, w=w), "conv4x4.gx": dict(gy=gy, w=w), "conv4x4.gw": dict(gy=gy, x=x)}[kind]
    if kind.startswith("conv5x5"):
        planes, B = map(int, rest.split("x"))
        x, w, bias, gy = TR.dense_inputs(POISON_SEED, planes, B)
        return kind, dict(x=x, w=w, bias=bias) if kind == "conv5x5.y" else dict(gy=gy, x=x)
    if kind in ("head.forward", "head.backward", "critic_loss", "actor_loss"):
        B, A = map(int, rest.split("x"))
        i = HR.dense_inputs(POISON_SEED, A, B)
        fwd = dict(h=i["h"], w1=i["w1"], b1=i["b1"], w3=i["w3"], b3=i["b3"])
        if kind == "head.forward":
            return kind, fwd
        a1, logits = (t.float() for t in HR.forward(*fwd.values(), torch.float32))
        if kind == "critic_loss":
            return kind, dict(q=logits, action=i["action"], td=i["td"])
        if kind == "actor_loss":
            return kind, dict(logits=logits, q_values=i["q_values"], mask=i["mask"], action=i["action"], eps=LOSS_EPS)
        dq = HR.critic_loss(logits, i["action"], i["td"], torch.float32)["dq"]
        dense = torch.randn(B, A, generator=torch.Generator().manual_seed(POISON_SEED)) / B      # (dq alone has one non-zero per row)
        return kind, dict(dlogits=dq + dense, scale=1.0, a1=a1, h=i["h"], w1=i["w1"], w3=i["w3"])
    A = int(rest)
    R, obs = (AR, AR.dense_obs) if kind == "actor" else (CR, CR.dense_states)
    return kind, dict(net=R.dense_net(POISON_SEED, A), x=obs(POISON_SEED, NET_BATCH), A=A)


def _window(lo, hi, n):
    return slice(max(lo, 0), min(hi, n))


def depends(entry, args, operand, idx):
    """{output: bool mask of the elements the definition connects to element ``idx`` of ``operand``}.  Written out from the formulas in
    the restatement modules' docstrings; the CPU test checks that nothing outside a mask moves in the restatement."""
    out = {k: torch.zeros(v.shape, dtype=torch.bool) for k, v in restate_shapes(entry, args).items()}
    if entry in ("conv4x4.y", "conv5x5.y"):
        k = 4 if entry == "conv4x4.y" else 5
        y = out["y"]
        if operand == "x":       # x[b,y,x,c] -> y[b, y-k+1 .. y, x-k+1 .. x, :], clipped to the output
            b, py, px, _ = idx
            y[b, _window(py - k + 1, py + 1, y.shape[1]), _window(px - k + 1, px + 1, y.shape[2]), :] = True
        else:                    # w[o,c,ty,tx], bias[o] -> channel o of every sample
            y[..., idx[0]] = True
    elif entry == "conv4x4.gx":
        gx = out["gx"]
        oh, ow = args["gy"].shape[1:3]
        if operand == "gy":      # gy[b,oy,ox,o] -> gx[b, oy .. oy+3, ox .. ox+3, :]
            b, oy, ox, _ = idx
            gx[b, oy:oy + 4, ox:ox + 4, :] = True
        else:                    # w[o,c,ty,tx] -> channel c at the input positions (oy + ty, ox + tx)
            _, c, ty, tx = idx
            gx[:, ty:ty + oh, tx:tx + ow, c] = True
    elif entry in ("conv4x4.gw", "conv5x5.gw"):
        gw = out["gw"]
        k = gw.shape[-1]
        oh, ow = args["gy"].shape[1:3]
        if operand == "gy":      # gy[b,oy,ox,o] -> gw[o,:,:,:]
            gw[idx[3]] = True
        else:                    # x[b,y,x,c] -> gw[:, c, ty, tx] for the taps with (y - ty, x - tx) inside the output
            _, py, px, c = idx
            for ty in range(k):
                for tx in range(k):
                    if 0 <= py - ty < oh and 0 <= px - tx < ow:
                        gw[:, c, ty, tx] = True
    elif entry == "head.forward":
        if operand == "h":       # h[m,k] -> row m
            out["a1"][idx[0]] = True
            out["logits"][idx[0]] = True
        elif operand in ("w1", "b1"):    # unit n of every row, and through fc3 every logit
            out["a1"][:, idx[0]] = True
            out["logits"][:] = True
        else:                    # w3[a,n], b3[a] -> action a of every row
            out["logits"][:, idx[0]] = True
    elif entry == "head.backward":
        if operand == "dlogits":         # d[m,a] -> gz1[m,:] -> gh[m,:], every gw1 and gb1; gw3[a,:], gb3[a]
            m, a = idx
            out["gh"][m] = True
            out["gw1"][:] = True
            out["gb1"][:] = True
            out["gw3"][a] = True
            out["gb3"][a] = True
        elif operand == "a1":            # a1[m,n] -> gw3[:,n]; its sign is the mask of gz1[m,n] -> gh[m,:], gw1[n,:], gb1[n]
            m, n = idx
            out["gw3"][:, n] = True
            out["gh"][m] = True
            out["gw1"][n] = True
            out["gb1"][n] = True
        elif operand == "h":             # h[m,k] -> gw1[:,k]
            out["gw1"][:, idx[1]] = True
        elif operand == "w1":            # w1[o,k] -> gh[:,k]
            out["gh"][:, idx[1]] = True
        else:                            # w3[a,n] -> gz1[:,n] -> every gh, gw1[n,:], gb1[n]
            n = idx[1]
            out["gh"][:] = True
            out["gw1"][n] = True
            out["gb1"][n] = True
    elif entry == "critic_loss":         # q[r, action[r]] -> loss, q_chosen[r], dq[r,:]; td[r] -> loss, dq[r,:]
        r = idx[0]
        out["loss"][...] = True
        out["dq"][r] = True
        if operand == "q":
            assert int(args["action"][r]) == idx[1]
            out["q_chosen"][r] = True
    elif entry == "actor_loss":          # logits[r,:] -> row r of everything; q_values[r,:] -> adv[r], dlogits[r,:] (not probs)
        r = idx[0]
        out["loss"][...] = True
        out["adv"][r] = True
        out["dlogits"][r] = True
        if operand == "logits":
            out["probs"][r] = True
    else:                                # the networks: a sample reaches its own row; fc3's row a its column (through the softmax: every
        for name, t in out.items():      # probability of every row); any other parameter everything
            if operand == "x":
                t[idx[0]] = True
            elif operand.startswith("fc3") and name != "probs":
                t[:, idx[0]] = True
            else:
                t[:] = True
    return out


def restate_shapes(entry, args):
    """{output: a tensor of the output's shape} without running the restatement"""
    def z(*shape):
        return torch.empty(shape)
    if entry == "conv4x4.y":
        B, ih, iw, _ = args["x"].shape
        return {"y": z(B, ih - 3, iw - 3, CH)}
    if entry == "conv4x4.gx":
        B, oh, ow, _ = args["gy"].shape
        return {"gx": z(B, oh + 3, ow + 3, CH)}
    if entry == "conv4x4.gw":
        return {"gw": z(*C2.W_SHAPE)}
    if entry == "conv5x5.y":
        return {"y": z(args["x"].shape[0], 7, 7, CH)}
    if entry == "conv5x5.gw":
        return {"gw": z(*TR.w_shape(args["x"].shape[-1]))}
    if entry == "head.forward":
        return {"a1": z(args["h"].shape[0], CH), "logits": z(args["h"].shape[0], args["w3"].shape[0])}
    if entry == "head.backward":
        B, A = args["dlogits"].shape
        return {"gh": z(B, CH), "gw1": z(CH, CH), "gb1": z(CH), "gw3": z(A, CH), "gb3": z(A)}
    if entry == "critic_loss":
        B, A = args["q"].shape
        return {"loss": z(), "q_chosen": z(B), "dq": z(B, A)}
    if entry == "actor_loss":
        B, A = args["logits"].shape
        return {"loss": z(), "adv": z(B), "probs": z(B, A), "dlogits": z(B, A)}
    B, A = args["x"].shape[0], args["A"]
    return {"logits": z(B, A), "probs": z(B, A)} if entry == "actor" else {"q": z(B, A)}


def _poison_sites():
    """{id: (base, operand, index)}: the first and the last element, a corner pixel (one output position or one tap), the last real k of
    conv1 (plane planes-1 at tap 24), action A-1 of 27 (next to the five padded ones), the last sample of batch tile + 1 and CHUNK + 1,
    a sample in the middle of the networks' batch of 17 and its last one."""
    sites = {}

    def add(base, operand, idx, note):
        sites[f"{base}/{operand}/{note}"] = (base, operand, tuple(idx))

    t4, c4 = TILE_ROWS + 1, C4_CHUNK + 1
    add(f"conv4x4.y@{t4}x4x4", "x", (0, 0, 0, 0), "first")
    add(f"conv4x4.y@{t4}x4x4", "x", (t4 - 1, 3, 3, 255), "last-of-tile+1")
    add("conv4x4.y@2x5x6", "x", (1, 4, 5, 3), "corner-pixel")
    add("conv4x4.y@2x5x6", "w", (0, 0, 0, 0), "first")
    add("conv4x4.y@2x5x6", "w", (255, 255, 3, 3), "last")
    add(f"conv4x4.gx@{t4}x4x4", "gy", (0, 0, 0, 0), "first")
    add(f"conv4x4.gx@{t4}x4x4", "gy", (t4 - 1, 0, 0, 255), "last-of-tile+1")
    add("conv4x4.gx@2x5x6", "gy", (1, 1, 2, 5), "corner-pixel")
    add("conv4x4.gx@2x5x6", "w", (0, 0, 0, 0), "first")
    add("conv4x4.gx@2x5x6", "w", (255, 255, 3, 3), "last-tap")          # (a tap that is invalid at most input positions)
    add(f"conv4x4.gw@{c4}x4x4", "gy", (0, 0, 0, 0), "first")
    add(f"conv4x4.gw@{c4}x4x4", "gy", (c4 - 1, 0, 0, 255), "last-of-chunk+1")
    add(f"conv4x4.gw@{c4}x4x4", "x", (c4 - 1, 3, 3, 255), "last-of-chunk+1")
    add("conv4x4.gw@2x5x6", "x", (0, 0, 0, 0), "corner-pixel")            # (one tap only)
    add("conv4x4.gw@2x5x6", "gy", (1, 1, 2, 128), "last-pixel")
    c5 = C5_CHUNK + 1
    for planes in TR.PLANES:
        add(f"conv5x5.y@{planes}x3", "x", (0, 0, 0, 0), "first")
        add(f"conv5x5.y@{planes}x3", "x", (2, 10, 10, planes - 1), "last-corner")    # (one output position, through the last real k)
        add(f"conv5x5.y@{planes}x3", "w", (0, 0, 0, 0), "first")
        add(f"conv5x5.y@{planes}x3", "w", (255, planes - 1, 4, 4), "last-real-k")
        add(f"conv5x5.y@{planes}x3", "bias", (255,), "last")
        add(f"conv5x5.gw@{planes}x{c5}", "gy", (0, 0, 0, 0), "first")
        add(f"conv5x5.gw@{planes}x{c5}", "gy", (c5 - 1, 6, 6, 255), "last-of-chunk+1")
        add(f"conv5x5.gw@{planes}x{c5}", "x", (c5 - 1, 10, 10, planes - 1), "last-of-chunk+1")   # (tap 24 only: the last real k)
        add(f"conv5x5.gw@{planes}x{c5}", "x", (0, 0, 0, 0), "first")
    B, A = HEAD_TILE + 1, 27
    hb = f"@{B}x{A}"
    for operand, idx, note in (("h", (0, 0), "first"), ("h", (B - 1, 255), "last-of-tile+1"), ("w1", (255, 255), "last"), ("b1", (0,), "first"),
                               ("w3", (A - 1, 255), "last-action"), ("b3", (A - 1,), "last-action")):
        add("head.forward" + hb, operand, idx, note)
    for operand, idx, note in (("dlogits", (0, 0), "first"), ("dlogits", (B - 1, A - 1), "last-of-chunk+1"), ("a1", (B - 1, 255), "last-of-chunk+1"),
                               ("h", (B - 1, 255), "last-of-chunk+1"), ("w1", (255, 255), "last"), ("w3", (A - 1, 255), "last-action")):
        add("head.backward" + hb, operand, idx, note)
    action = HR.dense_inputs(POISON_SEED, A, B)["action"]
    for r in (0, B - 1):
        add("critic_loss" + hb, "q", (r, int(action[r])), f"row{r}")
        add("critic_loss" + hb, "td", (r,), f"row{r}")
        add("actor_loss" + hb, "logits", (r, int(action[r])), f"row{r}")
        add("actor_loss" + hb, "q_values", (r, int(action[r])), f"row{r}")
    add("actor_loss" + hb, "logits", (B - 1, A - 1), "last")
    for kind, planes in PLANES.items():
        add(f"{kind}@27", "x", (NET_BATCH // 2, 0, 0, 0), "middle-sample")
        add(f"{kind}@27", "x", (NET_BATCH - 1, 4, 4, planes - 1), "last-sample")
        add(f"{kind}@27", "conv1.weight", (255, planes - 1, 4, 4), "last-real-k")
        add(f"{kind}@27", "conv2.weight", (0, 0, 0, 0), "first")
        add(f"{kind}@27", "conv3.weight", (255, 255, 3, 3), "last")
        add(f"{kind}@27", "fc1.weight", (0, 0), "first")
        add(f"{kind}@27", "fc1.bias", (255,), "last")
        add(f"{kind}@27", "fc3.weight", (26, 255), "last-action")
        add(f"{kind}@27", "fc3.bias", (26,), "last-action")
    return sites


POISON_SITES = _poison_sites()
POISON_CASES = [f"{site}/{p}" for site in POISON_SITES for p in POISONS]


def poison_case(case_id):
    """-> (entry, clean args, poisoned args, operand, index)"""
    site, _, p = case_id.rpartition("/")
    base, operand, idx = POISON_SITES[site]
    entry, args = poison_base(base)
    t = get(args, operand).clone()
    t[idx] = POISONS[p]
    return entry, args, replaced(args, operand, t), operand, idx


@functools.lru_cache(maxsize=None)
def poison_clean_expected(base):
    entry, args = poison_base(base)
    return restate(entry, args, torch.float64)


def poison_expected(case_id):
    """The float64 restatement of the poisoned case.  A poisoned network input is restated for its own sample only (the restatement's
    samples do not meet) and spliced into the clean batch."""
    entry, args, bad, operand, idx = poison_case(case_id)
    if entry in ("actor", "critic") and operand == "x":
        b = idx[0]
        one = restate(entry, dict(bad, x=bad["x"][b:b + 1]), torch.float64)
        out = {k: v.clone() for k, v in poison_clean_expected(case_id.split("/")[0]).items()}
        for k in out:
            out[k][b] = one[k][0]
        return out
    return restate(entry, bad, torch.float64)
