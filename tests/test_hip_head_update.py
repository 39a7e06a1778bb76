"""GPU checks of the native heads of the COMA update: csrc/head_train.hip behind ippm_head_forward, ippm_critic_loss, ippm_actor_loss and
ippm_head_backward, networks._HeadBf16 / _CriticLossBf16 / _ActorLossBf16, the learners' and the trainer's ``head_update="bf16"``.  The
reference of every numerical check is the CPU restatement of the contract (tests/head_train_ref.py), never the code under test; the dense
tolerances are ``MARGIN`` spreads between the float32 and the float64 restatement of the same case, the unit of the native forwards' tests."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import actor_native_ref as AR
import critic_native_ref as CR
import head_train_ref as R
from configs import make_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096                 # sentinel floats before and after every output
SENTINEL = -12345.678
PARTIAL_BYTES = 4 * (256 * 256 + 256 * 32 + 256 + 32)        # of one chunk's partial sums


def _lib():
    from ippmarl import _ffi
    return _ffi, _ffi.load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _scratch(B, A, fill=0xFF):
    _ffi, lib = _lib()
    nbytes = C.c_int64(0)
    _ffi.check(lib.ippm_head_scratch_bytes(B, A, C.addressof(nbytes)), "ippm_head_scratch_bytes")
    chunks = (B + R.CHUNK - 1) // R.CHUNK
    assert nbytes.value == (chunks + 1) // 2 * 16 + B * 256 * 4 + chunks * PARTIAL_BYTES
    return torch.full((nbytes.value,), fill, dtype=torch.uint8, device=DEV)      # (0xFF bytes: NaN as float32)


class _Guarded:
    """Outputs pre-filled with NaN between two bands of GUARD sentinels each."""

    def __init__(self, **shapes):
        self.shapes, self.whole, self.out = shapes, {}, {}
        for name, shape in shapes.items():
            n = int(np.prod(shape)) if shape else 1
            self.whole[name] = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
            self.out[name] = self.whole[name][GUARD:GUARD + n]
            self.out[name].fill_(float("nan"))

    def ptr(self, name):
        return self.out[name].data_ptr()

    def collect(self):
        torch.cuda.synchronize()
        for name, whole in self.whole.items():
            n = self.out[name].numel()
            assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all()), f"sentinels of {name} overwritten"
        return {name: self.out[name].cpu().view(self.shapes[name]) for name in self.shapes}

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(o).all()) for o in self.out.values())


def _dev(*tensors):
    return [t.to(DEV).contiguous() for t in tensors]


def _forward(h, w1, b1, w3, b3, scratch_fill=0xFF):
    _ffi, lib = _lib()
    B, A = h.shape[0], w3.shape[0]
    g = _Guarded(a1=(B, 256), logits=(B, A))
    h, w1, b1, w3, b3 = _dev(h, w1, b1, w3, b3)
    scratch = _scratch(B, A, scratch_fill)
    _ffi.check(lib.ippm_head_forward(h.data_ptr(), w1.data_ptr(), b1.data_ptr(), w3.data_ptr(), b3.data_ptr(), B, A, scratch.data_ptr(),
                                     g.ptr("a1"), g.ptr("logits"), _stream()), "ippm_head_forward")
    return g.collect()


def _backward(dlogits, scale, a1, h, w1, w3, scratch_fill=0xFF):
    """scale: None (NULL) or a float handed over as a device scalar"""
    _ffi, lib = _lib()
    B, A = dlogits.shape
    g = _Guarded(gh=(B, 256), gw1=(256, 256), gb1=(256,), gw3=(A, 256), gb3=(A,))
    dlogits, a1, h, w1, w3 = _dev(dlogits, a1, h, w1, w3)
    s = None if scale is None else torch.full((), float(scale), device=DEV)
    scratch = _scratch(B, A, scratch_fill)
    _ffi.check(lib.ippm_head_backward(dlogits.data_ptr(), None if s is None else s.data_ptr(), a1.data_ptr(), h.data_ptr(), w1.data_ptr(),
                                      w3.data_ptr(), B, A, scratch.data_ptr(), g.ptr("gh"), g.ptr("gw1"), g.ptr("gb1"), g.ptr("gw3"), g.ptr("gb3"),
                                      _stream()), "ippm_head_backward")
    return g.collect()


def _critic_loss(q, action, td, scratch_fill=0xFF):
    _ffi, lib = _lib()
    B, A = q.shape
    g = _Guarded(loss=(), q_chosen=(B,), dq=(B, A))
    q, action, td = _dev(q, action, td)
    scratch = _scratch(B, A, scratch_fill)
    _ffi.check(lib.ippm_critic_loss(q.data_ptr(), action.data_ptr(), td.data_ptr(), B, A, scratch.data_ptr(), g.ptr("loss"), g.ptr("q_chosen"),
                                    g.ptr("dq"), _stream()), "ippm_critic_loss")
    return g.collect()


def _actor_loss(logits, q, mask, action, eps, eps_on_device=False, scratch_fill=0xFF):
    _ffi, lib = _lib()
    B, A = logits.shape
    g = _Guarded(loss=(), adv=(B,), probs=(B, A), dlogits=(B, A))
    logits, q, mask, action = _dev(logits, q, mask, action)
    e = torch.full((), float(eps), device=DEV) if eps_on_device else None
    scratch = _scratch(B, A, scratch_fill)
    # (with a device scalar the float argument is a decoy: the non-NULL eps_dev wins)
    _ffi.check(lib.ippm_actor_loss(logits.data_ptr(), q.data_ptr(), mask.data_ptr(), action.data_ptr(), B, A, 0.9 if eps_on_device else float(eps),
                                   None if e is None else e.data_ptr(), scratch.data_ptr(), g.ptr("loss"), g.ptr("adv"), g.ptr("probs"),
                                   g.ptr("dlogits"), _stream()), "ippm_actor_loss")
    return g.collect()


# ---- 1. small integers: bit for bit against the float64 restatement -----------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 15, 16, 17, 127, 128, 129])
@pytest.mark.parametrize("A", R.ACTION_SETS)
def test_forward_small_integers_bit_for_bit(A, batch):
    a1, logits = R.int_forward(batch, A)
    assert float(logits.abs().max()) < 2 ** 24 and float(a1.max()) > 256
    got = _forward(R.int_h(batch), *R.int_weights(A))
    assert torch.equal(got["a1"].double(), a1), (A, batch, int((got["a1"].double() != a1).sum()))
    assert torch.equal(got["logits"].double(), logits), (A, batch, int((got["logits"].double() != logits).sum()))


@pytest.mark.parametrize("rel", ["1", "3", "chunk-1", "chunk", "chunk+1", "2chunk+3"])
@pytest.mark.parametrize("A", R.ACTION_SETS)
def test_backward_of_injected_integer_dlogits_bit_for_bit(A, rel):
    K = R.CHUNK
    B = {"1": 1, "3": 3, "chunk-1": K - 1, "chunk": K, "chunk+1": K + 1, "2chunk+3": 2 * K + 3}[rel]
    want = R.int_backward(B, A)
    w1, _, w3, _ = R.int_weights(A)
    got = _backward(R.int_dlogits(B, A), None, R.int_forward(B, A)[0].float(), R.int_h(B), w1, w3)
    for k, v in want.items():
        assert float(v.abs().max()) < 2 ** 24
        assert torch.equal(got[k].double(), v), (k, A, B, int((got[k].double() != v).sum()))


def test_backward_scales_dlogits_on_the_device():
    """scale_dev = 2: every output is that of the doubled dlogits, bit for bit (|gz1| <= 6 * 4 * 3 stays exact in bf16)."""
    A, B = 6, R.CHUNK + 1
    want = R.int_backward(B, A, 2.0)
    w1, _, w3, _ = R.int_weights(A)
    got = _backward(R.int_dlogits(B, A), 2.0, R.int_forward(B, A)[0].float(), R.int_h(B), w1, w3)
    for k, v in want.items():
        assert float(v.abs().max()) < 2 ** 24 and torch.equal(got[k].double(), v), k
    assert not torch.equal(want["gh"], R.int_backward(B, A)["gh"])


@pytest.mark.parametrize("batch", [16, 64])
@pytest.mark.parametrize("A", [4, 27])
def test_critic_loss_small_integers_bit_for_bit(A, batch):
    q, action, td = R.int_critic(batch, A)
    want = R.critic_loss(q, action, td, torch.float64)
    got = _critic_loss(q, action, td)
    for k, v in want.items():
        assert torch.equal(got[k].double(), v), (k, A, batch)
    assert float(want["loss"]) > 0 and int((want["dq"] != 0).sum()) > batch // 2


# ---- 2. dense real case -----------------------------------------------------------------------------------------------------------------
def _dense_stages(seed):
    """The chain head -> loss -> head backward on the device for both learners, and the restatement of every stage ON THE OPERANDS THE
    DEVICE STAGE WAS GIVEN: the losses and the backward on the device's logits, dlogits and a1, and, inside the forward, fc3 on the
    device's a1 (which is an output).  Why not one restated chain from h: a1 re-enters fc3 rounded to bf16, and one a1 whose float32 and
    float64 values straddle a bf16 rounding boundary moves a logit by |a1| 2^-9 |w3| -- 6e-4 here, 1600 times the float32 accumulation
    noise that the spread of a flip-free pair of restatements measures.  About two of the 76 800 a1 of a case do that under ANY float32
    summation order, the float32 restatement's own included (it showed the same 6e-4 on one CPU and none on another), so a chained
    comparison measures whether the two happen to flip the same element, not the kernels.  Stage by stage the reference is the same
    restatement, the unit the same spread, and the statement checked is tighter: the product takes bf16(a1) of the a1 that was returned.
    -> (device outputs, {output: (spread, float64 restatement)})"""
    i = R.dense_inputs(seed)
    got = _forward(i["h"], i["w1"], i["b1"], i["w3"], i["b3"])
    want = R.spreads(lambda t: {"a1": R.forward(i["h"], i["w1"], i["b1"], i["w3"], i["b3"], t)[0], "logits": R.fc3(got["a1"], i["w3"], i["b3"], t)})
    for kind in ("critic", "actor"):
        if kind == "critic":
            loss = _critic_loss(got["logits"], i["action"], i["td"])
            ref = R.spreads(lambda t: R.critic_loss(got["logits"], i["action"], i["td"], t))
        else:
            loss = _actor_loss(got["logits"], i["q_values"], i["mask"], i["action"], R.DENSE_EPS)
            ref = R.spreads(lambda t: R.actor_loss(got["logits"], i["q_values"], i["mask"], i["action"], R.DENSE_EPS, t))
        dl = loss["dq" if kind == "critic" else "dlogits"]
        back = _backward(dl, None, got["a1"], i["h"], i["w1"], i["w3"])
        ref.update(R.spreads(lambda t: R.backward(dl, 1.0, got["a1"].to(t), i["h"], i["w1"], i["w3"], t)))
        got.update({f"{kind}.{k}": v for k, v in {**loss, **back}.items()})
        want.update({f"{kind}.{k}": v for k, v in ref.items()})
    return got, want


@pytest.mark.parametrize("seed", R.DENSE_SEEDS)
def test_dense_case_within_four_spreads(seed):
    """Every output of the four entry points, for the critic's and the actor's chain, B = 300 (_dense_stages).  q_chosen is a copy of an
    input element: its restatements agree exactly, and so must the device.  Measured on MI355X (profiles/r13/test_figures.txt): the device
    sits between 0.26 and 2.56 spreads over the 18 other outputs and three seeds (a1 1.08 - 1.34, logits 1.38 - 2.56, the losses 0.39 -
    1.38, dq / dlogits 0.66 - 1.00, the ten gradients 0.26 - 1.88)."""
    assert R.dense_inputs(seed)["h"].shape[0] == 300
    got, spreads = _dense_stages(seed)
    assert set(got) == set(spreads) and len(got) == 2 + 2 * (4 + 5) - 1        # (the critic's loss has no probs)
    errs = {k: float((got[k].double() - spreads[k][1]).abs().max()) for k in got}
    for k in sorted(got):
        print(f"seed {seed} {k}: spread {spreads[k][0]:.3e}; device error {errs[k]:.3e} "
              f"({errs[k] / max(spreads[k][0], 1e-300):.2f} spreads); |ref| up to {float(spreads[k][1].abs().max()):.3e}")
    assert spreads.pop("critic.q_chosen")[0] == 0 and errs.pop("critic.q_chosen") == 0
    for k in spreads:
        assert spreads[k][0] > 0 and errs[k] <= R.MARGIN * spreads[k][0], (k, errs[k], spreads[k][0])


# ---- 3. the actor's loss ------------------------------------------------------------------------------------------------------------------
def _actor_case(A, seed=7, B=70):
    """Rows 0, 1: an all-zero mask; rows 2, 3: a single valid action (the chosen one); the rest 60 % valid with the chosen action valid."""
    g = torch.Generator().manual_seed(seed + A)
    logits, q = torch.randn(B, A, generator=g) * 2, torch.randn(B, A, generator=g)
    action = torch.randint(0, A, (B,), generator=g).int()
    mask = (torch.rand(B, A, generator=g) < 0.6).to(torch.uint8)
    mask[:4] = 0
    mask[2:].scatter_(1, action[2:].long().view(-1, 1), 1)
    return logits, q, mask, action


def _k7(probs, q, mask, action, A):
    from ippmarl import _ffi
    from ippmarl.derived import DerivedConstants
    d = DerivedConstants(make_params("small", experiment__constraints__num_actions=A))
    assert d.n_actions == A
    ctx = _ffi.Context(d)
    probs, q, mask, action = _dev(probs, q, mask, action)
    adv = torch.full((probs.shape[0],), float("nan"), device=DEV)
    ctx.call("ippm_coma_advantage", probs.data_ptr(), q.data_ptr(), mask.data_ptr(), action.data_ptr(), adv.data_ptr(), None, probs.shape[0], _stream())
    torch.cuda.synchronize()
    ctx.close()
    return adv.cpu()


@pytest.mark.parametrize("eps_on_device", [False, True])
@pytest.mark.parametrize("A", R.ACTION_SETS)
def test_actor_loss_cases(A, eps_on_device):
    """Every action set, epsilon from the float and from a device scalar, rows that exercise K7's floors; the returned adv is K7's on the
    returned probs, bit for bit."""
    eps = 0.3
    logits, q, mask, action = _actor_case(A)
    got = _actor_loss(logits, q, mask, action, eps, eps_on_device)
    r32, r64 = (R.actor_loss(logits, q, mask, action, eps, t) for t in (torch.float32, torch.float64))
    for k in r64:
        spread, err = float((r32[k].double() - r64[k]).abs().max()), float((got[k].double() - r64[k]).abs().max())
        print(f"A {A} {k}: spread {spread:.3e}; device error {err:.3e} ({err / spread:.2f} spreads)")
        assert spread > 0 and err <= R.MARGIN * spread, (k, err, spread)
    assert not bool(got["dlogits"][:4].any())                 # no valid action: weight 0; a single one: advantage 0
    assert torch.equal(got["adv"][2:4], torch.zeros(2)) and bool(got["dlogits"][4:].any())
    assert torch.equal(got["adv"], _k7(got["probs"], q, mask, action, A))


# ---- 4. independence and determinism --------------------------------------------------------------------------------------------------
def test_a_sample_does_not_depend_on_its_batch():
    """a1, logits, dlogits * B (both losses) and gh of a sample alone are the bits of the same sample in a batch -- of 256, a power of two,
    so that the division by the batch and the product with it are exact."""
    i = {k: (v[:256] if v.dim() and v.shape[0] == R.DENSE_BATCH else v) for k, v in R.dense_inputs(R.DENSE_SEEDS[0]).items()}
    B = i["h"].shape[0]
    assert B == 256
    f_all = _forward(i["h"], i["w1"], i["b1"], i["w3"], i["b3"])
    c_all = _critic_loss(f_all["logits"], i["action"], i["td"])
    a_all = _actor_loss(f_all["logits"], i["q_values"], i["mask"], i["action"], R.DENSE_EPS)
    gh_all = {"c": _backward(c_all["dq"], None, f_all["a1"], i["h"], i["w1"], i["w3"])["gh"],
              "a": _backward(a_all["dlogits"], None, f_all["a1"], i["h"], i["w1"], i["w3"])["gh"]}
    assert bool(a_all["dlogits"].any()) and bool(gh_all["a"].any())
    for n in (0, 63, 64, 255):                                # (the ends of the first row tile, the start of the second, the last row)
        one = slice(n, n + 1)
        f = _forward(i["h"][one], i["w1"], i["b1"], i["w3"], i["b3"])
        assert torch.equal(f["a1"][0], f_all["a1"][n]) and torch.equal(f["logits"][0], f_all["logits"][n]), n
        c = _critic_loss(f["logits"], i["action"][one], i["td"][one])
        a = _actor_loss(f["logits"], i["q_values"][one], i["mask"][one], i["action"][one], R.DENSE_EPS)
        assert torch.equal(c["q_chosen"][0], c_all["q_chosen"][n]) and torch.equal(a["adv"][0], a_all["adv"][n]), n
        assert torch.equal(c["dq"][0], c_all["dq"][n] * B) and torch.equal(a["dlogits"][0], a_all["dlogits"][n] * B), n
        # gh of the sample for the SAME dlogits row: alone and inside the batch
        for k, dl in (("c", c_all["dq"]), ("a", a_all["dlogits"])):
            alone = _backward(dl[one], None, f["a1"], i["h"][one], i["w1"], i["w3"])
            assert torch.equal(alone["gh"][0], gh_all[k][n]), (k, n)


def test_results_do_not_depend_on_the_scratch():
    """Twice the same bits for every output, on scratch pre-filled with NaN and with another pattern (0x7F7F7F7F: a large finite float)."""
    i = R.dense_inputs(R.DENSE_SEEDS[1])
    assert i["h"].shape[0] > 2 * R.CHUNK                      # several partial sums
    runs = []
    for fill in (0xFF, 0x7F):
        f = _forward(i["h"], i["w1"], i["b1"], i["w3"], i["b3"], fill)
        c = _critic_loss(f["logits"], i["action"], i["td"], fill)
        a = _actor_loss(f["logits"], i["q_values"], i["mask"], i["action"], R.DENSE_EPS, False, fill)
        b = _backward(a["dlogits"], None, f["a1"], i["h"], i["w1"], i["w3"], fill)
        runs.append({**f, **{"c." + k: v for k, v in c.items()}, **{"a." + k: v for k, v in a.items()}, **b})
    for k in runs[0]:
        assert not bool(torch.isnan(runs[0][k]).any()) and torch.equal(runs[0][k], runs[1][k]), k


# ---- 5. argument errors -------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    """Every error returns -1 with a message before anything is launched: the outputs keep their NaN fill and the sentinels stay."""
    _ffi, lib = _lib()
    B, A = 5, 6
    stream = _stream()
    w1, b1, w3, b3 = _dev(*R.int_weights(A))
    h, dl = _dev(R.int_h(B), R.int_dlogits(B, A))
    q, action, td = _dev(*R.int_critic(8, A))
    q, action, td = q[:B].contiguous(), action[:B].contiguous(), td[:B].contiguous()
    mask = torch.ones(B, A, dtype=torch.uint8, device=DEV)
    g = _Guarded(a1=(B, 256), logits=(B, A), loss=(), q_chosen=(B,), dq=(B, A), adv=(B,), probs=(B, A), dlogits=(B, A), gh=(B, 256),
                 gw1=(256, 256), gb1=(256,), gw3=(A, 256), gb3=(A,))
    a1 = torch.ones(B, 256, device=DEV)
    scratch = _scratch(B, A)
    nbytes = C.c_int64(0)

    def fails(rc, name, word):
        msg = lib.ippm_last_error().decode()
        assert rc == -1 and name in msg and word in msg, (rc, name, msg)

    name = "ippm_head_scratch_bytes"
    fails(lib.ippm_head_scratch_bytes(B, A, None), name, "null")
    for bad in (0, -1, (1 << 24) + 1):
        fails(lib.ippm_head_scratch_bytes(bad, A, C.addressof(nbytes)), name, "batch")
    for bad in (0, -1, 33):
        fails(lib.ippm_head_scratch_bytes(B, bad, C.addressof(nbytes)), name, "n_actions")
    s = scratch.data_ptr()
    # name -> (a good call, the slots that may not be null, the slots that must be 16-byte aligned, the batch's slot, n_actions' slot)
    calls = {
        "ippm_head_forward": ([h.data_ptr(), w1.data_ptr(), b1.data_ptr(), w3.data_ptr(), b3.data_ptr(), B, A, s, g.ptr("a1"), g.ptr("logits"), stream],
                              (0, 1, 2, 3, 4, 8, 9), (0, 1, 2, 3, 7, 8), 5, 6),
        "ippm_critic_loss": ([q.data_ptr(), action.data_ptr(), td.data_ptr(), B, A, s, g.ptr("loss"), g.ptr("q_chosen"), g.ptr("dq"), stream],
                             (0, 1, 2, 5, 6, 7, 8), (5,), 3, 4),
        "ippm_actor_loss": ([q.data_ptr(), q.data_ptr(), mask.data_ptr(), action.data_ptr(), B, A, 0.1, None, s, g.ptr("loss"), g.ptr("adv"),
                             g.ptr("probs"), g.ptr("dlogits"), stream], (0, 1, 2, 3, 8, 9, 10, 12), (8,), 4, 5),
        "ippm_head_backward": ([dl.data_ptr(), None, a1.data_ptr(), h.data_ptr(), w1.data_ptr(), w3.data_ptr(), B, A, s, g.ptr("gh"), g.ptr("gw1"),
                                g.ptr("gb1"), g.ptr("gw3"), g.ptr("gb3"), stream], (0, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13), (2, 3, 4, 5, 8, 9), 6, 7),
    }
    for name, (ok, pointers, aligned, i_batch, i_actions) in calls.items():
        fn = getattr(lib, name)

        def bad_call(slot, value):
            call = list(ok)
            call[slot] = value
            return fn(*call)

        for slot in pointers:
            fails(bad_call(slot, None), name, "null")
        for bad in (0, -1, (1 << 24) + 1):
            fails(bad_call(i_batch, bad), name, "batch")
        for bad in (0, -1, 33):
            fails(bad_call(i_actions, bad), name, "n_actions")
        for slot in aligned:
            fails(bad_call(slot, ok[slot] + 4), name, "16-byte aligned")
    assert g.untouched()                                      # nothing was launched
    g.collect()                                               # ... and the sentinels are intact
    assert lib.ippm_head_scratch_bytes(B, A, C.addressof(nbytes)) == 0 and nbytes.value > 0


# ---- 6. the seam ------------------------------------------------------------------------------------------------------------------------------
def _module(kind, seed, batch=64, exact_trunk=False):
    """A device network, its parameters as the restatement takes them, and inputs: the dense network on dense inputs, or (exact_trunk)
    the exact network's integer conv1 .. conv3 on its {0,1} inputs under the dense fc1 and fc3."""
    from ippmarl.networks import ActorNetwork, CriticNetwork
    net = (ActorNetwork if kind == "actor" else CriticNetwork)(make_params("small"))
    M = AR if kind == "actor" else CR
    ref = dict(M.dense_net(seed, net.n_actions))
    if exact_trunk:
        ref.update({n: M.exact_net(seed, net.n_actions)[n] for n in ("conv1", "conv2", "conv3")})
    with torch.no_grad():
        for name, (w, b) in ref.items():
            getattr(net, name).weight.copy_(w)
            getattr(net, name).bias.copy_(b)
    if exact_trunk:
        inputs = AR.exact_obs(seed, batch) if kind == "actor" else CR.exact_states(seed, batch)
    else:
        inputs = AR.dense_obs(seed, batch) if kind == "actor" else CR.dense_states(seed, batch)
    return net.to(DEV), ref, inputs


def _count(monkeypatch, function):
    calls = []
    real = function.apply
    monkeypatch.setattr(function, "apply", staticmethod(lambda *a: (calls.append(1), real(*a))[1]))
    return calls


def _head_functions():
    from ippmarl import networks
    return networks._HeadBf16, networks._CriticLossBf16, networks._ActorLossBf16


@pytest.mark.parametrize("trunk", ["float32", "bf16"])
@pytest.mark.parametrize("kind", ["critic", "actor"])
def test_learner_gradients_against_the_restated_network(kind, trunk, monkeypatch):
    """After a learner's ``backward`` under head_update="bf16": the .grad of every used parameter, the loss and q_chosen / adv against a CPU
    float64 network whose head and loss are the restatement -- with the float32 trunk (plain convolutions) and with trunk_update="bf16"
    (trunk_train_ref's restated convolutions).

    The two cases differ in what keeps the spread a unit.  The head rounds h and a1 to bf16; where the value one side rounds and the
    float64 reference's straddle a rounding boundary, the operand moves by 2^-9 of itself, thousands of times the float32 summation noise
    that a pair of restatements without such an element measures.  Under the bf16 trunk every evaluation -- the float32 restatement's as
    the device's -- has dozens of them among the 10^6 rounded activations and gradients of 64 dense samples, and the spread contains
    them.  Under the float32 trunk only the head rounds (16 384 elements at 64 samples: a few such elements or none, by the luck of each
    side's summation order -- measured: the same kernels at 0.00 spreads for the actor and at 2914 for the critic, whose pair of CPU
    restatements happened to have none), so that case is built to have none on either side: the exact network's integer convolutions on
    {0,1} inputs give every side the same h, exactly, and 8 samples leave 2048 a1 to round.  Measured on MI355X: 0.38 - 1.38 spreads
    under the bf16 trunk, 0.52 - 2.28 under the float32 one (fc1's weight gradient of the critic case is exact on every side: spread 0)."""
    from ippmarl.learners import ActorLearner, CriticLearner
    seed, eps = 5, 0.2
    B = 64 if trunk == "bf16" else 8
    net, ref, inputs = _module(kind, seed, B, exact_trunk=trunk == "float32")
    if trunk == "float32":
        h = inputs.permute(0, 3, 1, 2)
        for name in ("conv1", "conv2", "conv3"):
            h = torch.relu(torch.nn.functional.conv2d(h, *ref[name]))
        assert torch.equal(h, h.round()) and 0 < float(h.max()) <= 256 and float((h > 0).float().mean()) > 0.1      # integers, bf16-exact, alive
    A = net.n_actions
    g = torch.Generator().manual_seed(seed)
    action = torch.randint(0, A, (B,), generator=g).int()
    if kind == "critic":
        spec = ("critic", action, torch.randn(B, generator=g))
    else:
        mask = (torch.rand(B, A, generator=g) < 0.7).to(torch.uint8)
        mask.scatter_(1, action.long().view(-1, 1), 1)
        spec = ("actor", torch.randn(B, A, generator=g), mask, action, eps)
    want32, want64 = (R.net_grads(ref, inputs, spec, t, trunk == "bf16") for t in (torch.float32, torch.float64))
    counts = [_count(monkeypatch, f) for f in _head_functions()]
    if kind == "critic":
        learner = CriticLearner(make_params("small"), net, torch.device(DEV), head_update="bf16", trunk_update=trunk)
        loss = learner.backward(inputs.to(DEV), action.to(DEV), spec[2].to(DEV))
        side = learner._pending[4].view(-1)
    else:
        learner = ActorLearner(make_params("small"), net, torch.device(DEV), head_update="bf16", trunk_update=trunk)
        loss, side = learner.backward(inputs.to(DEV), action.to(DEV), mask.to(DEV), spec[1].to(DEV), eps)
    torch.cuda.synchronize()
    assert [len(c) for c in counts] == ([1, 1, 0] if kind == "critic" else [1, 0, 1])
    assert net.fc2.weight.grad is None or not bool(net.fc2.weight.grad.any())
    got = {"loss": loss.cpu().double(), "side": side.cpu().double()}
    got.update({name: getattr(getattr(net, name.split(".")[0]), name.split(".")[1]).grad.cpu().double() for name in want64[2]})
    r32 = {"loss": want32[0].double(), "side": want32[1].double(), **{k: v.double() for k, v in want32[2].items()}}
    r64 = {"loss": want64[0], "side": want64[1], **want64[2]}
    figures = {k: (float((got[k] - r64[k]).abs().max()), float((r32[k] - r64[k]).abs().max())) for k in r64}
    for k, (err, spread) in figures.items():
        print(f"{kind} trunk {trunk} {k}: spread {spread:.3e}; device error {err:.3e} ({err / max(spread, 1e-300):.2f} spreads); "
              f"|ref| up to {float(r64[k].abs().max()):.3e}")
    for k, (err, spread) in figures.items():        # (a spread of 0 -- sums that are exact in float32 -- asks for the exact result)
        assert err <= R.MARGIN * spread, (k, err, spread)
    assert sum(spread > 0 for _, spread in figures.values()) >= len(figures) - 2


def _params64(**kw):
    """2 UAVs on a 64 x 64 grid, as the native forwards' trainer tests."""
    return make_params("small", experiment__missions__n_agents=2, sensor__field_of_view__angle_x=99.0, sensor__field_of_view__angle_y=99.0, **kw)


def _trainer(seed=5, n_envs=3, params=None, **kw):
    from ippmarl.trainer import COMATrainer
    torch.manual_seed(seed)
    return COMATrainer(params or _params64(), n_envs=n_envs, first_episode=3, **kw)


ALL_ENV = ("IPPMARL_HEAD_UPDATE", "IPPMARL_TRUNK_UPDATE", "IPPMARL_CONV2_UPDATE")


def test_call_counts_and_trainer_modes(monkeypatch):
    """With the switch on each new Function runs exactly once per learner ``backward`` and never in a rollout, the TD targets, the post-step
    Q or a diagnostics minibatch (collect=True); a default-mode trainer built afterwards in the same process never runs them."""
    for v in ALL_ENV:
        monkeypatch.delenv(v, raising=False)
    head, closs, aloss = (_count(monkeypatch, f) for f in _head_functions())
    tr = _trainer(head_update="bf16")
    assert tr.head_update == tr.critic_learner.head_update == tr.actor_learner.head_update == "bf16"
    assert tr.trunk_update == tr.conv2_update == "float32"             # independent of the other switches
    assert tr.rollout("train")["faults"] == 0 and not head            # the no-grad forwards of the rollout keep the float32 path
    n = tr.T * tr.E * tr.N
    td, _ = tr.td_targets()
    assert not head and not closs and not aloss
    states, obs = tr.buf_state[:1].reshape(n, 11, 11, 12), tr.buf_obs[:1].reshape(n, 11, 11, 7)
    actions, masks = tr.buf_action[:1].reshape(n), tr.buf_mask[:1].reshape(n, tr.A)
    tr.critic_learner.backward(states, actions, td)
    assert (len(head), len(closs), len(aloss)) == (1, 1, 0)
    q = tr.critic_learner.apply()                                      # (the post-step Q: a no-grad forward)
    assert (len(head), len(closs), len(aloss)) == (1, 1, 0)
    tr.actor_learner.backward(obs, actions, masks, q, tr.eps)
    assert (len(head), len(closs), len(aloss)) == (2, 1, 1)
    tr.actor_learner.apply()
    tr.critic_learner.collect = tr.actor_learner.collect = True       # diagnostics take the PyTorch head for that minibatch
    tr.critic_learner.backward(states, actions, td)
    q = tr.critic_learner.apply()
    tr.actor_learner.backward(obs, actions, masks, q, tr.eps)
    tr.actor_learner.apply()
    assert tr.critic_learner.last is not None and tr.actor_learner.last is not None
    tr.critic_learner.collect = tr.actor_learner.collect = False
    assert (len(head), len(closs), len(aloss)) == (2, 1, 1)
    tr.update()
    steps = tr.data_passes * tr.batch_number
    assert (len(head), len(closs), len(aloss)) == (2 + 2 * steps, 1 + steps, 1 + steps)
    plain = _trainer(seed=6)
    assert plain.head_update == plain.critic_learner.head_update == plain.actor_learner.head_update == "float32"
    assert plain.rollout("train")["faults"] == 0
    stats = plain.update()
    assert np.isfinite(stats["critic_loss"]) and (len(head), len(closs), len(aloss)) == (2 + 2 * steps, 1 + steps, 1 + steps)
    tr.rollout("train")
    tr.update()                                                        # ... and the first trainer has kept its own mode
    assert (len(head), len(closs), len(aloss)) == (2 + 4 * steps, 1 + 2 * steps, 1 + 2 * steps)


# ---- 7. the trainer ---------------------------------------------------------------------------------------------------------------------------
def test_trainer_round_at_the_smallest_env_count(monkeypatch):
    from ippmarl import networks
    for v in ALL_ENV:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv(networks.HEAD_UPDATE_ENV, "bf16")              # the environment variable is how bench.py gets the switch
    tr = _trainer(seed=8, n_envs=1)
    assert tr.head_update == "bf16" and tr.T * tr.E * tr.N // tr.batch_number >= 1
    before = {net: torch.cat([p.detach().reshape(-1).clone() for p in getattr(tr, net).parameters()]) for net in ("actor", "critic")}
    assert tr.rollout("train")["faults"] == 0
    stats = tr.update()
    assert np.isfinite(stats["critic_loss"]) and np.isfinite(stats["actor_loss"])
    for net in ("actor", "critic"):
        module = getattr(tr, net)
        after = torch.cat([p.detach().reshape(-1) for p in module.parameters()])
        assert bool(torch.isfinite(after).all()) and float((after - before[net]).abs().max()) > 0, net
        for layer in (module.conv1, module.conv3, module.fc1, module.fc3):
            for p in layer.parameters():
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any())
        for p in module.fc2.parameters():
            assert p.grad is None or not bool(p.grad.any()), net
    assert int(tr.env.fault.ne(0).sum()) == 0


# ---- 8. graphs ------------------------------------------------------------------------------------------------------------------------------------
def _flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()])


def _copy_training_state(src, dst):
    with torch.no_grad():
        for net in ("actor", "critic"):
            for p_dst, p_src in zip(getattr(dst, net).parameters(), getattr(src, net).parameters()):
                p_dst.copy_(p_src)
        for learner in ("actor_learner", "critic_learner"):
            src_opt, dst_opt = getattr(src, learner).optimizer, getattr(dst, learner).optimizer
            for g_src, g_dst in zip(src_opt.param_groups, dst_opt.param_groups):
                for p_src, p_dst in zip(g_src["params"], g_dst["params"]):
                    for k, v in src_opt.state.get(p_src, {}).items():
                        dst_opt.state[p_dst][k].copy_(v)
        for p_dst, p_src in zip(dst.critic_learner.target_critic.parameters(), src.critic_learner.target_critic.parameters()):
            p_dst.copy_(p_src)


def _run_recorded_rounds():
    """One round of a trainer replayed from hipGraphs beside the same round run launch by launch twice (the premise: two eager rounds
    agree), all three with head_update="bf16" and from identical training state
    -> {net: flat parameters of (eager, eager again, recorded)}, and the parameters before the round."""
    saved = {v: os.environ.pop(v, None) for v in ALL_ENV}
    try:
        eager, again, rec = (_trainer(seed=11, graphs=True, head_update="bf16") for _ in range(3))
        for tr in (eager, again, rec):       # first round launch by launch (kernel selection, allocator)
            torch.manual_seed(12)
            tr.rollout("train")
            tr.update()
        _copy_training_state(eager, again)
        _copy_training_state(eager, rec)
        rec.capture_graphs()
        before = {net: _flat(getattr(eager, net)).clone() for net in ("critic", "actor")}
        for tr in (eager, again, rec):
            torch.manual_seed(20)
            assert tr.rollout("train")["faults"] == 0
            stats = tr.update()
            assert np.isfinite(stats["critic_loss"]) and np.isfinite(stats["actor_loss"])
        assert rec._update_graph is not None and again._update_graph is None
        return {net: tuple(_flat(getattr(tr, net)).clone() for tr in (eager, again, rec)) for net in ("critic", "actor")}, before
    finally:
        for v, value in saved.items():
            if value is not None:
                os.environ[v] = value


def test_recorded_round_equals_eager_round(tmp_path):
    """tests/head_recorded_rounds.py in a process of its own (the convolution library in deterministic mode): two eager rounds agree, and
    after a recorded round both nets' parameters are the eager round's bit for bit, finite, and moved."""
    out = tmp_path / "digests.json"
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "head_recorded_rounds.py")
    env = {k: v for k, v in os.environ.items() if k not in ALL_ENV}
    run = subprocess.run([sys.executable, script, str(out)], env=env, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]        # (nothing further is started after a failure)
    with open(out) as f:
        nets = json.load(f)
    assert set(nets) == {"critic", "actor"}
    for net, n in nets.items():
        print(f"{net}: {n['differ']} of {n['numel']} parameters differ eager - recorded (max {n['max']:.3e}), {n['premise_differ']} eager - eager; "
              f"the round moved them by up to {n['moved']:.3e}")
    for net, n in nets.items():
        assert n["finite"] and n["moved"] > 0, (net, n)
        assert n["digests"][0] == n["digests"][1] and n["premise_differ"] == 0, (net, n)      # the premise: two eager rounds agree
        assert n["digests"][0] == n["digests"][2] and n["differ"] == 0, (net, n)
