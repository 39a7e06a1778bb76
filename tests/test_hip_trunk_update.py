"""GPU checks of the bf16 matrix-core conv1 and conv3 of the COMA update: csrc/conv5x5_train.hip behind ippm_conv5x5_bf16_forward /
_grad_weight, networks._Conv5x5Bf16 and _Conv3Bf16, the learners' and the trainer's ``trunk_update="bf16"``.  The reference of every
numerical check is the CPU restatement of the contract (tests/trunk_train_ref.py), never the code under test; the dense tolerances are
``MARGIN`` spreads between the float32 and the float64 restatement of the same case, the unit of the native forwards' tests."""
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
import trunk_train_ref as R
from configs import make_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096                 # sentinel floats before and after every output
SENTINEL = -12345.678
PADDED_K = {7: 192, 12: 320}


def _lib():
    from ippmarl import _ffi
    return _ffi, _ffi.load_library()


def _chunk():
    return _lib()[0].CONV5X5_WGRAD_CHUNK


def _scratch(B, planes, fill=0xFF):
    _ffi, lib = _lib()
    nbytes = C.c_int64(0)
    _ffi.check(lib.ippm_conv5x5_bf16_scratch_bytes(B, planes, C.addressof(nbytes)), "ippm_conv5x5_bf16_scratch_bytes")
    chunks = (B + _chunk() - 1) // _chunk()
    assert nbytes.value == 256 * PADDED_K[planes] * (2 + 4 * chunks)      # one bf16 pack, one float32 partial per chunk
    return torch.full((nbytes.value,), fill, dtype=torch.uint8, device=DEV)      # (0xFF bytes: NaN as bf16 and as float32)


def _guarded(shape):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    out = whole[GUARD:GUARD + n]
    out.fill_(float("nan"))
    return whole, out, n


def _intact(whole, n):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all())


def _forward(x, w, bias, scratch_fill=0xFF):
    """ippm_conv5x5_bf16_forward on an output pre-filled with NaN between two bands of GUARD sentinels, and a pre-filled scratch
    -> y on the CPU; asserts rc == 0 and intact sentinels."""
    _ffi, lib = _lib()
    B, planes = x.shape[0], x.shape[-1]
    whole, out, n = _guarded((B, 7, 7, R.OUT))
    x, w = x.to(DEV).contiguous(), w.to(DEV).contiguous()
    b = None if bias is None else bias.to(DEV).contiguous()
    scratch = _scratch(B, planes, scratch_fill)
    _ffi.check(lib.ippm_conv5x5_bf16_forward(x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), B, planes, scratch.data_ptr(),
                                             out.data_ptr(), torch.cuda.current_stream().cuda_stream), "ippm_conv5x5_bf16_forward")
    torch.cuda.synchronize()
    assert _intact(whole, n), "sentinels overwritten"
    return out.cpu().view(B, 7, 7, R.OUT)


def _grad_weight(gy, x, scratch_fill=0xFF):
    _ffi, lib = _lib()
    B, planes = x.shape[0], x.shape[-1]
    whole, out, n = _guarded(R.w_shape(planes))
    gy, x = gy.to(DEV).contiguous(), x.to(DEV).contiguous()
    scratch = _scratch(B, planes, scratch_fill)
    _ffi.check(lib.ippm_conv5x5_bf16_grad_weight(gy.data_ptr(), x.data_ptr(), B, planes, scratch.data_ptr(), out.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "ippm_conv5x5_bf16_grad_weight")
    torch.cuda.synchronize()
    assert _intact(whole, n), "sentinels overwritten"
    return out.cpu().view(R.w_shape(planes))


# ---- 1. small integers: bit for bit against the float64 restatement -----------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("batch", [1, 2, 3, 6])          # 49, 98 rows (under one tile), 147 (one + a partial one), 294 (two + a partial one)
@pytest.mark.parametrize("planes", R.PLANES)
def test_forward_small_integers_bit_for_bit(planes, batch, with_bias):
    want = R.int_forward(batch, planes, with_bias)
    got = _forward(R.int_x(batch, planes), R.int_w(planes), R.int_bias() if with_bias else None)
    assert float(want.abs().max()) < 2 ** 24
    bad = int((got.double() != want).sum())
    assert bad == 0, (planes, batch, with_bias, bad, want.numel())


@pytest.mark.parametrize("rel", ["1", "3", "chunk-1", "chunk", "chunk+1", "2chunk+3"])
@pytest.mark.parametrize("planes", R.PLANES)
def test_weight_gradient_small_integers_bit_for_bit(planes, rel):
    K = _chunk()
    B = {"1": 1, "3": 3, "chunk-1": K - 1, "chunk": K, "chunk+1": K + 1, "2chunk+3": 2 * K + 3}[rel]
    want = R.int_grad_weight(B, planes)
    assert float(want.abs().max()) < 2 ** 24
    got = _grad_weight(R.int_gy(B), R.int_x(B, planes))
    assert torch.equal(got.double(), want), (planes, B, int((got.double() != want).sum()))


# ---- 2. dense real case -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.DENSE_SEEDS)
@pytest.mark.parametrize("planes", R.PLANES)
def test_dense_case_within_four_spreads(planes, seed):
    x, w, bias, gy = R.dense_inputs(seed, planes)
    assert x.shape[0] == 300
    got = {"y": _forward(x, w, None), "yb": _forward(x, w, bias), "gw": _grad_weight(gy, x)}
    spreads = R.dense_spreads(seed, planes)
    errs = {op: float((got[op].double() - spreads[op][1]).abs().max()) for op in got}
    for op in got:
        print(f"planes {planes} seed {seed} {op}: spread {spreads[op][0]:.3e}; device error {errs[op]:.3e} "
              f"({errs[op] / spreads[op][0]:.2f} spreads); |ref| up to {float(spreads[op][1].abs().max()):.3e}")
    for op in got:
        assert spreads[op][0] > 0 and errs[op] <= R.MARGIN * spreads[op][0], (op, errs[op], spreads[op][0])


def test_fused_store_equals_the_separate_bias_relu_pass():
    """bias non-null gives the float32 bits of ippm_bias_relu_nhwc run on the bias-free output."""
    _ffi, lib = _lib()
    x, w, bias, _ = R.dense_inputs(R.DENSE_SEEDS[0], 12)
    fused = _forward(x, w, bias)
    plain = _forward(x, w, None).to(DEV)
    b = bias.to(DEV)
    _ffi.check(lib.ippm_bias_relu_nhwc(plain.data_ptr(), b.data_ptr(), plain.numel() // 256, 256, torch.cuda.current_stream().cuda_stream),
               "ippm_bias_relu_nhwc")
    torch.cuda.synchronize()
    assert torch.equal(plain.cpu(), fused) and float((fused == 0).float().mean()) > 0.05


# ---- 3. independence and determinism --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", R.PLANES)
def test_a_sample_does_not_depend_on_its_batch(planes):
    x, w, bias, _ = R.dense_inputs(R.DENSE_SEEDS[0], planes)
    got = _forward(x, w, bias)
    for i in (0, 2, 3, 299):                              # (rows of sample 2 straddle the first tile's end)
        assert torch.equal(_forward(x[i:i + 1], w, bias)[0], got[i]), i


@pytest.mark.parametrize("planes", R.PLANES)
def test_weight_gradient_is_deterministic_and_ignores_prior_content(planes):
    """Twice the same bits, on scratch and outputs pre-filled with NaN and with another pattern: nothing is read before it is written,
    the padded K columns included."""
    x, _, _, gy = R.dense_inputs(R.DENSE_SEEDS[0], planes)
    assert x.shape[0] > _chunk()                          # more than one partial sum
    first = _grad_weight(gy, x, scratch_fill=0xFF)
    second = _grad_weight(gy, x, scratch_fill=0x7F)       # (0x7F7F7F7F: another pattern, a large finite float)
    assert not torch.isnan(first).any()
    assert torch.equal(first, second)


# ---- 4. guard bands (every call above asserts them; these are the shapes whose rows end inside a tile) -----------------------------
@pytest.mark.parametrize("planes", R.PLANES)
def test_guard_bands_stay_intact(planes):
    B = 3
    y = _forward(R.int_x(B, planes), R.int_w(planes), R.int_bias())
    gw = _grad_weight(R.int_gy(B), R.int_x(B, planes))
    assert not torch.isnan(y).any() and not torch.isnan(gw).any()          # and every element was written


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    _ffi, lib = _lib()
    B, planes = 3, 7
    stream = torch.cuda.current_stream().cuda_stream
    x, w, bias, gy = R.int_x(B, planes).to(DEV), R.int_w(planes).to(DEV), R.int_bias().to(DEV), R.int_gy(B).to(DEV)
    y = torch.full((B, 7, 7, R.OUT), float("nan"), device=DEV)
    gw = torch.full(R.w_shape(planes), float("nan"), device=DEV)
    scratch = _scratch(B, planes)
    nbytes = C.c_int64(0)

    def fails(rc, name, word):
        msg = lib.ippm_last_error().decode()
        assert rc == -1 and name in msg and word in msg, (rc, name, msg)

    name = "ippm_conv5x5_bf16_scratch_bytes"
    fails(lib.ippm_conv5x5_bf16_scratch_bytes(B, planes, None), name, "null")
    for bad in (0, -1, (1 << 24) + 1):
        fails(lib.ippm_conv5x5_bf16_scratch_bytes(bad, planes, C.addressof(nbytes)), name, "batch")
    for bad in (0, 6, 8, 13, 256):
        fails(lib.ippm_conv5x5_bf16_scratch_bytes(B, bad, C.addressof(nbytes)), name, "planes")
    # (slots: the pointers that may not be null, the batch, the planes, the scratch)
    calls = {"ippm_conv5x5_bf16_forward": ([x.data_ptr(), w.data_ptr(), bias.data_ptr(), B, planes, scratch.data_ptr(), y.data_ptr(), stream],
                                           (0, 1, 5, 6), 3, 4, 5),
             "ippm_conv5x5_bf16_grad_weight": ([gy.data_ptr(), x.data_ptr(), B, planes, scratch.data_ptr(), gw.data_ptr(), stream],
                                               (0, 1, 4, 5), 2, 3, 4)}
    for name, (ok, pointers, i_batch, i_planes, i_scratch) in calls.items():
        fn = getattr(lib, name)

        def bad_call(slot, value):
            call = list(ok)
            call[slot] = value
            return fn(*call)

        for slot in pointers:
            fails(bad_call(slot, None), name, "null")
        for bad in (0, -1, (1 << 24) + 1):
            fails(bad_call(i_batch, bad), name, "batch")
        for bad in (0, 6, 8, 13):
            fails(bad_call(i_planes, bad), name, "planes")
        fails(bad_call(i_scratch, scratch.data_ptr() + 8), name, "16-byte aligned")
        for slot in pointers:
            if slot != i_scratch:
                fails(bad_call(slot, ok[slot] + 4), name, "16-byte aligned")
    fails(lib.ippm_conv5x5_bf16_forward(x.data_ptr(), w.data_ptr(), bias.data_ptr() + 4, B, planes, scratch.data_ptr(), y.data_ptr(), stream),
          "ippm_conv5x5_bf16_forward", "16-byte aligned")
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(gw).all())         # nothing was launched
    assert lib.ippm_conv5x5_bf16_scratch_bytes(B, planes, C.addressof(nbytes)) == 0 and nbytes.value > 0


# ---- 6. the seam ------------------------------------------------------------------------------------------------------------------------------
def _module(kind, seed):
    from ippmarl.networks import ActorNetwork, CriticNetwork
    net = (ActorNetwork if kind == "actor" else CriticNetwork)(make_params("small"))
    ref = (AR if kind == "actor" else CR).dense_net(seed, net.n_actions)
    with torch.no_grad():
        for name, (w, b) in ref.items():
            getattr(net, name).weight.copy_(w)
            getattr(net, name).bias.copy_(b)
    inputs = AR.dense_obs(seed, 64) if kind == "actor" else CR.dense_states(seed, 64)
    return net.to(DEV), ref, inputs


def _count(monkeypatch, function):
    calls = []
    real = function.apply
    monkeypatch.setattr(function, "apply", staticmethod(lambda *a: (calls.append(1), real(*a))[1]))
    return calls


@pytest.mark.parametrize("kind", ["critic", "actor"])
def test_device_gradients_against_the_restated_network(kind, monkeypatch):
    """The .grad of every used parameter of a device network run under trunk_update("bf16") against a CPU float64 network whose conv1,
    conv2 and conv3 are the restatement.  The loss is a mean squared error of fc3's output against seeded targets (so that every gradient,
    fc3's bias included, carries the network's rounding and not only a sum's)."""
    from ippmarl import networks
    seed, B = 5, 64
    net, ref, inputs = _module(kind, seed)
    target = torch.randn(B, net.n_actions, generator=torch.Generator().manual_seed(seed))

    def loss_fn(out):
        return (out - target.to(out.device, out.dtype)).square().mean()

    g32, g64 = R.net_grads(ref, inputs, loss_fn, torch.float32), R.net_grads(ref, inputs, loss_fn, torch.float64)
    counts = {f.__name__: _count(monkeypatch, f) for f in (networks._Conv5x5Bf16, networks._Conv4x4Bf16, networks._Conv3Bf16)}
    with networks.trunk_update("bf16"):
        out, _ = net.trunk(inputs.to(DEV))
    loss_fn(out).backward()
    torch.cuda.synchronize()
    assert {k: len(v) for k, v in counts.items()} == {"_Conv5x5Bf16": 1, "_Conv4x4Bf16": 1, "_Conv3Bf16": 1}
    assert net.fc2.weight.grad is None and net.fc2.bias.grad is None
    figures = {}
    for name in g64:
        layer, what = name.split(".")
        got = getattr(getattr(net, layer), what).grad.cpu().double()
        figures[name] = (float((got - g64[name]).abs().max()), float((g32[name].double() - g64[name]).abs().max()))
        print(f"{kind} {name}: spread {figures[name][1]:.3e}; device error {figures[name][0]:.3e} "
              f"({figures[name][0] / figures[name][1]:.2f} spreads); |grad| up to {float(g64[name].abs().max()):.3e}")
    for name, (err, spread) in figures.items():
        assert spread > 0 and err <= R.MARGIN * spread, (name, err, spread)


def _params64(**kw):
    """2 UAVs on a 64 x 64 grid, as the native forwards' trainer tests."""
    return make_params("small", experiment__missions__n_agents=2, sensor__field_of_view__angle_x=99.0, sensor__field_of_view__angle_y=99.0, **kw)


def _trainer(seed=5, n_envs=3, params=None, **kw):
    from ippmarl.trainer import COMATrainer
    torch.manual_seed(seed)
    return COMATrainer(params or _params64(), n_envs=n_envs, first_episode=3, **kw)


def test_call_counts_and_trainer_modes(monkeypatch):
    """In bf16 mode each of the two new Functions runs exactly once per learner ``backward`` and never in a no-grad forward; a default-mode
    trainer built afterwards in the same process never runs them (the mode is the learner's, not the process's), even with the bf16
    trainer still alive; a conv2_update="bf16" trainer runs neither."""
    from ippmarl import networks
    monkeypatch.delenv(networks.TRUNK_UPDATE_ENV, raising=False)
    monkeypatch.delenv(networks.CONV2_UPDATE_ENV, raising=False)
    calls, calls3, calls2 = (_count(monkeypatch, f) for f in (networks._Conv5x5Bf16, networks._Conv3Bf16, networks._Conv4x4Bf16))
    tr = _trainer(trunk_update="bf16")
    assert tr.trunk_update == tr.critic_learner.trunk_update == tr.actor_learner.trunk_update == "bf16"
    assert tr.conv2_update == tr.critic_learner.conv2_update == "float32"          # implied for conv2, not rewritten
    assert tr.rollout("train")["faults"] == 0 and not calls           # the no-grad forwards of the rollout keep the float32 path
    n = tr.T * tr.E * tr.N
    td, _ = tr.td_targets()
    assert not calls
    states, obs = tr.buf_state[:1].reshape(n, 11, 11, 12), tr.buf_obs[:1].reshape(n, 11, 11, 7)
    actions, masks = tr.buf_action[:1].reshape(n), tr.buf_mask[:1].reshape(n, tr.A)
    tr.critic_learner.backward(states, actions, td)
    assert len(calls) == 1
    q = tr.critic_learner.apply()                                      # (the post-step Q: a no-grad forward)
    assert len(calls) == 1
    tr.actor_learner.backward(obs, actions, masks, q, tr.eps)
    assert len(calls) == 2
    tr.actor_learner.apply()
    tr.update()
    steps = 2 * tr.data_passes * tr.batch_number
    assert len(calls) == len(calls3) == len(calls2) == 2 + steps
    plain = _trainer(seed=6)
    assert plain.trunk_update == plain.critic_learner.trunk_update == plain.actor_learner.trunk_update == "float32"
    assert plain.rollout("train")["faults"] == 0
    stats = plain.update()
    assert np.isfinite(stats["critic_loss"]) and len(calls) == len(calls2) == 2 + steps
    conv2 = _trainer(seed=7, conv2_update="bf16")
    assert conv2.trunk_update == "float32" and conv2.rollout("train")["faults"] == 0
    conv2.update()
    assert len(calls) == len(calls3) == 2 + steps and len(calls2) == 2 + 2 * steps
    tr.rollout("train")
    tr.update()                                                        # ... and the first trainer has kept its own mode
    assert len(calls) == len(calls3) == 2 + 2 * steps


# ---- 7. the trainer ---------------------------------------------------------------------------------------------------------------------------
def test_trainer_round_at_the_smallest_env_count(monkeypatch):
    from ippmarl import networks
    monkeypatch.delenv(networks.CONV2_UPDATE_ENV, raising=False)
    monkeypatch.setenv(networks.TRUNK_UPDATE_ENV, "bf16")             # the environment variable is how bench.py gets the switch
    tr = _trainer(seed=8, n_envs=1)
    assert tr.trunk_update == "bf16" and tr.T * tr.E * tr.N // tr.batch_number >= 1
    before = {net: torch.cat([p.detach().reshape(-1).clone() for p in getattr(tr, net).parameters()]) for net in ("actor", "critic")}
    assert tr.rollout("train")["faults"] == 0
    stats = tr.update()
    assert np.isfinite(stats["critic_loss"]) and np.isfinite(stats["actor_loss"])
    for net in ("actor", "critic"):
        module = getattr(tr, net)
        after = torch.cat([p.detach().reshape(-1) for p in module.parameters()])
        assert bool(torch.isfinite(after).all()) and float((after - before[net]).abs().max()) > 0, net
        for conv in (module.conv1, module.conv2, module.conv3):
            assert conv.weight.grad is not None and bool(torch.isfinite(conv.weight.grad).all()) and bool(conv.weight.grad.any())
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
    agree), all three with trunk_update="bf16" and from identical training state
    -> {net: flat parameters of (eager, eager again, recorded)}, and the parameters before the round."""
    from ippmarl import networks
    saved = {v: os.environ.pop(v, None) for v in (networks.TRUNK_UPDATE_ENV, networks.CONV2_UPDATE_ENV)}
    try:
        eager, again, rec = (_trainer(seed=11, graphs=True, trunk_update="bf16") for _ in range(3))
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


def test_recorded_bf16_round_equals_eager_round(tmp_path):
    """tests/trunk_recorded_rounds.py in a process of its own (the convolution library in deterministic mode for whatever it still runs):
    two eager rounds agree, and after a recorded round both nets' parameters are the eager round's bit for bit, finite, and moved."""
    out = tmp_path / "digests.json"
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "trunk_recorded_rounds.py")
    env = {k: v for k, v in os.environ.items() if k not in ("IPPMARL_TRUNK_UPDATE", "IPPMARL_CONV2_UPDATE")}
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
