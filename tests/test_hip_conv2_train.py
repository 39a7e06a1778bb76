"""GPU checks of the bf16 matrix-core conv2 of the COMA update: csrc/conv4x4_train.hip behind ippm_conv4x4_bf16_forward / _grad_input /
_grad_weight, networks._Conv4x4Bf16, the learners' and the trainer's ``conv2_update="bf16"``.  The reference of every numerical check is
the CPU restatement of the contract (tests/conv2_train_ref.py), never the code under test; the dense tolerances are ``MARGIN`` spreads
between the float32 and the float64 restatement of the same case, the unit of the native forwards' tests."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import actor_native_ref as AR
import conv2_train_ref as R
import critic_native_ref as CR
from configs import make_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096                 # sentinel floats before and after every output
SENTINEL = -12345.678
OPS = {"y": "ippm_conv4x4_bf16_forward", "gx": "ippm_conv4x4_bf16_grad_input", "gw": "ippm_conv4x4_bf16_grad_weight"}


def _lib():
    from ippmarl import _ffi
    return _ffi, _ffi.load_library()


def _chunk():
    return _lib()[0].CONV4X4_WGRAD_CHUNK


def _scratch(B, ih, iw, fill=0xFF):
    _ffi, lib = _lib()
    nbytes = C.c_int64(0)
    _ffi.check(lib.ippm_conv4x4_bf16_scratch_bytes(B, ih, iw, C.addressof(nbytes)), "ippm_conv4x4_bf16_scratch_bytes")
    chunks = (B + _chunk() - 1) // _chunk()
    assert nbytes.value == (4 << 20) + chunks * (4 << 20)          # two bf16 packs, one float32 [16,256,256] partial per chunk
    return torch.full((nbytes.value,), fill, dtype=torch.uint8, device=DEV)      # (0xFF bytes: NaN as bf16 and as float32)


def _run(op, a, b, B, ih, iw, scratch_fill=0xFF):
    """One entry point on an output pre-filled with NaN between two bands of GUARD sentinels, and a pre-filled scratch
    -> the output on the CPU; asserts rc == 0 and intact sentinels."""
    _ffi, lib = _lib()
    shape = {"y": (B, ih - 3, iw - 3, R.CH), "gx": (B, ih, iw, R.CH), "gw": R.W_SHAPE}[op]
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    out = whole[GUARD:GUARD + n]
    out.fill_(float("nan"))
    a, b = a.to(DEV).contiguous(), b.to(DEV).contiguous()
    scratch = _scratch(B, ih, iw, scratch_fill)
    _ffi.check(getattr(lib, OPS[op])(a.data_ptr(), b.data_ptr(), B, ih, iw, scratch.data_ptr(), out.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), OPS[op])
    torch.cuda.synchronize()
    assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all()), (op, "sentinels overwritten")
    return out.cpu().view(shape)


def _all_ops(x, w, gy, ops=("y", "gx", "gw"), **kw):
    B, ih, iw, _ = x.shape
    args = {"y": (x, w), "gx": (gy, w), "gw": (gy, x)}
    return {op: _run(op, *args[op], B, ih, iw, **kw) for op in ops}


# ---- 1. small integers: bit for bit against the float64 restatement -----------------------------------------------------------------
INT_SHAPES = [(1, 4, 4), (3, 5, 6), (5, 7, 7), (8, 7, 7), (9, 7, 7), (3, 11, 11)]


@pytest.mark.parametrize("shape", INT_SHAPES)
def test_small_integers_bit_for_bit(shape):
    want = R.int_case(*shape)
    got = _all_ops(R.int_x(*shape), R.int_w(), R.int_gy(*shape))
    for op in ("y", "gx", "gw"):
        assert float(want[op].abs().max()) < 2 ** 24
        bad = int((got[op].double() != want[op]).sum())
        assert bad == 0, (shape, op, bad, want[op].numel())


@pytest.mark.parametrize("rel", ["chunk-1", "chunk", "chunk+1", "2chunk+3"])
def test_weight_gradient_chunk_edges_bit_for_bit(rel):
    K = _chunk()
    B = {"chunk-1": K - 1, "chunk": K, "chunk+1": K + 1, "2chunk+3": 2 * K + 3}[rel]
    want = R.int_case(B, 7, 7, ops=("gw",))["gw"]
    assert float(want.abs().max()) < 2 ** 24
    got = _run("gw", R.int_gy(B, 7, 7), R.int_x(B, 7, 7), B, 7, 7)
    assert torch.equal(got.double(), want), (B, int((got.double() != want).sum()))


# ---- 2. dense real case -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.DENSE_SEEDS)
def test_dense_case_within_four_spreads(seed):
    x, w, gy = R.dense_inputs(seed)
    assert x.shape[0] == 300 and tuple(x.shape[1:3]) == (7, 7)
    got = _all_ops(x, w, gy)
    spreads = R.dense_spreads(seed)
    errs = {op: float((got[op].double() - spreads[op][1]).abs().max()) for op in got}
    for op in got:
        print(f"seed {seed} {op}: spread {spreads[op][0]:.3e}; device error {errs[op]:.3e}; |ref| up to {float(spreads[op][1].abs().max()):.3e}")
    for op in got:
        assert spreads[op][0] > 0 and errs[op] <= R.MARGIN * spreads[op][0], (op, errs[op], spreads[op][0])


# ---- 3. independence and determinism --------------------------------------------------------------------------------------------------
def test_a_sample_does_not_depend_on_its_batch():
    x, w, gy = R.dense_inputs(R.DENSE_SEEDS[0])
    got = _all_ops(x, w, gy, ops=("y", "gx"))
    for i in (0, 127, 128, 299):
        one = _all_ops(x[i:i + 1], w, gy[i:i + 1], ops=("y", "gx"))
        assert torch.equal(one["y"][0], got["y"][i]) and torch.equal(one["gx"][0], got["gx"][i]), i


def test_weight_gradient_is_deterministic_and_ignores_prior_content():
    x, w, gy = R.dense_inputs(R.DENSE_SEEDS[0])
    B = x.shape[0]
    assert B > _chunk()                                   # more than one partial sum
    first = _run("gw", gy, x, B, 7, 7, scratch_fill=0xFF)
    second = _run("gw", gy, x, B, 7, 7, scratch_fill=0x7F)    # (0x7F7F7F7F: another pattern, a large finite float)
    assert not torch.isnan(first).any()
    assert torch.equal(first, second)


# ---- 4. guard bands (every _run asserts them; these are the shapes whose rows end inside a tile) ---------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 6), (9, 7, 7)])
def test_guard_bands_stay_intact(shape):
    got = _all_ops(R.int_x(*shape), R.int_w(), R.int_gy(*shape))
    for op, t in got.items():
        assert not torch.isnan(t).any(), (shape, op)       # and every element was written


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    _ffi, lib = _lib()
    B, ih, iw = 3, 5, 6
    stream = torch.cuda.current_stream().cuda_stream
    x, w, gy = R.int_x(B, ih, iw).to(DEV), R.int_w().to(DEV), R.int_gy(B, ih, iw).to(DEV)
    outs = {"y": torch.full((B, ih - 3, iw - 3, R.CH), float("nan"), device=DEV), "gx": torch.full((B, ih, iw, R.CH), float("nan"), device=DEV),
            "gw": torch.full(R.W_SHAPE, float("nan"), device=DEV)}
    args = {"y": (x, w), "gx": (gy, w), "gw": (gy, x)}
    scratch = _scratch(B, ih, iw)
    nbytes = C.c_int64(0)

    def fails(rc, name, word):
        msg = lib.ippm_last_error().decode()
        assert rc == -1 and name in msg and word in msg, (rc, name, msg)

    name = "ippm_conv4x4_bf16_scratch_bytes"
    fails(lib.ippm_conv4x4_bf16_scratch_bytes(B, ih, iw, None), name, "null")
    fails(lib.ippm_conv4x4_bf16_scratch_bytes(0, ih, iw, C.addressof(nbytes)), name, "batch")
    for bad in (3, 12):
        fails(lib.ippm_conv4x4_bf16_scratch_bytes(B, bad, iw, C.addressof(nbytes)), name, "[4, 11]")
        fails(lib.ippm_conv4x4_bf16_scratch_bytes(B, ih, bad, C.addressof(nbytes)), name, "[4, 11]")
    for op, name in OPS.items():
        fn, (a, b), out = getattr(lib, name), args[op], outs[op]
        ok = [a.data_ptr(), b.data_ptr(), B, ih, iw, scratch.data_ptr(), out.data_ptr(), stream]
        for slot in (0, 1, 5, 6):
            call = list(ok)
            call[slot] = None
            fails(fn(*call), name, "null")
        for bad in (0, -1):
            call = list(ok)
            call[2] = bad
            fails(fn(*call), name, "batch")
        for slot in (3, 4):
            for bad in (3, 12):
                call = list(ok)
                call[slot] = bad
                fails(fn(*call), name, "[4, 11]")
        call = list(ok)
        call[5] = scratch.data_ptr() + 8
        fails(fn(*call), name, "16-byte aligned")
    torch.cuda.synchronize()
    for op, out in outs.items():
        assert bool(torch.isnan(out).all()), op                 # nothing was launched
    assert lib.ippm_conv4x4_bf16_scratch_bytes(B, ih, iw, C.addressof(nbytes)) == 0 and nbytes.value > 0


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


@pytest.mark.parametrize("kind", ["critic", "actor"])
def test_device_gradients_against_the_restated_network(kind, monkeypatch):
    """The .grad of every used parameter of a device network run under conv2_update("bf16") -- conv1's included: it flows through the new
    input gradient -- against a CPU float64 network whose conv2 is the restatement.  The loss is a mean squared error of fc3's output
    against seeded targets (so that every gradient, fc3's bias included, carries the network's rounding and not only a sum's)."""
    from ippmarl import networks
    seed, B = 5, 64
    net, ref, inputs = _module(kind, seed)
    target = torch.randn(B, net.n_actions, generator=torch.Generator().manual_seed(seed))

    def loss_fn(out):
        return (out - target.to(out.device, out.dtype)).square().mean()

    g32, g64 = R.net_grads(ref, inputs, loss_fn, torch.float32), R.net_grads(ref, inputs, loss_fn, torch.float64)
    calls = []
    real = networks._Conv4x4Bf16.apply
    monkeypatch.setattr(networks._Conv4x4Bf16, "apply", staticmethod(lambda *a: (calls.append(1), real(*a))[1]))
    with networks.conv2_update("bf16"):
        out, _ = net.trunk(inputs.to(DEV))
    loss_fn(out).backward()
    torch.cuda.synchronize()
    assert len(calls) == 1
    assert net.fc2.weight.grad is None and net.fc2.bias.grad is None
    figures = {}
    for name in g64:
        layer, what = name.split(".")
        got = getattr(getattr(net, layer), what).grad.cpu().double()
        figures[name] = (float((got - g64[name]).abs().max()), float((g32[name].double() - g64[name]).abs().max()))
        print(f"{kind} {name}: spread {figures[name][1]:.3e}; device error {figures[name][0]:.3e}; |grad| up to {float(g64[name].abs().max()):.3e}")
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
    """In bf16 mode the Function runs exactly once per learner ``backward``; a default-mode trainer built afterwards in the same process
    never runs it (the mode is the learner's, not the process's), even with the bf16 trainer still alive."""
    from ippmarl import networks
    monkeypatch.delenv(networks.CONV2_UPDATE_ENV, raising=False)
    calls = []
    real = networks._Conv4x4Bf16.apply
    monkeypatch.setattr(networks._Conv4x4Bf16, "apply", staticmethod(lambda *a: (calls.append(1), real(*a))[1]))
    tr = _trainer(conv2_update="bf16")
    assert tr.conv2_update == tr.critic_learner.conv2_update == tr.actor_learner.conv2_update == "bf16"
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
    assert len(calls) == 2 + steps
    plain = _trainer(seed=6)
    assert plain.conv2_update == plain.critic_learner.conv2_update == plain.actor_learner.conv2_update == "float32"
    assert plain.rollout("train")["faults"] == 0
    stats = plain.update()
    assert np.isfinite(stats["critic_loss"]) and len(calls) == 2 + steps
    tr.rollout("train")
    tr.update()                                                        # ... and the first trainer has kept its own mode
    assert len(calls) == 2 + 2 * steps


# ---- 7. the trainer ---------------------------------------------------------------------------------------------------------------------------
def test_trainer_round_at_the_smallest_env_count(monkeypatch):
    from ippmarl import networks
    monkeypatch.setenv(networks.CONV2_UPDATE_ENV, "bf16")             # the environment variable is how bench.py gets the switch
    tr = _trainer(seed=8, n_envs=1)
    assert tr.conv2_update == "bf16" and tr.T * tr.E * tr.N // tr.batch_number >= 1
    before = {net: torch.cat([p.detach().reshape(-1).clone() for p in getattr(tr, net).parameters()]) for net in ("actor", "critic")}
    assert tr.rollout("train")["faults"] == 0
    stats = tr.update()
    assert np.isfinite(stats["critic_loss"]) and np.isfinite(stats["actor_loss"])
    for net in ("actor", "critic"):
        module = getattr(tr, net)
        after = torch.cat([p.detach().reshape(-1) for p in module.parameters()])
        assert bool(torch.isfinite(after).all()) and float((after - before[net]).abs().max()) > 0, net
        assert module.conv2.weight.grad is not None and bool(torch.isfinite(module.conv2.weight.grad).all())
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


def _run_recorded_round():
    """One round of a trainer replayed from hipGraphs beside the same round run launch by launch, both with conv2_update="bf16" and from
    identical training state -> {net: flat parameters of (eager, recorded)}, and the parameters before the round."""
    from ippmarl import networks
    saved = os.environ.pop(networks.CONV2_UPDATE_ENV, None)
    try:
        eager, rec = (_trainer(seed=11, graphs=True, conv2_update="bf16") for _ in range(2))
        for tr in (eager, rec):              # first round launch by launch (kernel selection, allocator)
            torch.manual_seed(12)
            tr.rollout("train")
            tr.update()
        _copy_training_state(eager, rec)
        rec.capture_graphs()
        before = {net: _flat(getattr(eager, net)).clone() for net in ("critic", "actor")}
        for tr in (eager, rec):
            torch.manual_seed(20)
            assert tr.rollout("train")["faults"] == 0
            stats = tr.update()
            assert np.isfinite(stats["critic_loss"]) and np.isfinite(stats["actor_loss"])
        assert rec._update_graph is not None
        return {net: (_flat(getattr(eager, net)).clone(), _flat(getattr(rec, net)).clone()) for net in ("critic", "actor")}, before
    finally:
        if saved is not None:
            os.environ[networks.CONV2_UPDATE_ENV] = saved


def test_recorded_bf16_round_equals_eager_round(tmp_path):
    """tests/conv2_recorded_rounds.py in a process of its own (the convolution library in deterministic mode: its default float32
    weight-gradient kernels, which conv1 still uses, sum with atomics): after a recorded round both nets' parameters are the eager
    round's bit for bit, finite, and moved."""
    out = tmp_path / "digests.json"
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv2_recorded_rounds.py")
    env = {k: v for k, v in os.environ.items() if k != "IPPMARL_CONV2_UPDATE"}
    run = subprocess.run([sys.executable, script, str(out)], env=env, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]        # (nothing further is started after a failure)
    with open(out) as f:
        nets = json.load(f)
    assert set(nets) == {"critic", "actor"}
    for net, n in nets.items():
        print(f"{net}: {n['differ']} of {n['numel']} parameters differ eager - recorded (max {n['max']:.3e}); the round moved them by up to {n['moved']:.3e}")
    for net, n in nets.items():
        assert n["finite"] and n["moved"] > 0, (net, n)
        assert n["digests"][0] == n["digests"][1] and n["differ"] == 0, (net, n)
