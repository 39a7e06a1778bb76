"""GPU checks of ``adam="native"`` above the kernel: optim_native.NativeAdam, the learners' and the trainer's switch, the inference packs the
step keeps current, state dicts, and the recorded round.  Numbers are judged against the restated contract (tests/adam_ref.py) in MARGIN
spreads; the kernel itself is tests/test_hip_adam.py's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adam_ref as R
from configs import make_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL_ENV = ("IPPMARL_ADAM", "IPPMARL_HEAD_UPDATE", "IPPMARL_TRUNK_UPDATE", "IPPMARL_CONV2_UPDATE", "IPPMARL_ACTOR_INFERENCE",
           "IPPMARL_CRITIC_INFERENCE")


def _lib():
    from ippmarl import _ffi
    return _ffi, _ffi.load_library()


def _count_lib(monkeypatch, name):
    """Calls of a C entry point, counted through a wrapper on the bound function."""
    _, lib = _lib()
    real, calls = getattr(lib, name), []
    monkeypatch.setattr(lib, name, lambda *a: (calls.append(a), real(*a))[1])
    return calls


def _params64(**kw):
    """2 UAVs on a 64 x 64 grid, as the native forwards' trainer tests."""
    return make_params("small", experiment__missions__n_agents=2, sensor__field_of_view__angle_x=99.0, sensor__field_of_view__angle_y=99.0, **kw)


def _trainer(seed=5, n_envs=3, params=None, **kw):
    from ippmarl.trainer import COMATrainer
    torch.manual_seed(seed)
    return COMATrainer(params or _params64(), n_envs=n_envs, first_episode=3, **kw)


def _used(module):
    from ippmarl import optim_native
    return optim_native.used_parameters(module)


def _np(t):
    return t.detach().cpu().numpy()


# ---- 8. native against torch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["actor", "critic"])
def test_native_and_torch_learners_on_the_same_gradients(kind):
    """An adam="native" learner and an adam="torch" learner from the same parameters, fed the same hand-written gradients for 10 apply()
    calls: both end within MARGIN spreads of the float64 restatement (parameters and both moments)."""
    from ippmarl import optim_native
    from ippmarl.learners import ActorLearner, CriticLearner
    from ippmarl.networks import ActorNetwork, CriticNetwork
    params = make_params("small")
    torch.manual_seed(21)
    net = (ActorNetwork if kind == "actor" else CriticNetwork)(params)
    learners = {}
    for mode in ("native", "torch"):
        twin = type(net)(params)
        twin.load_state_dict(net.state_dict())
        learners[mode] = (ActorLearner if kind == "actor" else CriticLearner)(params, twin, torch.device(DEV), adam=mode)
    assert type(learners["native"].optimizer) is optim_native.NativeAdam and type(learners["torch"].optimizer) is torch.optim.Adam
    module = {mode: (lrn.actor if kind == "actor" else lrn.critic) for mode, lrn in learners.items()}
    shapes = [tuple(p.shape) for p in _used(module["native"])]
    lr = learners["native"].lr
    p0 = [_np(p) for p in _used(module["native"])]
    a32, a64 = R.Adam(p0, lr, np.float32), R.Adam(p0, lr, np.float64)
    states = torch.zeros(2, 11, 11, 12, device=DEV)
    for s in range(10):
        grads = R.gradients(300 + s, shapes)
        a32.step(grads)
        a64.step(grads)
        for mode, lrn in learners.items():
            for p, g in zip(_used(module[mode]), grads):
                p.grad = torch.from_numpy(g).to(DEV)
            if kind == "critic":
                lrn._pending = (states, torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(2, device=DEV), torch.zeros((), device=DEV),
                                torch.zeros(2, 1, device=DEV))
                assert bool(torch.isfinite(lrn.apply()).all())
            else:
                lrn.apply()
    torch.cuda.synchronize()
    spread = R.spreads(a32, a64)
    for mode, lrn in learners.items():
        used = _used(module[mode])
        st = lrn.optimizer.state
        got = {"p": [_np(p) for p in used], "m": [_np(st[p]["exp_avg"]) for p in used], "v": [_np(st[p]["exp_avg_sq"]) for p in used]}
        err = R.errors(got, a64)
        print(f"{kind} {mode}: spreads {spread}; errors {err}")
        for k in err:
            assert spread[k] > 0 and err[k] <= R.MARGIN * spread[k], (mode, k, err[k], spread[k])
        assert int(float(st[used[0]]["step"])) == 10
    native = learners["native"]
    assert all(not bool(p.grad.any()) for p in _used(module["native"]))                    # the step cleared what it read
    assert module["native"].fc2.weight not in native.optimizer.state                       # fc2 is listed, never stepped
    assert [id(p) for p in native.optimizer.param_groups[0]["params"]] == [id(p) for p in module["native"].parameters()]


def test_step_needs_every_gradient_and_zero_grad_rules():
    from ippmarl import _ffi, optim_native
    ps = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (5, 300)]
    opt = optim_native.NativeAdam(ps, lr=1e-3)
    ps[0].grad = torch.ones(5, device=DEV)
    with pytest.raises(_ffi.IppmError, match="no gradient"):
        opt.step()
    ps[1].grad = torch.ones(300, device=DEV)
    versions = [p._version for p in ps]
    opt.step()
    assert [p._version for p in ps] != versions and all(p._version > v for p, v in zip(ps, versions))
    assert not bool(ps[1].grad.any()) and opt.steps_taken() == 1
    ps[1].grad.fill_(3.0)                   # (breaking the rule on purpose: somebody else wrote the gradients)
    opt.zero_grad(set_to_none=False)        # right behind step(): launches nothing, so the write survives
    assert bool((ps[1].grad == 3.0).all())
    opt.zero_grad(set_to_none=False)        # the previous call was not step(): fills
    assert not bool(ps[1].grad.any())
    ps[1].grad.fill_(3.0)
    opt.step()
    ps[1].grad.fill_(3.0)
    opt.zero_grad(force=True)
    assert not bool(ps[1].grad.any()) and opt.steps_taken() == 2


# ---- 9. one trainer round ---------------------------------------------------------------------------------------------------------------------
def test_trainer_round_at_one_env(monkeypatch):
    from ippmarl import optim_native
    for v in ALL_ENV:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv(optim_native.ENV_VAR, "native")                # the environment variable is how bench.py gets the switch
    steps = _count_lib(monkeypatch, "ippm_adam_step")
    built = []
    real_init = torch.optim.Adam.__init__
    monkeypatch.setattr(torch.optim.Adam, "__init__", lambda self, *a, **k: (built.append(1), real_init(self, *a, **k))[1])
    tr = _trainer(seed=8, n_envs=1)
    assert tr.adam == tr.critic_learner.adam == tr.actor_learner.adam == "native"
    assert type(tr.critic_learner.optimizer) is type(tr.actor_learner.optimizer) is optim_native.NativeAdam
    before = {net: [p.detach().clone() for p in _used(getattr(tr, net))] for net in ("actor", "critic")}
    assert tr.rollout("train")["faults"] == 0
    stats = tr.update()
    torch.cuda.synchronize()
    assert np.isfinite(stats["critic_loss"]) and np.isfinite(stats["actor_loss"])
    assert len(steps) == stats["adam_steps"] == 2 * tr.data_passes * tr.batch_number and not built
    for net in ("actor", "critic"):
        module = getattr(tr, net)
        for p, b in zip(_used(module), before[net]):
            assert bool(torch.isfinite(p).all()) and float((p.detach() - b).abs().max()) > 0
            assert p.grad is not None and not bool(p.grad.any())        # every gradient of the used layers is zero after update()
        opt = getattr(tr, net + "_learner").optimizer
        assert opt.steps_taken() == stats["adam_steps"] // 2
    assert tr.rollout("train")["faults"] == 0                           # the diagnostics path keeps working
    stats = tr.update(diagnostics=True)
    assert np.isfinite(stats["critic_loss"]) and tr.last_diagnostics and len(steps) == 2 * stats["adam_steps"] and not built


# ---- 10. the packs ------------------------------------------------------------------------------------------------------------------------------
def test_steps_keep_both_inference_packs_current(monkeypatch):
    from ippmarl.actor_native import NativeActor
    from ippmarl.critic_native import NativeCritic
    for v in ALL_ENV:
        monkeypatch.delenv(v, raising=False)
    tr = _trainer(seed=9, n_envs=2, adam="native", actor_inference="native", critic_inference="native")
    assert tr.rollout("train")["faults"] == 0
    mine = tr.native_actor()
    assert tr.actor_learner.optimizer._pack is mine
    bystander = NativeActor(tr.actor, tr.device)                         # unattached, built before the update
    old_pack = bystander.packed.clone()
    critic_packs = _count_lib(monkeypatch, "ippm_critic_pack")
    actor_packs = _count_lib(monkeypatch, "ippm_actor_pack")
    steps = _count_lib(monkeypatch, "ippm_adam_step")
    stats = tr.update()
    torch.cuda.synchronize()
    assert tr.critic_learner.optimizer._pack is tr._native_critic
    assert len(steps) == stats["adam_steps"] and all(c[12] for c in steps)              # every step carried a pack
    assert [c for c in critic_packs if c[11] == tr._native_critic.packed.data_ptr()] == []
    assert [c for c in actor_packs if c[11] == mine.packed.data_ptr()] == []
    assert len(actor_packs) == 0
    fresh = {}
    for native, cls, module in ((tr._native_critic, NativeCritic, tr.critic), (mine, NativeActor, tr.actor)):
        fresh[cls] = cls(module, tr.device)
        differ = int((fresh[cls].packed != native.packed).sum())
        assert differ == 0, (cls.__name__, differ)
        assert native._stamp == fresh[cls]._stamp                                        # ... and the pack is marked current
    # the stale-pack rule: the unattached pack is old until its owner looks, and its next forward looks (sync sees the written parameters)
    assert torch.equal(bystander.packed, old_pack) and not torch.equal(old_pack, fresh[NativeActor].packed)
    obs = tr.buf_obs[0, 0].reshape(tr.E * tr.N, 11, 11, 7)
    got, want = bystander(obs, 0.1)[0], fresh[NativeActor](obs, 0.1)[0]
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(bystander.packed, fresh[NativeActor].packed)


# ---- 11. state dicts ----------------------------------------------------------------------------------------------------------------------------
def _tensors(seed, sizes=(4099, 1, 65537)):
    return [torch.nn.Parameter(torch.from_numpy(p).to(DEV)) for p in R.parameters(seed, [(n,) for n in sizes])]


def _feed(params, grads):
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g).to(DEV)


def test_state_dict_round_trips():
    from ippmarl import optim_native
    lr, sizes = 1e-3, (4099, 1, 65537)
    shapes = [(n,) for n in sizes]
    grads = [R.gradients(400 + s, shapes) for s in range(5)]
    a = _tensors(30)
    opt_a = optim_native.NativeAdam(a, lr)
    for s in range(3):
        _feed(a, grads[s])
        opt_a.step()
    sd = opt_a.state_dict()
    assert set(sd) == {"state", "param_groups"} and sd["param_groups"][0]["params"] == [0, 1, 2] and float(sd["state"][0]["step"]) == 3.0
    # native -> native continues bit for bit
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    opt_b = optim_native.NativeAdam(b, lr)
    opt_b.load_state_dict(sd)
    assert opt_b.steps_taken() == 3 and torch.equal(opt_a.blob, opt_b.blob)            # counters, powers and moments: the same bytes
    # native -> torch: the moments bit for bit, step the count
    c = [torch.nn.Parameter(p.detach().clone()) for p in a]
    opt_c = torch.optim.Adam(c, lr=lr)
    opt_c.load_state_dict(sd)
    for pa, pc in zip(a, c):
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt_c.state[pc][k].view(torch.int32), opt_a.state[pa][k].view(torch.int32))
        assert float(opt_c.state[pc]["step"]) == 3.0
    for s in (3, 4):
        for params, opt in ((a, opt_a), (b, opt_b)):
            _feed(params, grads[s])
            opt.step()
    torch.cuda.synchronize()
    assert torch.equal(opt_a.blob, opt_b.blob) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    # torch -> native is accepted and continues within MARGIN spreads of the float64 restatement of all five steps
    d = _tensors(30)
    p0 = [_np(p) for p in d]
    opt_t = torch.optim.Adam(d, lr=lr)
    for s in range(3):
        _feed(d, grads[s])
        opt_t.step()
    opt_d = optim_native.NativeAdam(d, lr)
    opt_d.load_state_dict(opt_t.state_dict())
    assert opt_d.steps_taken() == 3
    assert float(opt_d.state[d[0]]["beta1_power"]) == 0.9 * 0.9 * 0.9 and float(opt_d.state[d[0]]["beta2_power"]) == 0.999 * 0.999 * 0.999
    for s in (3, 4):
        _feed(d, grads[s])
        opt_d.step()
    a32, a64 = R.Adam(p0, lr, np.float32), R.Adam(p0, lr, np.float64)
    for s in range(5):
        a32.step(grads[s])
        a64.step(grads[s])
    spread = R.spreads(a32, a64)
    got = {"p": [_np(p) for p in d], "m": [_np(opt_d.state[p]["exp_avg"]) for p in d], "v": [_np(opt_d.state[p]["exp_avg_sq"]) for p in d]}
    err = R.errors(got, a64)
    print(f"torch -> native: spreads {spread}; errors {err}")
    for k in err:
        assert err[k] <= R.MARGIN * spread[k], (k, err[k], spread[k])
    # (and the run that never left the native optimizer is the float32 restatement itself)
    for x, y in zip(a, a32.p):
        assert np.array_equal(_np(x).view(np.uint32), y.view(np.uint32))


# ---- 12. graphs -----------------------------------------------------------------------------------------------------------------------------------
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
    agree), all three with adam="native", graphs=True, head_update="bf16" and from identical training state
    -> {net: flat parameters of (eager, eager again, recorded)}, the parameters before the round, and the optimizers' step counts."""
    saved = {v: os.environ.pop(v, None) for v in ALL_ENV}
    try:
        eager, again, rec = (_trainer(seed=11, graphs=True, head_update="bf16", adam="native") for _ in range(3))
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
        counts = {name: [getattr(tr, name).optimizer.steps_taken() for tr in (eager, again, rec)] for name in ("critic_learner", "actor_learner")}
        return {net: tuple(_flat(getattr(tr, net)).clone() for tr in (eager, again, rec)) for net in ("critic", "actor")}, before, counts
    finally:
        for v, value in saved.items():
            if value is not None:
                os.environ[v] = value


def test_recorded_round_equals_eager_round(tmp_path):
    """tests/adam_recorded_rounds.py in a process of its own (the convolution library in deterministic mode): two eager rounds agree, and
    after a recorded round both nets' parameters are the eager round's bit for bit, finite, and moved; the counters in the state blobs
    advanced under replay as they did launch by launch."""
    out = tmp_path / "digests.json"
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "adam_recorded_rounds.py")
    env = {k: v for k, v in os.environ.items() if k not in ALL_ENV}
    run = subprocess.run([sys.executable, script, str(out)], env=env, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]        # (nothing further is started after a failure)
    with open(out) as f:
        result = json.load(f)
    nets, counts = result["nets"], result["counts"]
    assert set(nets) == {"critic", "actor"}
    for net, n in nets.items():
        print(f"{net}: {n['differ']} of {n['numel']} parameters differ eager - recorded (max {n['max']:.3e}), {n['premise_differ']} eager - eager; "
              f"the round moved them by up to {n['moved']:.3e}")
    for net, n in nets.items():
        assert n["finite"] and n["moved"] > 0, (net, n)
        assert n["digests"][0] == n["digests"][1] and n["premise_differ"] == 0, (net, n)      # the premise: two eager rounds agree
        assert n["digests"][0] == n["digests"][2] and n["differ"] == 0, (net, n)
    for name, c in counts.items():
        assert c[0] == c[1] == c[2] > 0, (name, c)


# ---- 13. the default ------------------------------------------------------------------------------------------------------------------------------
def test_default_round_never_touches_the_native_step(monkeypatch):
    for v in ALL_ENV:
        monkeypatch.delenv(v, raising=False)
    steps = _count_lib(monkeypatch, "ippm_adam_step")
    tr = _trainer(seed=6, n_envs=1)
    assert tr.adam == "torch"
    for learner in (tr.critic_learner, tr.actor_learner):
        assert learner.adam == "torch" and type(learner.optimizer) is torch.optim.Adam
    assert tr.rollout("train")["faults"] == 0
    stats = tr.update()
    assert np.isfinite(stats["critic_loss"]) and not steps
