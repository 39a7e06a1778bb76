"""CPU checks of the ``adam`` switch (optim_native, the learners, the trainer's signature) and of the restated contract itself
(tests/adam_ref.py): that it IS Adam as the reference configures it, measured against ``torch.optim.Adam`` on CPU tensors."""
import inspect

import numpy as np
import pytest
import torch

import adam_ref as R
from configs import make_params


def test_switch_parsing(monkeypatch):
    from ippmarl import optim_native
    monkeypatch.delenv(optim_native.ENV_VAR, raising=False)
    assert optim_native.ENV_VAR == "IPPMARL_ADAM" and optim_native.MODES == ("torch", "native")
    assert optim_native.resolve_mode() == "torch" and optim_native.resolve_mode(None) == "torch"
    monkeypatch.setenv(optim_native.ENV_VAR, "native")
    assert optim_native.resolve_mode() == "native"
    assert optim_native.resolve_mode("torch") == "torch"                 # the argument wins over the environment
    monkeypatch.setenv(optim_native.ENV_VAR, "")
    assert optim_native.resolve_mode() == "torch"
    for bad in ("fused", "Native", "1"):
        with pytest.raises(ValueError, match="adam"):
            optim_native.resolve_mode(bad)
        monkeypatch.setenv(optim_native.ENV_VAR, bad)
        with pytest.raises(ValueError, match="adam"):
            optim_native.resolve_mode()
        assert optim_native.resolve_mode("native") == "native"


def test_signatures():
    from ippmarl.learners import ActorLearner, CriticLearner
    from ippmarl.trainer import COMATrainer
    for cls, default in ((COMATrainer, None), (CriticLearner, "torch"), (ActorLearner, "torch")):
        sig = inspect.signature(cls.__init__)
        names = list(sig.parameters)
        assert sig.parameters["adam"].default == default, cls
        assert names[-3:] == ["head_update", "conv2_update", "trunk_update"], cls
        assert names.index("adam") == names.index("head_update") - 1, cls
    names = list(inspect.signature(COMATrainer.__init__).parameters)
    assert names[names.index("adam") - 1] == "critic_inference"
    for cls in (CriticLearner, ActorLearner):
        names = list(inspect.signature(cls.__init__).parameters)
        assert names[names.index("adam") - 1] == "capturable"


def test_trainer_rejects_an_unknown_mode(monkeypatch):
    """The trainer resolves ``adam`` before it builds anything that needs the GPU."""
    from ippmarl import optim_native
    from ippmarl.trainer import COMATrainer
    monkeypatch.delenv(optim_native.ENV_VAR, raising=False)
    with pytest.raises(ValueError, match="adam"):
        COMATrainer(make_params("small"), n_envs=1, adam="fused")
    monkeypatch.setenv(optim_native.ENV_VAR, "both")
    with pytest.raises(ValueError, match="adam"):
        COMATrainer(make_params("small"), n_envs=1)


def test_restatement_is_adam_as_the_reference_configures_it():
    """50 steps of 200 000 elements at lr 1e-4 on the tests' gradient family: the float32 restatement and torch.optim.Adam on CPU tensors
    both stay within MARGIN spreads of the float64 restatement (the float32 restatement sits at 1.0 by definition), and nothing leaves the
    normal range of float32 on this input -- subnormals are outside the contract."""
    n, steps, lr = 200_000, 50, 1e-4
    p0 = R.parameters(1, [(n,)])
    a32, a64 = R.Adam(p0, lr, np.float32), R.Adam(p0, lr, np.float64)
    tp = torch.from_numpy(p0[0].copy()).requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=lr)
    tiny = float(np.finfo(np.float32).tiny)
    for s in range(steps):
        g = R.gradients(100 + s, [(n,)])
        a32.step(g)
        a64.step(g)
        tp.grad = torch.from_numpy(g[0].copy())
        opt.step()
        for x in (a32.m[0], a32.v[0], a32.p[0]):
            nz = np.abs(x[x != 0])
            assert nz.size and float(nz.min()) >= tiny
    spread = R.spreads(a32, a64)
    st = opt.state[tp]
    got = {"p": [tp.detach().numpy()], "m": [st["exp_avg"].numpy()], "v": [st["exp_avg_sq"].numpy()]}
    err = R.errors(got, a64)
    same = float(np.mean(got["p"][0] == a32.p[0]))
    print(f"spreads {spread}; torch.optim.Adam errors {err} ({ {k: err[k] / spread[k] for k in err} } spreads); "
          f"{same:.3f} of the parameters equal the float32 restatement's bits; smallest v {float(a32.v[0][a32.v[0] > 0].min()):.3e}")
    assert float(st["step"]) == steps == a32.t
    for k in err:
        assert spread[k] > 0 and err[k] <= R.MARGIN * spread[k], (k, err[k], spread[k])
    assert float(np.max(np.abs(a32.p[0] - p0[0]))) > 10 * lr           # the parameters moved


def test_restatement_counters_and_zero_gradient():
    """The powers are products (no pow); a zero gradient leaves m and v at exactly 0 and the parameter in place (0 / (0 + eps) = 0)."""
    a = R.Adam([np.ones(4, np.float32)], 1e-3, np.float32)
    for _ in range(3):
        a.step([np.zeros(4, np.float32)])
    assert a.t == 3 and a.b1p == 0.9 * 0.9 * 0.9 and a.b2p == 0.999 * 0.999 * 0.999
    assert not a.m[0].any() and not a.v[0].any() and np.array_equal(a.p[0], np.ones(4, np.float32))


def test_a_cpu_parameter_is_refused():
    from ippmarl import _ffi, optim_native
    p = torch.zeros(8, requires_grad=True)
    with pytest.raises(_ffi.IppmError, match="GPU only"):
        optim_native.NativeAdam([p], lr=1e-3)


def test_default_learners_hold_torch_adam(monkeypatch):
    from ippmarl import optim_native
    from ippmarl.learners import ActorLearner, CriticLearner
    from ippmarl.networks import ActorNetwork, CriticNetwork
    monkeypatch.delenv(optim_native.ENV_VAR, raising=False)
    params = make_params("small")
    critic = CriticLearner(params, CriticNetwork(params), torch.device("cpu"))
    actor = ActorLearner(params, ActorNetwork(params), torch.device("cpu"))
    for learner in (critic, actor):
        assert learner.adam == "torch" and type(learner.optimizer) is torch.optim.Adam
    with pytest.raises(ValueError, match="adam"):
        CriticLearner(params, CriticNetwork(params), torch.device("cpu"), adam="fused")
    with pytest.raises(_ffi_error()):
        ActorLearner(params, ActorNetwork(params), torch.device("cpu"), adam="native")     # no CPU fallback


def _ffi_error():
    from ippmarl import _ffi
    return _ffi.IppmError
