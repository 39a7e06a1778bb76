"""CPU side of the bf16 trunk update checks: the switch parses as documented, a CPU network ignores it (the silent float32 fallback), and
the restatement the GPU tests compare against (tests/trunk_train_ref.py) is plain convolution on bf16-exact operands."""
import inspect
import pickle

import pytest

torch = pytest.importorskip("torch")

import trunk_train_ref as R  # noqa: E402
from configs import make_params  # noqa: E402


def test_trunk_update_switch_parsing(monkeypatch):
    from ippmarl import _ffi, networks
    from ippmarl.learners import ActorLearner, CriticLearner
    from ippmarl.trainer import COMATrainer
    resolve, var = networks.resolve_trunk_update, networks.TRUNK_UPDATE_ENV
    assert var == "IPPMARL_TRUNK_UPDATE" and networks.TRUNK_UPDATE_MODES == ("float32", "bf16")
    monkeypatch.delenv(var, raising=False)
    assert resolve() == "float32" and resolve(None) == "float32"
    assert resolve("bf16") == "bf16" and resolve("float32") == "float32"
    monkeypatch.setenv(var, "bf16")
    assert resolve() == "bf16"
    assert resolve("float32") == "float32"           # the argument wins over the environment
    monkeypatch.setenv(var, "")
    assert resolve() == "float32"
    monkeypatch.setenv(var, "native")
    with pytest.raises(ValueError, match="trunk update"):
        resolve()
    with pytest.raises(ValueError, match="trunk update"):
        resolve("fp16")
    with pytest.raises(ValueError, match="trunk update"):
        with networks.trunk_update("fast"):
            pass
    # the trainer reads the environment (None), the learners take the mode as an argument; the new keyword comes last
    assert inspect.signature(COMATrainer.__init__).parameters["trunk_update"].default is None
    assert list(inspect.signature(COMATrainer.__init__).parameters)[-2:] == ["conv2_update", "trunk_update"]
    for cls in (CriticLearner, ActorLearner):
        params = inspect.signature(cls.__init__).parameters
        assert params["trunk_update"].default == "float32" and list(params)[-2:] == ["conv2_update", "trunk_update"]
    # the chunk constant of the header and its Python mirror
    assert R.header_chunk() == _ffi.CONV5X5_WGRAD_CHUNK


def test_context_manager_nests_and_restores():
    from ippmarl import networks
    mode, conv2 = networks._TRUNK_UPDATE.get, networks._CONV2_UPDATE.get
    assert mode() == "float32"
    with networks.trunk_update("bf16"):
        assert mode() == "bf16" and conv2() == "float32"      # a variable of its own
        with networks.trunk_update("float32"):
            assert mode() == "float32"
        assert mode() == "bf16"
    assert mode() == "float32"
    with pytest.raises(RuntimeError):
        with networks.trunk_update("bf16"):
            raise RuntimeError("x")
    assert mode() == "float32"


def _net_and_inputs(kind, seed=3, batch=6):
    from ippmarl.networks import ActorNetwork, CriticNetwork
    torch.manual_seed(seed)
    net = (ActorNetwork if kind == "actor" else CriticNetwork)(make_params("small"))
    inputs = torch.rand(batch, 11, 11, 7 if kind == "actor" else 12, generator=torch.Generator().manual_seed(seed))
    return net, inputs


def _run(net, inputs, mode):
    from ippmarl import networks
    net.zero_grad(set_to_none=True)
    with networks.trunk_update(mode):
        out, _ = net.trunk(inputs)
    out.square().mean().backward()
    return out.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("kind", ["critic", "actor"])
def test_cpu_network_ignores_the_switch(kind):
    """The fallback: under trunk_update("bf16") a CPU network gives the outputs and gradients of "float32", bit for bit."""
    net, inputs = _net_and_inputs(kind)
    o0, g0 = _run(net, inputs, "float32")
    o1, g1 = _run(net, inputs, "bf16")
    assert torch.equal(o0, o1)
    assert set(g0) == set(g1) and {"conv1.weight", "conv3.weight"} <= set(g0) and not any(n.startswith("fc2") for n in g0)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


@pytest.mark.parametrize("kind", ["critic", "actor"])
def test_module_pickle_does_not_change_under_the_context_manager(kind):
    net, inputs = _net_and_inputs(kind, seed=4)
    before = pickle.dumps(net)
    attrs = set(vars(net)) | set(vars(net.conv1)) | set(vars(net.conv3))
    _run(net, inputs, "bf16")
    net.zero_grad(set_to_none=True)
    assert (set(vars(net)) | set(vars(net.conv1)) | set(vars(net.conv3))) == attrs
    assert pickle.dumps(net) == before


@pytest.mark.parametrize("planes", R.PLANES)
def test_restated_integer_case_is_plain_convolution(planes):
    """On bf16-exact operands (the small integers) the rounding is the identity: the restated forward equals float64 conv2d, the restated
    weight gradient equals torch.autograd.grad of it, in float64 and in float32 -- every sum is an integer below 2^24."""
    B = 3
    x, w, b, gy = R.int_x(B, planes), R.int_w(planes), R.int_bias(), R.int_gy(B)
    for t in (x, w, gy):
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    x64, w64 = x.double().permute(0, 3, 1, 2), w.double().requires_grad_(True)
    y = torch.nn.functional.conv2d(x64, w64)
    assert torch.equal(y.detach().permute(0, 2, 3, 1), R.forward(x, w, None, torch.float64))
    assert torch.equal(R.int_forward(B, planes, False), R.forward(x, w, None, torch.float64))
    assert torch.equal(torch.relu(y.detach() + b.double().view(1, -1, 1, 1)).permute(0, 2, 3, 1), R.int_forward(B, planes, True))
    assert float((R.int_forward(B, planes, True) == 0).double().mean()) > 0.2        # the ReLU clips a good share
    (gw,) = torch.autograd.grad(y, (w64,), gy.double().permute(0, 3, 1, 2))
    assert torch.equal(R.int_grad_weight(B, planes), gw) and torch.equal(R.grad_weight(gy, x, torch.float32).double(), gw)
    assert 0 < float(gw.abs().max()) < 2 ** 24
    # RestatedConv (the seam tests' CPU network) is the same formulas in logical NCHW
    wn = w.double().requires_grad_(True)
    yn = R.RestatedConv.apply(x64, wn)
    assert torch.equal(yn.detach(), y.detach())
    (gwn,) = torch.autograd.grad(yn, (wn,), gy.double().permute(0, 3, 1, 2))
    assert torch.equal(gwn, gw)
