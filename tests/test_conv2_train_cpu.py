"""CPU side of the bf16 conv2 update checks: the restatement the GPU tests compare against (tests/conv2_train_ref.py) is the gradient of
its own forward, the switch parses as documented, and a CPU network ignores it (the silent float32 fallback)."""
import os
import pickle

import pytest

torch = pytest.importorskip("torch")

import conv2_train_ref as R  # noqa: E402
from configs import make_params  # noqa: E402


@pytest.mark.parametrize("shape", [(1, 4, 4), (3, 5, 6), (2, 7, 7)])
def test_restated_gradients_are_the_gradients_of_the_restated_forward(shape):
    """On bf16-exact operands (the small integers) the rounding is the identity, so gx and gw must equal torch.autograd.grad of the
    float64 forward with gy as the output gradient -- bit for bit: every sum is an integer below 2^24."""
    x, w, gy = R.int_x(*shape), R.int_w(), R.int_gy(*shape)
    for t in (x, w, gy):
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    # (differentiated without the casts: autograd would round the GRADIENT to bf16 on its way back through ``.to(bfloat16)``; on these
    #  operands the casts are the identity, so this is the restated forward -- asserted)
    y = torch.nn.functional.conv2d(x64.permute(0, 3, 1, 2), w64).permute(0, 2, 3, 1)
    assert torch.equal(y.detach(), R.forward(x, w, torch.float64))
    gx, gw = torch.autograd.grad(y, (x64, w64), gy.double())
    assert torch.equal(R.grad_input(gy, w, torch.float64), gx)
    assert torch.equal(R.grad_weight(gy, x, torch.float64), gw)
    assert torch.equal(R.grad_input(gy, w, torch.float32).double(), gx) and torch.equal(R.grad_weight(gy, x, torch.float32).double(), gw)
    assert float(gw.abs().max()) < 2 ** 24 and float(gx.abs().max()) > 0
    # RestatedConv2 (the seam tests' CPU network) is the same three formulas in logical NCHW
    xn = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    wn = w.double().requires_grad_(True)
    y = R.RestatedConv2.apply(xn, wn)
    assert torch.equal(y.permute(0, 2, 3, 1), R.forward(x, w, torch.float64))
    gxn, gwn = torch.autograd.grad(y, (xn, wn), gy.double().permute(0, 3, 1, 2))
    assert torch.equal(gxn.permute(0, 2, 3, 1), gx) and torch.equal(gwn, gw)


def test_conv2_update_switch_parsing(monkeypatch):
    import inspect

    from ippmarl import _ffi, networks
    from ippmarl.learners import ActorLearner, CriticLearner
    from ippmarl.trainer import COMATrainer
    resolve, var = networks.resolve_conv2_update, networks.CONV2_UPDATE_ENV
    assert var == "IPPMARL_CONV2_UPDATE"
    monkeypatch.delenv(var, raising=False)
    assert resolve() == "float32" and resolve(None) == "float32"
    assert resolve("bf16") == "bf16" and resolve("float32") == "float32"
    monkeypatch.setenv(var, "bf16")
    assert resolve() == "bf16"
    assert resolve("float32") == "float32"           # the argument wins over the environment
    monkeypatch.setenv(var, "")
    assert resolve() == "float32"
    monkeypatch.setenv(var, "native")
    with pytest.raises(ValueError, match="conv2 update"):
        resolve()
    with pytest.raises(ValueError, match="conv2 update"):
        resolve("fp16")
    with pytest.raises(ValueError, match="conv2 update"):
        with networks.conv2_update("fast"):
            pass
    assert inspect.signature(COMATrainer.__init__).parameters["conv2_update"].default is None
    # the learners take the mode as an argument and do not read the environment
    for cls in (CriticLearner, ActorLearner):
        assert inspect.signature(cls.__init__).parameters["conv2_update"].default == "float32"
    # the chunk constant of the header and its Python mirror
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ippmarl.h")).read()
    assert f"#define IPPM_CONV4X4_WGRAD_CHUNK {_ffi.CONV4X4_WGRAD_CHUNK}\n" in header


def test_context_manager_nests_and_restores():
    from ippmarl import networks
    mode = networks._CONV2_UPDATE.get
    assert mode() == "float32"
    with networks.conv2_update("bf16"):
        assert mode() == "bf16"
        with networks.conv2_update("float32"):
            assert mode() == "float32"
        assert mode() == "bf16"
    assert mode() == "float32"
    with pytest.raises(RuntimeError):
        with networks.conv2_update("bf16"):
            raise RuntimeError("x")
    assert mode() == "float32"


def _critic_and_states(seed=3, batch=6):
    from ippmarl.networks import CriticNetwork
    torch.manual_seed(seed)
    net = CriticNetwork(make_params("small"))
    states = torch.rand(batch, 11, 11, 12, generator=torch.Generator().manual_seed(seed))
    return net, states


def _run(net, states, mode):
    from ippmarl import networks
    net.zero_grad(set_to_none=True)
    with networks.conv2_update(mode):
        q, logp = net(states)
    q.square().mean().backward()
    return q.detach().clone(), logp.clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}


def test_cpu_network_ignores_the_switch():
    """The fallback: under conv2_update("bf16") a CPU CriticNetwork gives the outputs and gradients of "float32", bit for bit."""
    net, states = _critic_and_states()
    q0, l0, g0 = _run(net, states, "float32")
    q1, l1, g1 = _run(net, states, "bf16")
    assert torch.equal(q0, q1) and torch.equal(l0, l1)
    assert set(g0) == set(g1) and "conv2.weight" in g0 and not any(n.startswith("fc2") for n in g0)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_module_pickle_does_not_change_under_the_context_manager():
    net, states = _critic_and_states(seed=4)
    before = pickle.dumps(net)
    attrs = set(vars(net)) | set(vars(net.conv2))
    _run(net, states, "bf16")
    net.zero_grad(set_to_none=True)
    assert (set(vars(net)) | set(vars(net.conv2))) == attrs
    assert pickle.dumps(net) == before
