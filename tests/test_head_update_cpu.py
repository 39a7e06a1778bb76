"""CPU side of the native COMA heads' checks: the switch parses as documented, a CPU network and a CPU learner ignore it (the silent
float32 fallback), and the restatement the GPU tests compare against (tests/head_train_ref.py) is plain linear algebra on bf16-exact
operands and the learners' own loss on real ones."""
import inspect
import pickle

import pytest

torch = pytest.importorskip("torch")

import head_train_ref as R  # noqa: E402
from configs import make_params  # noqa: E402


def test_head_update_switch_parsing(monkeypatch):
    from ippmarl import _ffi, networks
    from ippmarl.learners import ActorLearner, CriticLearner
    from ippmarl.trainer import COMATrainer
    resolve, var = networks.resolve_head_update, networks.HEAD_UPDATE_ENV
    assert var == "IPPMARL_HEAD_UPDATE" and networks.HEAD_UPDATE_MODES == ("float32", "bf16")
    monkeypatch.delenv(var, raising=False)
    assert resolve() == "float32" and resolve(None) == "float32"
    assert resolve("bf16") == "bf16" and resolve("float32") == "float32"
    monkeypatch.setenv(var, "bf16")
    assert resolve() == "bf16"
    assert resolve("float32") == "float32"           # the argument wins over the environment
    monkeypatch.setenv(var, "")
    assert resolve() == "float32"
    monkeypatch.setenv(var, "native")
    with pytest.raises(ValueError, match="head update must be one of"):
        resolve()
    with pytest.raises(ValueError, match="head update must be one of"):
        resolve("fp16")
    with pytest.raises(ValueError, match="head update must be one of"):
        with networks.head_update("fast"):
            pass
    # the trainer reads the environment (None), the learners take the mode as an argument; the keyword sits before conv2_update
    assert inspect.signature(COMATrainer.__init__).parameters["head_update"].default is None
    assert list(inspect.signature(COMATrainer.__init__).parameters)[-3:] == ["head_update", "conv2_update", "trunk_update"]
    for cls in (CriticLearner, ActorLearner):
        params = inspect.signature(cls.__init__).parameters
        assert params["head_update"].default == "float32" and list(params)[-3:] == ["head_update", "conv2_update", "trunk_update"]
    # the chunk constant of the header and its Python mirror
    assert R.header_chunk() == _ffi.HEAD_WGRAD_CHUNK == R.CHUNK


def test_context_manager_nests_and_restores():
    from ippmarl import networks
    mode, trunk, conv2 = networks._HEAD_UPDATE.get, networks._TRUNK_UPDATE.get, networks._CONV2_UPDATE.get
    assert mode() == "float32"
    with networks.head_update("bf16"):
        assert mode() == "bf16" and trunk() == "float32" and conv2() == "float32"      # a variable of its own
        with networks.trunk_update("bf16"):
            assert mode() == "bf16" and trunk() == "bf16"
        with networks.head_update("float32"):
            assert mode() == "float32"
        assert mode() == "bf16"
    assert mode() == "float32"
    with pytest.raises(RuntimeError):
        with networks.head_update("bf16"):
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
    with networks.head_update(mode):
        out, _ = net.trunk(inputs)
    out.square().mean().backward()
    return out.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("kind", ["critic", "actor"])
def test_cpu_network_ignores_the_switch(kind):
    """The fallback: under head_update("bf16") a CPU network gives the outputs and gradients of "float32", bit for bit."""
    net, inputs = _net_and_inputs(kind)
    o0, g0 = _run(net, inputs, "float32")
    o1, g1 = _run(net, inputs, "bf16")
    assert torch.equal(o0, o1)
    assert set(g0) == set(g1) and {"fc1.weight", "fc1.bias", "fc3.weight", "fc3.bias"} <= set(g0) and not any(n.startswith("fc2") for n in g0)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_cpu_critic_learner_ignores_the_switch():
    """A learner on the CPU keeps the PyTorch head and loss under head_update="bf16": the loss and every gradient, bit for bit."""
    from ippmarl.learners import CriticLearner
    got = []
    for mode in ("float32", "bf16"):
        net, states = _net_and_inputs("critic", seed=5)
        learner = CriticLearner(make_params("small"), net, torch.device("cpu"), head_update=mode)
        assert learner.head_update == mode
        g = torch.Generator().manual_seed(9)
        actions, td = torch.randint(0, net.n_actions, (states.shape[0],), generator=g).int(), torch.randn(states.shape[0], generator=g)
        loss = learner.backward(states, actions, td)
        got.append((loss, {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}))
    assert torch.equal(got[0][0], got[1][0])
    assert set(got[0][1]) == set(got[1][1]) and "fc3.bias" in got[0][1] and not any(n.startswith("fc2") for n in got[0][1])
    for n in got[0][1]:
        assert torch.equal(got[0][1][n], got[1][1][n]), n


@pytest.mark.parametrize("kind", ["critic", "actor"])
def test_module_pickle_does_not_change_under_the_context_manager(kind):
    net, inputs = _net_and_inputs(kind, seed=4)
    before = pickle.dumps(net)
    attrs = set(vars(net)) | set(vars(net.fc1)) | set(vars(net.fc3))
    _run(net, inputs, "bf16")
    net.zero_grad(set_to_none=True)
    assert (set(vars(net)) | set(vars(net.fc1)) | set(vars(net.fc3))) == attrs
    assert pickle.dumps(net) == before


@pytest.mark.parametrize("A", R.ACTION_SETS)
def test_restated_integer_case_is_plain_linear_algebra(A):
    """On the small integers the restated head equals float64 F.linear and torch.autograd.grad of it, but for the ONE rounding the
    contract keeps there (a1 enters fc3 and gW3 as bf16): with a1 replaced by its bf16 value both are plain, in float64 and in float32."""
    import torch.nn.functional as F
    B = 5
    w1, b1, w3, b3 = R.int_weights(A)
    h, dl = R.int_h(B), R.int_dlogits(B, A)
    for t in (w1, w3, h, dl):
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    a1, logits = R.int_forward(B, A)
    assert torch.equal(a1, torch.relu(F.linear(h.double(), w1.double(), b1.double())))
    assert 0.2 < float((a1 == 0).double().mean()) < 0.8 and float(a1.max()) > 256           # the ReLU clips; a1 is not bf16-exact
    a1r = a1.to(torch.bfloat16).double()
    assert torch.equal(logits, F.linear(a1r, w3.double(), b3.double())) and float(logits.abs().max()) < 2 ** 24
    a32, l32 = R.forward(h, w1, b1, w3, b3, torch.float32)
    assert torch.equal(a32.double(), a1) and torch.equal(l32.double(), logits)
    # gradients: fc3 at the rounded a1, the ReLU's mask, fc1
    p = [t.double().requires_grad_(True) for t in (h, w1, b1, w3, b3)]
    z = torch.relu(F.linear(p[0], p[1], p[2]))
    ga1 = dl.double() @ w3.double()
    gh, gw1, gb1 = torch.autograd.grad(z, p[:3], ga1)
    a1p = a1r.clone().requires_grad_(True)
    _, gw3, gb3 = torch.autograd.grad(F.linear(a1p, p[3], p[4]), (a1p, p[3], p[4]), dl.double())
    want = {"gh": gh, "gw1": gw1, "gb1": gb1, "gw3": gw3, "gb3": gb3}
    for dtype in (torch.float64, torch.float32):
        got = R.backward(dl, 1.0, a1.to(dtype), h, w1, w3, dtype)
        for k in want:
            assert torch.equal(got[k].double(), want[k]) and 0 < float(want[k].abs().max()) < 2 ** 24, (k, dtype)
    assert all(torch.equal(R.int_backward(B, A)[k], want[k]) for k in want)


def test_restated_losses_are_the_learners_arithmetic():
    """The restated losses against the learners' own PyTorch expressions and autograd, in float64: the critic's squared error, the actor's
    masked policy-gradient loss with the advantage held constant; K7's floors are hit by the all-zero and the single-action rows."""
    B, A, eps = 12, 6, 0.2
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(B, A, generator=g).double().requires_grad_(True)
    q, td = torch.randn(B, A, generator=g), torch.randn(B, generator=g)
    action = torch.randint(0, A, (B,), generator=g).int()
    mask = (torch.rand(B, A, generator=g) < 0.6).to(torch.uint8)
    mask[0] = 0
    mask[1] = 0
    mask[1, action[1]] = 1
    mask[2:].scatter_(1, action[2:].long().view(-1, 1), 1)
    idx = action.long().view(-1, 1)
    # critic
    qc = logits.gather(1, idx)
    loss = torch.square(qc - td.double().view(-1, 1)).squeeze().mean()
    (dq,) = torch.autograd.grad(loss, logits)
    r = R.critic_loss(logits.detach(), action, td, torch.float64)
    assert torch.allclose(r["loss"], loss.detach(), rtol=1e-13) and torch.allclose(r["dq"], dq, rtol=1e-13, atol=0)
    assert torch.equal(r["q_chosen"], qc.detach().squeeze(1))
    # actor (learners.ActorLearner.backward)
    probs = (1 - eps) * torch.softmax(logits, dim=1) + eps / A
    r = R.actor_loss(logits.detach(), q, mask, action, eps, torch.float64)
    m = mask.double()
    pm = probs.detach() * m
    pn = (pm / pm.sum(1, keepdim=True).clamp_min(1e-5)).clamp_min(1e-5)
    adv = q.double().gather(1, idx).squeeze(1) - (pn * q.double() * m).sum(1)
    assert torch.equal(r["adv"], adv) and float(pn[0].max()) == 1e-5 and float(pn[1, action[1]]) == 1.0
    loss = -(adv * torch.log(probs).gather(1, idx).squeeze(1) * (m.sum(-1) / A)).mean()
    (dl,) = torch.autograd.grad(loss, logits)
    assert torch.allclose(r["loss"], loss.detach(), rtol=1e-13) and torch.allclose(r["dlogits"], dl, rtol=1e-10, atol=1e-18)
    assert torch.equal(r["probs"], probs.detach()) and not bool(r["dlogits"][0].any()) and bool(r["dlogits"][2:].any())
    assert float(r["adv"][1]) == 0.0            # a single valid action is its own baseline
