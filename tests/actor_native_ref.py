"""Shared by test_actor_native_cpu.py and test_hip_actor_native.py: the numerical contract of the native actor forward restated in
PyTorch on the CPU (``emulate``), and the two constructed networks the tests run.  Nothing here calls the code under test.

Contract: each layer's input and weights are rounded to bf16 and promoted to the accumulation type, the bias is
added in that type, ReLU; logits, softmax and the epsilon mix stay in that type.  ``float64`` is the reference; ``float32`` is a second
legitimate accumulation order, and the spread between the two is the unit the dense tolerances are stated in."""
import functools

import torch
import torch.nn.functional as F

SHAPES = {"conv1": (256, 7, 5, 5), "conv2": (256, 256, 4, 4), "conv3": (256, 256, 4, 4), "fc1": (256, 256)}
TRUNK = tuple(SHAPES)


def _bf16(x, dtype):
    return x.to(torch.bfloat16).to(dtype)


def emulate_trunk(net, obs, dtype):
    """obs float32 [B,11,11,7], net: {layer: (weight, bias)} float32 in PyTorch's layouts -> fc1's activation [B,256] in ``dtype``."""
    h = obs.to(torch.float32).permute(0, 3, 1, 2)
    for name in ("conv1", "conv2", "conv3"):
        w, b = net[name]
        h = F.relu(F.conv2d(_bf16(h, dtype), _bf16(w, dtype), b.to(dtype)))
    w, b = net["fc1"]
    return F.relu(F.linear(_bf16(h.flatten(1), dtype), _bf16(w, dtype), b.to(dtype)))


def emulate_head(net, h, dtype):
    w, b = net["fc3"]
    return F.linear(_bf16(h, dtype), _bf16(w, dtype), b.to(dtype))


def emulate(net, obs, dtype):
    """-> logits [B,A] in ``dtype``."""
    return emulate_head(net, emulate_trunk(net, obs, dtype), dtype)


def mix(logits, eps):
    """(1 - eps) * softmax + eps / A in the logits' type."""
    return (1 - eps) * torch.softmax(logits, dim=1) + eps / logits.shape[1]


def module_net(module):
    """The five used layers of an ActorNetwork as the dict ``emulate`` takes (CPU float32 copies)."""
    return {n: (getattr(module, n).weight.detach().cpu().float().clone(), getattr(module, n).bias.detach().cpu().float().clone())
            for n in TRUNK + ("fc3",)}


# ---- the exact network: sparse integer weights, {0,1} biases and observations --------------------------------------------------
def _sparse_layer(shape, g):
    """Every output unit gets exactly three non-zeros (+1, +1, -1) at seeded random positions; bias in {0, 1}."""
    out, fan = shape[0], int(torch.tensor(shape[1:]).prod())
    w = torch.zeros(out, fan)
    for o in range(out):
        idx = torch.randperm(fan, generator=g)[:3]
        w[o, idx] = torch.tensor([1.0, 1.0, -1.0])
    return w.view(shape), torch.randint(0, 2, (out,), generator=g).float()


@functools.lru_cache(maxsize=None)
def _exact_trunk(seed):
    g = torch.Generator().manual_seed(seed)
    return {n: _sparse_layer(SHAPES[n], g) for n in TRUNK}


@functools.lru_cache(maxsize=None)
def exact_net(seed, n_actions):
    net = dict(_exact_trunk(seed))
    net["fc3"] = _sparse_layer((n_actions, 256), torch.Generator().manual_seed(1000 * seed + n_actions))
    return net


@functools.lru_cache(maxsize=None)
def exact_obs(seed, batch):
    return torch.randint(0, 2, (batch, 11, 11, 7), generator=torch.Generator().manual_seed(seed + 1)).float()


@functools.lru_cache(maxsize=None)
def exact_hidden(seed, batch, dtype):
    return emulate_trunk(_exact_trunk(seed), exact_obs(seed, batch), dtype)


def exact_logits(seed, batch, n_actions, dtype=torch.float64):
    return emulate_head(exact_net(seed, n_actions), exact_hidden(seed, batch, dtype), dtype)


# ---- the dense network: He-normal weights, N(0, 0.1) biases -----------------------------------------------------------------------
def _dense_layer(shape, g):
    fan = int(torch.tensor(shape[1:]).prod())
    return torch.randn(shape, generator=g) * (2.0 / fan) ** 0.5, torch.randn(shape[0], generator=g) * 0.1


@functools.lru_cache(maxsize=None)
def _dense_trunk(seed):
    g = torch.Generator().manual_seed(seed)
    return {n: _dense_layer(SHAPES[n], g) for n in TRUNK}


@functools.lru_cache(maxsize=None)
def dense_net(seed, n_actions):
    net = dict(_dense_trunk(seed))
    net["fc3"] = _dense_layer((n_actions, 256), torch.Generator().manual_seed(1000 * seed + n_actions))
    return net


@functools.lru_cache(maxsize=None)
def dense_obs(seed, batch):
    g = torch.Generator().manual_seed(seed + 7)
    return torch.rand(batch, 11, 11, 7, generator=g) * (torch.rand(batch, 1, 1, 7, generator=g) < 0.7)


@functools.lru_cache(maxsize=None)
def dense_hidden(seed, batch, dtype):
    return emulate_trunk(_dense_trunk(seed), dense_obs(seed, batch), dtype)


def dense_logits(seed, batch, n_actions, dtype):
    return emulate_head(dense_net(seed, n_actions), dense_hidden(seed, batch, dtype), dtype)


DENSE_SEEDS, DENSE_BATCH = (1, 2, 3), 1024
EXACT_SEED, EXACT_BATCH = 11, 300
MARGIN = 4          # the device may be this many float32-vs-float64 spreads away from the float64 reference
EXCUSED_CAP = 0.10  # at most this share of rows may have a top-2 gap too small to pin the decision


def spreads(seed, n_actions, batch=DENSE_BATCH, eps=0.0):
    """(d_logits, d_probs, logits64, probs64): max |emulate(float32) - emulate(float64)| over the dense case, and the reference."""
    l32, l64 = dense_logits(seed, batch, n_actions, torch.float32), dense_logits(seed, batch, n_actions, torch.float64)
    p32, p64 = mix(l32, eps), mix(l64, eps)
    return float((l32.double() - l64).abs().max()), float((p32.double() - p64).abs().max()), l64, p64


def top2_gap(probs):
    top = probs.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]
