"""Shared by test_critic_native_cpu.py and test_hip_critic_native.py: the two constructed 12-plane networks the critic tests run, with
their states and their references.  The numerical contract itself is restated in tests/actor_native_ref.py (``emulate_trunk``,
``emulate_head``: shape-agnostic); that file's SHAPES and observation builders are the actor's 7-plane ones, so the networks and
states are built here.  Nothing here calls the code under test.

``float64`` is the reference; ``float32`` is a second legitimate accumulation order, and the spread between the two is the unit every
dense tolerance is stated in (``MARGIN`` spreads, the actor tests' value)."""
import functools

import torch

from actor_native_ref import MARGIN, _dense_layer, _sparse_layer, emulate_head, emulate_trunk  # noqa: F401

PLANES = 12
SHAPES = {"conv1": (256, PLANES, 5, 5), "conv2": (256, 256, 4, 4), "conv3": (256, 256, 4, 4), "fc1": (256, 256)}
TRUNK = tuple(SHAPES)
EXACT_SEED, EXACT_BATCH = 17, 300
DENSE_SEEDS, DENSE_BATCH = (1, 2, 3), 1024


def emulate(net, states, dtype):
    """states float32 [B,11,11,12], net: {layer: (weight, bias)} float32 in PyTorch's layouts -> Q [B,A] in ``dtype``."""
    return emulate_head(net, emulate_trunk(net, states, dtype), dtype)


def gather(q, actions):
    return q.gather(1, actions.long().view(-1, 1)).squeeze(1)


def module_net(module):
    """The five used layers of a CriticNetwork as the dict ``emulate`` takes (CPU float32 copies)."""
    return {n: (getattr(module, n).weight.detach().cpu().float().clone(), getattr(module, n).bias.detach().cpu().float().clone())
            for n in TRUNK + ("fc3",)}


def spread(net, states):
    """(max |emulate(float32) - emulate(float64)|, emulate(float64)) of a network on ``states`` (CPU tensors)."""
    q32, q64 = emulate(net, states, torch.float32), emulate(net, states, torch.float64)
    return float((q32.double() - q64).abs().max()), q64


# ---- the exact network: sparse integer weights, {0,1} biases and states ----------------------------------------------------------
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
def exact_states(seed, batch):
    return torch.randint(0, 2, (batch, 11, 11, PLANES), generator=torch.Generator().manual_seed(seed + 1)).float()


@functools.lru_cache(maxsize=None)
def exact_activations(seed, batch, dtype):
    """Every layer's activation of the exact network (conv1, conv2, conv3, fc1), by the same formula as ``emulate_trunk``."""
    trunk, acts = _exact_trunk(seed), []
    h = exact_states(seed, batch).permute(0, 3, 1, 2)
    for name in ("conv1", "conv2", "conv3"):
        w, b = trunk[name]
        h = torch.relu(torch.nn.functional.conv2d(h.to(torch.bfloat16).to(dtype), w.to(torch.bfloat16).to(dtype), b.to(dtype)))
        acts.append(h)
    acts.append(emulate_trunk(trunk, exact_states(seed, batch), dtype))
    return acts


def exact_q(seed, batch, n_actions, dtype=torch.float64):
    return emulate_head(exact_net(seed, n_actions), exact_activations(seed, batch, dtype)[-1], dtype)


@functools.lru_cache(maxsize=None)
def exact_actions(seed, batch, n_actions):
    return torch.randint(0, n_actions, (batch,), generator=torch.Generator().manual_seed(seed + 2), dtype=torch.int32)


# ---- the dense network: He-normal weights, N(0, 0.1) biases -----------------------------------------------------------------------
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
def dense_states(seed, batch):
    """``rand`` with whole planes dropped per sample, as actor_native_ref.dense_obs."""
    g = torch.Generator().manual_seed(seed + 7)
    return torch.rand(batch, 11, 11, PLANES, generator=g) * (torch.rand(batch, 1, 1, PLANES, generator=g) < 0.7)


@functools.lru_cache(maxsize=None)
def dense_hidden(seed, batch, dtype):
    return emulate_trunk(_dense_trunk(seed), dense_states(seed, batch), dtype)


def dense_q(seed, batch, n_actions, dtype):
    return emulate_head(dense_net(seed, n_actions), dense_hidden(seed, batch, dtype), dtype)


def dense_spread(seed, n_actions, batch=DENSE_BATCH):
    """(max |emulate(float32) - emulate(float64)| over the dense case, emulate(float64))."""
    q32, q64 = dense_q(seed, batch, n_actions, torch.float32), dense_q(seed, batch, n_actions, torch.float64)
    return float((q32.double() - q64).abs().max()), q64
