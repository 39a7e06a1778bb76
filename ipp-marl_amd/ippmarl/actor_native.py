"""Opt-in native inference of the actor: libippmarl's bf16 matrix-core forward (ippm_actor_forward) instead of the float32 PyTorch
module, for the no-grad consumers of a trained actor (rollouts, evaluation, deployment).  The update keeps the float32 module.

Numerical contract: every layer's input and weights are bf16 (round to nearest even), products accumulate in
float32, the float32 bias is added to the accumulator, ReLU, one rounding to bf16 at the store; logits, softmax and the epsilon mix
are float32.  Deterministic: a sample's probabilities are the same bits alone and at any position of any batch.

``actor_inference`` / ``IPPMARL_ACTOR_INFERENCE`` select the path: "torch" (default) or "native"."""
from __future__ import annotations

from typing import Optional

import torch

from . import _ffi, switches
from .native_net import MODES, NativeNet  # noqa: F401

ENV_VAR = switches.TABLE["actor_inference"].env_var


def resolve_mode(actor_inference: Optional[str] = None) -> str:
    """The actor's inference path: the argument, else the environment variable, else "torch"; anything but "torch" / "native" raises.
    (The critic's switch: critic_native.resolve_mode.)"""
    return switches.resolve("actor_inference", actor_inference)


class NativeActor(NativeNet):
    """Holds the packed bf16 weights of ``actor_module`` and the forward's scratch on ``device`` (native_net.NativeNet: ``refresh()``,
    ``sync()``, ``reserve()`` and the rules that keep the pack current); ``__call__(obs, eps)`` is the module's no-grad forward,
    ``-> (probs, None)``."""

    PREFIX, WHO, WHAT, PLANES = "ippm_actor", "NativeActor", "actor", _ffi.ACTOR_PLANES

    def forward(self, obs: torch.Tensor, eps=0.0, logits: bool = False):
        """obs float32 [B,11,11,7] -> (probs [B,A], logits [B,A] or None).  ``eps``: a float, or a 0-dim float32 device tensor that
        the kernel reads (what a recorded graph needs)."""
        obs = self._input(obs)
        self.sync()
        B = obs.shape[0]
        probs = torch.empty(B, self.n_actions, dtype=torch.float32, device=self.device)
        lg = torch.empty_like(probs) if logits else None
        eps_dev = None
        if isinstance(eps, torch.Tensor):
            if eps.dtype != torch.float32 or eps.device != self.device or eps.numel() != 1:
                raise _ffi.IppmError("NativeActor: a tensor epsilon must be one float32 on the actor's device")
            eps_dev, eps = eps.data_ptr(), 0.0
        _ffi.check(self.lib.ippm_actor_forward(self.packed.data_ptr(), obs.data_ptr(), B, self.n_actions, float(eps), eps_dev,
                                               self.scratch.data_ptr(), probs.data_ptr(), _ffi.ptr(lg), self._stream()),
                   "ippm_actor_forward")
        return probs, lg

    def __call__(self, obs: torch.Tensor, eps=0.0):
        probs, _ = self.forward(obs, eps)
        return probs, None


class DeployedActor:
    """An actor module behind the interface ``COMATest.execute`` uses of its network (``to``, ``eval``, ``forward(obs, eps)``), with the
    forward run by a NativeActor.  Set it as ``COMATest.net``, or let ``deployment()`` do so."""

    def __init__(self, actor_module):
        self.module = actor_module
        self.native = None

    def to(self, device):
        self.module = self.module.to(device)
        if self.native is None or self.native.module is not self.module or self.native.device != NativeActor._device(device):
            self.native = NativeActor(self.module, device)
        return self

    def eval(self):
        self.module.eval()
        return self

    def forward(self, obs: torch.Tensor, eps=0.0):
        if self.native is None:
            raise _ffi.IppmError("DeployedActor: call to(device) first")
        return self.native(obs, eps)

    __call__ = forward


def deployment(params, writer, num_episode, model_path: Optional[str] = None, actor_inference: Optional[str] = None):
    """``ippmarl.coma_test.COMATest(params, writer, num_episode, model_path)`` honouring the inference switch of COMATrainer:
    with "native" (argument, or IPPMARL_ACTOR_INFERENCE when it is None) the greedy deployment's forward passes go through the same
    NativeActor; with "torch" this is the plain class."""
    from .coma_test import COMATest
    mode = resolve_mode(actor_inference)
    ct = COMATest(params, writer, num_episode, model_path)
    if mode == "native":
        ct.net = DeployedActor(ct._load_net())
    ct.actor_inference = mode
    return ct
