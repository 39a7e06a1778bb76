"""Opt-in native inference of the actor: libippmarl's bf16 matrix-core forward (ippm_actor_forward) instead of the float32 PyTorch
module, for the no-grad consumers of a trained actor (rollouts, evaluation, deployment).  The update keeps the float32 module.

Numerical contract: every layer's input and weights are bf16 (round to nearest even), products accumulate in
float32, the float32 bias is added to the accumulator, ReLU, one rounding to bf16 at the store; logits, softmax and the epsilon mix
are float32.  Deterministic: a sample's probabilities are the same bits alone and at any position of any batch.

``actor_inference`` / ``IPPMARL_ACTOR_INFERENCE`` select the path: "torch" (default) or "native"."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _ffi

MODES = ("torch", "native")
ENV_VAR = "IPPMARL_ACTOR_INFERENCE"
_LAYERS = ("conv1", "conv2", "conv3", "fc1", "fc3")   # fc2 is never used by the network (networks._ConvTrunk)


def resolve_mode(actor_inference: Optional[str] = None) -> str:
    """The inference path: the argument, else the environment variable, else "torch"; anything but "torch" / "native" raises."""
    mode = actor_inference if actor_inference is not None else os.environ.get(ENV_VAR, "") or "torch"
    if mode not in MODES:
        raise ValueError(f"actor inference must be one of {MODES}, got {mode!r}")
    return mode


class NativeActor:
    """Holds the packed bf16 weights of ``actor_module`` and the forward's scratch on ``device``.  ``refresh()`` repacks from the
    module's current parameters (one kernel, capturable); ``__call__(obs, eps)`` is the module's no-grad forward, ``-> (probs, None)``.
    A call also repacks by itself when the parameters' version counters say that they were written since the last pack, so a
    ``load_state_dict`` or an eager optimizer step cannot leave a stale pack behind; a replayed graph changes no counter, which is why the
    trainer records ``refresh()`` into its update graph.  A repack that is only recorded during a capture does not count as a pack:
    ``COMATrainer.capture_graphs`` repacks before it starts recording."""

    def __init__(self, actor_module, device):
        self.module = actor_module
        self.device = self._device(device)
        self.lib = _ffi.load_library()
        self.n_actions = int(actor_module.fc3.out_features)
        nbytes = C.c_int64(0)
        _ffi.check(self.lib.ippm_actor_pack_bytes(self.n_actions, C.addressof(nbytes)), "ippm_actor_pack_bytes")
        self.packed = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        self.scratch = None
        self._capacity = 0
        self._stamp = None
        self.refresh()

    @staticmethod
    def _device(device) -> torch.device:
        device = torch.device(device)
        if device.type != "cuda":
            raise _ffi.IppmError("NativeActor: the native actor forward runs on the GPU only (there is no CPU fallback)")
        return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device

    def _params(self):
        out = []
        for name in _LAYERS:
            layer = getattr(self.module, name)
            out += [layer.weight, layer.bias]
        return out

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def refresh(self):
        params = self._params()
        for p in params:
            if p.device != self.device or p.dtype != torch.float32 or not p.is_contiguous():
                raise _ffi.IppmError("NativeActor: the actor's parameters must be contiguous float32 tensors on the actor's device")
        _ffi.check(self.lib.ippm_actor_pack(*[p.data_ptr() for p in params], self.n_actions, self.packed.data_ptr(), self._stream()),
                   "ippm_actor_pack")
        # (a launch that is only being RECORDED into a graph has packed nothing yet: the pack stays marked as it was, and the
        #  next call outside the capture repacks if the parameters were written)
        if not torch.cuda.is_current_stream_capturing():
            self._stamp = [(p.data_ptr(), p._version) for p in params]

    def sync(self):
        """Repack if the parameters were written since the last pack (host-side check of their version counters)."""
        if self._stamp != [(p.data_ptr(), p._version) for p in self._params()]:
            self.refresh()

    def reserve(self, batch: int):
        """Scratch for batches up to ``batch`` (allocates; call it before a graph capture)."""
        if batch > self._capacity:
            nbytes = C.c_int64(0)
            _ffi.check(self.lib.ippm_actor_scratch_bytes(int(batch), C.addressof(nbytes)), "ippm_actor_scratch_bytes")
            if self.scratch is None or nbytes.value > self.scratch.numel():
                self.scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
            self._capacity = int(batch)

    def forward(self, obs: torch.Tensor, eps=0.0, logits: bool = False):
        """obs float32 [B,11,11,7] -> (probs [B,A], logits [B,A] or None).  ``eps``: a float, or a 0-dim float32 device tensor that
        the kernel reads (what a recorded graph needs)."""
        if obs.dim() == 3:
            obs = obs.unsqueeze(0)
        if obs.dtype != torch.float32 or tuple(obs.shape[1:]) != (_ffi.FEAT, _ffi.FEAT, _ffi.ACTOR_PLANES) or obs.device != self.device:
            raise _ffi.IppmError(f"NativeActor: needs float32 observations [B,11,11,7] on {self.device}, got {tuple(obs.shape)} {obs.dtype}")
        self.sync()
        obs = obs.contiguous()
        B = obs.shape[0]
        self.reserve(B)
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
