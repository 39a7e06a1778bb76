"""Opt-in native training metrics: the 32 per-training-step scalars of ``ippmarl.metrics`` reduced on the device by libippmarl
(csrc/metrics.hip) from the arrays the learners have anyway, instead of per-minibatch records kept for ~45 ``float(...)`` reads.

With ``metrics="native"`` a round run with ``update(diagnostics=True)`` is computed exactly as without diagnostics: the learners' ``collect``
stays off, the native head, gathers, critic forward and Adam run as configured, and the numbers describe that configured path.  The learners
hand their arrays to a ``NativeMetrics``; the launches record into the update graph, and ``last_diagnostics`` is filled from ONE
``out.tolist()``.

Arithmetic contract (include/ippmarl.h): float64 on the float32 inputs, fixed reduction trees, Chan-merged moments, no
atomics -- the same bits whatever the blob held, in whatever order the slots were called.

``metrics`` / ``IPPMARL_METRICS`` select the path: "torch" (default) or "native".  GPU only: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from . import _ffi, switches
from .metrics import LAYER_TAGS

ENV_VAR, MODES = switches.TABLE["metrics"][:2]
SCALARS = 32        # IPPM_METRICS_SCALARS
CHUNK = 256         # IPPM_METRICS_CHUNK

# the keys of metrics.critic_metrics followed by metrics.actor_metrics, in their order: out[i] of ippm_metrics_finalize is KEYS[i]
KEYS = (("Critic/Loss", "Critic/TD-Targets mean", "Critic/TD-Targets std", "Critic/Q chosen mean", "Critic/Q values mean",
         "Critic/Q values min", "Critic/Q values std", "Critic/Explained variance", "Critic/Discounted returns mean",
         "Critic/Discounted_returns std", "Critic/Abs deviation Q-value <-> Return mean", "Critic/Abs deviation Q-value <-> Return std",
         "Critic/Log probs according to critic")
        + tuple(f"Parameters/Critic/{tag} gradients" for tag in LAYER_TAGS)
        + ("Actor/Loss", "Actor/Advantages mean", "Actor/Advantages std", "Actor/Log probs chosen mean", "Actor/Policy entropy",
           "Actor/KL divergence policy", "Actor/Hidden state entropy")
        + tuple(f"Parameters/Actor/{tag} gradients" for tag in LAYER_TAGS))
assert len(KEYS) == SCALARS


def resolve_mode(metrics: Optional[str] = None) -> str:
    """The trainer's diagnostics path: the argument, else the environment variable, else "torch"; anything but "torch" / "native" raises."""
    return switches.resolve("metrics", metrics)


def _f32(x: torch.Tensor, numel: int, what: str, device) -> torch.Tensor:
    if x.device != device or x.numel() != numel:
        raise _ffi.IppmError(f"NativeMetrics: {what} must hold {numel} values on {device}, got {tuple(x.shape)} on {x.device}")
    return x.detach().reshape(-1).float().contiguous()


class NativeMetrics:
    """The accumulator of one round of ``n_minibatches`` minibatches of ``batch`` rows and ``n_actions`` actions on ``device``.  It owns the
    blob of partial results, the [n_minibatches, batch, n_actions] buffer of pre-step probabilities (``probs_old``: the actor's loss kernel
    may write a slot's rows directly), a [n_minibatches, batch] buffer for the gathered discounted returns (``disc``) and ``out`` (float64
    [32]).  All addresses are fixed for the object's life: what a recorded graph needs.  Nothing here synchronises but ``read()``."""

    def __init__(self, n_minibatches: int, batch: int, n_actions: int, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _ffi.IppmError("NativeMetrics: the native metrics run on the GPU only (there is no CPU fallback)")
        self.lib = _ffi.load_library()
        self.nb, self.B, self.A = int(n_minibatches), int(batch), int(n_actions)
        nbytes = C.c_int64(0)
        _ffi.check(self.lib.ippm_metrics_bytes(self.nb, self.B, self.A, C.addressof(nbytes)), "ippm_metrics_bytes")
        self.blob = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        self.probs_old = torch.empty(self.nb, self.B, self.A, dtype=torch.float32, device=self.device)
        self.disc = torch.empty(self.nb, self.B, dtype=torch.float32, device=self.device)
        self.out = torch.zeros(SCALARS, dtype=torch.float64, device=self.device)
        self._numel = (C.c_int64 * 10)()
        self._ptrs = (C.c_void_p * 10)()

    def matches(self, n_minibatches: int, batch: int, n_actions: int) -> bool:
        return (self.nb, self.B, self.A) == (int(n_minibatches), int(batch), int(n_actions))

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def critic(self, slot: int, loss, q_chosen, td, disc, q_new, action):
        """Minibatch ``slot`` of the critic: loss (one value), q_chosen (pre-step), td, disc [B], q_new [B,A] (post-step), action [B]."""
        B, A, d = self.B, self.A, self.device
        loss, q_chosen, td, disc = _f32(loss, 1, "loss", d), _f32(q_chosen, B, "q_chosen", d), _f32(td, B, "td", d), _f32(disc, B, "disc", d)
        q_new = _f32(q_new, B * A, "q_new", d)
        a32 = action.reshape(-1).to(torch.int32).contiguous()
        _ffi.check(self.lib.ippm_metrics_critic(self.blob.data_ptr(), int(slot), self.nb, loss.data_ptr(), q_chosen.data_ptr(), td.data_ptr(),
                                                disc.data_ptr(), q_new.data_ptr(), a32.data_ptr(), B, A, self._stream()), "ippm_metrics_critic")

    def actor(self, slot: int, loss, adv, probs, action, hidden0):
        """Minibatch ``slot`` of the actor: loss, adv [B], probs [B,A] (epsilon-mixed, pre-step; copied into ``probs_old[slot]`` unless it
        IS that buffer's slice), action [B], hidden0 [256]."""
        B, A, d = self.B, self.A, self.device
        old = self.probs_old[slot]
        if probs.data_ptr() != old.data_ptr():
            old.copy_(probs.detach().reshape(B, A))
        loss, adv, hidden0 = _f32(loss, 1, "loss", d), _f32(adv, B, "adv", d), _f32(hidden0, 256, "hidden0", d)
        a32 = action.reshape(-1).to(torch.int32).contiguous()
        _ffi.check(self.lib.ippm_metrics_actor(self.blob.data_ptr(), int(slot), self.nb, loss.data_ptr(), adv.data_ptr(), old.data_ptr(),
                                               a32.data_ptr(), hidden0.data_ptr(), B, A, self._stream()), "ippm_metrics_actor")

    def actor_after(self, slot: int, probs_after):
        """The updated actor's probabilities on minibatch ``slot``: the KL figure's terms against ``probs_old[slot]``."""
        after = _f32(probs_after, self.B * self.A, "probs_after", self.device)
        _ffi.check(self.lib.ippm_metrics_actor_after(self.blob.data_ptr(), int(slot), self.nb, self.probs_old[slot].data_ptr(), after.data_ptr(),
                                                     self.B, self.A, self._stream()), "ippm_metrics_actor_after")

    def grad_l1(self, net: int, grads: Sequence[torch.Tensor]):
        """The L1 norms of a net's ten gradients (``net`` 0: critic, 1: actor), in optim_native.used_parameters order."""
        grads = list(grads)
        if len(grads) != 10:
            raise _ffi.IppmError(f"NativeMetrics.grad_l1: the ten gradients of a network are needed, got {len(grads)}")
        for i, g in enumerate(grads):
            if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.device != self.device:
                raise _ffi.IppmError("NativeMetrics.grad_l1: gradients must be contiguous float32 tensors on the metrics' device")
            self._ptrs[i], self._numel[i] = g.data_ptr(), g.numel()
        _ffi.check(self.lib.ippm_metrics_grad_l1(self.blob.data_ptr(), int(net), self._ptrs, self._numel, 10, self._stream()),
                   "ippm_metrics_grad_l1")

    def finalize(self):
        _ffi.check(self.lib.ippm_metrics_finalize(self.blob.data_ptr(), self.nb, self.B, self.A, self.out.data_ptr(), self._stream()),
                   "ippm_metrics_finalize")

    def read(self) -> Dict[str, float]:
        """The 32 scalars under the reference's names, in ``ippmarl.metrics``' order: one device-to-host read."""
        return dict(zip(KEYS, self.out.tolist()))
