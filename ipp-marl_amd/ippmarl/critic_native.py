"""Opt-in native inference of the critic: libippmarl's bf16 matrix-core forward (ippm_critic_forward) instead of the float32 PyTorch
module, for the two no-grad uses of a critic in the COMA round: the TD targets (the target critic over the whole buffer) and the
post-step Q of every critic minibatch.  Everything that takes gradients keeps the float32 module.

Numerical contract, the actor's: every layer's input and weights are bf16 (round to nearest even), products
accumulate in float32, the float32 bias is added to the accumulator, ReLU, one rounding to bf16 at the store; Q is float32.
Deterministic: a sample's Q is the same bits alone and at any position of any batch.  The log_softmax over the batch that
``CriticNetwork.forward`` also returns is a logged metric and is not computed here.

``critic_inference`` / ``IPPMARL_CRITIC_INFERENCE`` select the path: "torch" (default) or "native"."""
from __future__ import annotations

from typing import Optional

import torch

from . import _ffi, switches
from .native_net import MODES, NativeNet  # noqa: F401

ENV_VAR = switches.TABLE["critic_inference"].env_var


def resolve_mode(critic_inference: Optional[str] = None) -> str:
    """The critic's inference path: the argument, else the environment variable, else "torch"; anything but "torch" / "native" raises."""
    return switches.resolve("critic_inference", critic_inference)


class NativeCritic(NativeNet):
    """Holds the packed bf16 weights of ``critic_module`` and the forward's scratch on ``device`` (native_net.NativeNet: ``refresh()``,
    ``sync()``, ``reserve()`` and the rules that keep the pack current)."""

    PREFIX, WHO, WHAT, PLANES = "ippm_critic", "NativeCritic", "critic", _ffi.CRITIC_PLANES

    def forward(self, states: torch.Tensor, actions: Optional[torch.Tensor] = None, want_q: bool = True):
        """states float32 [B,11,11,12] -> (q [B,A] or None, q_sel [B] or None): ``q_sel[b] = q[b][actions[b]]`` when ``actions``
        (integers [B]) is given; ``want_q=False`` (with ``actions``) leaves the full table unwritten."""
        self.sync()
        return self._forward(states, actions, want_q)

    def after_step(self, states: torch.Tensor) -> torch.Tensor:
        """The learner's hook (CriticLearner.apply): repack from the parameters the optimizer has just stepped, then Q [B,A] of
        ``states`` on that pack.  Both launches are capturable; no version check is needed in between."""
        self.refresh()
        return self._forward(states, None, True)[0]

    def after_native_step(self, states: torch.Tensor) -> torch.Tensor:
        """``after_step`` behind a native Adam step that had this pack attached (optim_native.NativeAdam.attach_pack): the step's launch
        has rewritten the pack already, so Q [B,A] of ``states`` is the only launch."""
        return self._forward(states, None, True)[0]

    def _forward(self, states, actions, want_q):
        states = self._input(states)
        B = states.shape[0]
        if actions is None and not want_q:
            raise _ffi.IppmError("NativeCritic: nothing to compute (no actions and want_q=False)")
        q = torch.empty(B, self.n_actions, dtype=torch.float32, device=self.device) if want_q else None
        q_sel = act = None
        if actions is not None:
            if actions.device != self.device or actions.numel() != B or actions.is_floating_point():
                raise _ffi.IppmError(f"NativeCritic: actions must be {B} integers on {self.device}")
            act = actions.reshape(B).to(torch.int32).contiguous()     # (stays referenced until the launch is queued)
            q_sel = torch.empty(B, dtype=torch.float32, device=self.device)
        _ffi.check(self.lib.ippm_critic_forward(self.packed.data_ptr(), states.data_ptr(), B, self.n_actions, _ffi.ptr(act),
                                                self.scratch.data_ptr(), _ffi.ptr(q), _ffi.ptr(q_sel), self._stream()),
                   "ippm_critic_forward")
        return q, q_sel

    def __call__(self, states: torch.Tensor):
        return self.forward(states)[0]
