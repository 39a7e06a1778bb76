"""Opt-in native replay buffer of ``COMATrainer``: libippmarl's three replay launches (csrc/replay.hip) instead of the tensor operations
that move a round's data around -- ``ippm_replay_store`` for a rollout step's transition and the return accumulators (five ``copy_`` and
three ``+=``), ``ippm_td_lambda_buffer`` for the TD(lambda) targets straight from buffer order (the permutes around ``ippm_td_lambda``),
``ippm_replay_gather`` for a minibatch of all five training arrays (six index kernels per minibatch pair).

Nothing is computed differently: the copies move bytes, every accumulator takes one float32 add per step, and the TD kernel runs K8's own
per-(chain, t) code at other strides -- a round with ``buffer="native"`` leaves the bits that ``buffer="torch"`` leaves.

``buffer`` / ``IPPMARL_BUFFER`` select the implementation: "torch" (default) or "native".  GPU only: there is no CPU fallback."""
from __future__ import annotations

from typing import Optional

import torch

from . import _ffi, switches

ENV_VAR, MODES = switches.TABLE["buffer"][:2]


def resolve_mode(buffer: Optional[str] = None) -> str:
    """The trainer's replay buffer: the argument, else the environment variable, else "torch"; anything but "torch" / "native" raises."""
    return switches.resolve("buffer", buffer)


class NativeReplay:
    """The native side of a trainer's replay buffer.  It owns no transition storage: ``buffers`` are the trainer's ``buf_obs``, ``buf_state``,
    ``buf_action``, ``buf_mask``, ``buf_reward`` ([W,T,E,N,...]; the reward [W,T,E], or [W,T,E,N] for DeepQ) and ``returns`` its ``ret``,
    ``abs_ret``, ``team_ret`` ([E]) -- the same tensors whoever writes them.  It owns the TD targets of the last ``td_targets`` call and two
    fixed sets of minibatch outputs (slots 0 and 1), sized on first use and reused afterwards: fixed addresses are what a recorded graph
    needs.

    ``last_agent`` (integers [E], DeepQ only): the agent whose reward an env's episode return sums."""

    def __init__(self, ctx: _ffi.Context, buffers, returns, batch_number: int, last_agent: Optional[torch.Tensor] = None):
        self.ctx, self.lib = ctx, ctx.lib
        self.obs, self.state, self.action, self.mask, self.reward = buffers
        self.ret, self.abs_ret, self.team_ret = returns
        self.device = self.obs.device
        if self.device.type != "cuda":
            raise _ffi.IppmError("NativeReplay: the native replay buffer runs on the GPU only (there is no CPU fallback)")
        self.W, self.T, self.E, self.N = (int(v) for v in self.obs.shape[:4])
        self.A = int(self.mask.shape[-1])
        self.deepq = self.reward.dim() == 4
        lead = (self.W, self.T, self.E, self.N)
        want = {"obs": (self.obs, torch.float32, lead + (11, 11, 7)), "state": (self.state, torch.float32, lead + (11, 11, 12)),
                "action": (self.action, torch.int32, lead), "mask": (self.mask, torch.uint8, lead + (self.A,)),
                "reward": (self.reward, torch.float32, lead if self.deepq else lead[:3])}
        for name, (buf, dtype, shape) in want.items():
            if buf.dtype != dtype or tuple(buf.shape) != shape or not buf.is_contiguous() or buf.device != self.device:
                raise _ffi.IppmError(f"NativeReplay: buf_{name} must be a contiguous {dtype} tensor {shape} on {self.device}, "
                                     f"got {buf.dtype} {tuple(buf.shape)}")
        for name, acc in zip(("ret", "abs_ret", "team_ret"), returns):
            if acc.dtype != torch.float32 or tuple(acc.shape) != (self.E,) or not acc.is_contiguous() or acc.device != self.device:
                raise _ffi.IppmError(f"NativeReplay: {name} must be a contiguous float32 tensor ({self.E},) on {self.device}")
        if self.deepq != (last_agent is not None):
            raise _ffi.IppmError("NativeReplay: per-agent rewards (a [W,T,E,N] reward buffer) and last_agent go together")
        self.last_agent = None if last_agent is None else last_agent.reshape(self.E).to(torch.int32).contiguous()
        self.batch_number = int(batch_number)
        n = self.W * self.T * self.E * self.N
        self.td = torch.empty(n, device=self.device)       # TD(lambda) targets / discounted returns of the last td_targets(), buffer order
        self.dr = torch.empty(n, device=self.device)
        self.rows = 0                                      # rows of td / dr that the last td_targets() wrote
        self.bad = torch.zeros(1, dtype=torch.int32, device=self.device)    # minibatch indices outside the buffer, ever (must stay 0)
        self._slots = None

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # ------------------------------------------------------------------------------------------------
    def store(self, w: int, t: int, obs, state, action, mask, reward, agent_reward=None, store: bool = True):
        """One rollout step in one launch: the transition into slot (w, t) (``store``) and one float32 add on each return accumulator.
        ``reward`` [E,2]: the env's team reward; ``agent_reward`` [E,N,2]: the per-agent rewards of a DeepQ mission."""
        if self.deepq != (agent_reward is not None):
            raise _ffi.IppmError("NativeReplay.store: agent_reward goes with a per-agent reward buffer (DeepQ), and only with one")
        EN = self.E * self.N
        for name, x, dtype, numel in (("obs", obs, torch.float32, EN * 847), ("state", state, torch.float32, EN * 1452),
                                      ("action", action, torch.int32, EN), ("mask", mask, torch.uint8, EN * self.A),
                                      ("reward", reward, torch.float32, self.E * 2), ("agent_reward", agent_reward, torch.float32, EN * 2)):
            if x is not None and (x.dtype != dtype or x.numel() != numel or x.device != self.device):
                raise _ffi.IppmError(f"NativeReplay.store: {name} must hold {numel} {dtype} values on {self.device}, "
                                     f"got {x.dtype} {tuple(x.shape)}")
        p = _ffi.ptr
        _ffi.check(self.lib.ippm_replay_store(p(obs), p(state), p(action), p(mask), p(reward), p(agent_reward), p(self.last_agent),
                                              self.E, self.N, self.A, self.W, self.T, int(w), int(t), 1 if store else 0, p(self.obs),
                                              p(self.state), p(self.action), p(self.mask), p(self.reward), p(self.ret), p(self.abs_ret),
                                              p(self.team_ret), self._stream()), "ippm_replay_store")

    def td_targets(self, q_sel: torch.Tensor, W: int):
        """TD(lambda) targets and discounted returns of the first ``W`` waves from ``q_sel`` (float32, W*T*E*N values in buffer order), in
        one launch and without a transposed copy -> (td, dr), flat views in buffer order of tensors this object keeps (overwritten by the
        next call)."""
        n = W * self.T * self.E * self.N
        if not 1 <= W <= self.W or q_sel.numel() != n or q_sel.dtype != torch.float32 or q_sel.device != self.device:
            raise _ffi.IppmError(f"NativeReplay.td_targets: q_sel must hold {n} float32 values on {self.device} for {W} of {self.W} waves")
        self.ctx.call("ippm_td_lambda_buffer", _ffi.ptr(self.reward), 1 if self.deepq else 0, _ffi.ptr(q_sel), _ffi.ptr(self.td),
                      _ffi.ptr(self.dr), W, self.T, self.E, self.N, self._stream())
        self.rows = n
        return self.td[:n], self.dr[:n]

    def minibatch(self, idx: torch.Tensor, slot: int):
        """One launch gathers rows ``idx`` (int64 on the device) of the first ``rows`` transitions into output set ``slot`` (0 or 1)
        -> (states, obs, actions, masks, td): views of the slot's tensors, valid until the slot is gathered into again."""
        count = int(idx.numel())
        if self._slots is None:
            cap = max(1, (self.W * self.T * self.E * self.N) // self.batch_number)
            mk = lambda *shape, dtype=torch.float32: torch.empty(cap, *shape, dtype=dtype, device=self.device)  # noqa: E731
            self._slots = [(mk(11, 11, 12), mk(11, 11, 7), mk(dtype=torch.int32), mk(self.A, dtype=torch.uint8), mk()) for _ in range(2)]
        out = self._slots[slot]
        if idx.dtype != torch.int64 or idx.device != self.device or count > out[0].shape[0] or self.rows < 1:
            raise _ffi.IppmError(f"NativeReplay.minibatch: idx must be at most {out[0].shape[0]} int64 indices on {self.device}, drawn "
                                 "after td_targets()")
        idx = idx.contiguous()
        p = _ffi.ptr
        _ffi.check(self.lib.ippm_replay_gather(p(self.state), p(self.obs), p(self.action), p(self.mask), p(self.td), self.rows, p(idx), count,
                                               self.A, p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(out[4]), p(self.bad), self._stream()),
                   "ippm_replay_gather")
        return tuple(o[:count] for o in out)

    def gather_values(self, values: torch.Tensor, idx: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """``out[r] = values[idx[r]]`` for a float32 array in buffer order (the discounted returns of the native metrics): the gather launch
        with ``values`` in the TD targets' place and every other output left out.  ``out``: a caller-owned float32 tensor of idx.numel()."""
        count = int(idx.numel())
        if (idx.dtype != torch.int64 or idx.device != self.device or self.rows < 1 or values.dtype != torch.float32 or values.numel() < self.rows
                or out.dtype != torch.float32 or out.numel() != count or not out.is_contiguous()):
            raise _ffi.IppmError("NativeReplay.gather_values: float32 values in buffer order, int64 indices and a float32 output of their "
                                 "number are needed, after td_targets()")
        idx = idx.contiguous()
        p = _ffi.ptr
        _ffi.check(self.lib.ippm_replay_gather(None, None, None, None, p(values), self.rows, p(idx), count, self.A, None, None, None, None,
                                               p(out), p(self.bad), self._stream()), "ippm_replay_gather")
        return out
