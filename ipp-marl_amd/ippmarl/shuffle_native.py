"""Opt-in keyed minibatch shuffle of ``COMATrainer``: libippmarl's ``ippm_minibatch_permutation`` (csrc/shuffle.hip) instead of
``torch.randperm`` for the minibatch order of ``update()``.  The permutation of (round, data_pass) is a pure function of the trainer's
``philox_seed`` -- cycle-walking over a six-round Feistel network whose round function is Philox (include/ippmarl.h states it,
tests/shuffle_ref.py restates it in NumPy) -- so the one random stream of a training run that lived in the device generator's hidden state
is keyed like the others: two runs from the same weights draw the same minibatches, a replayed round draws what the eager round draws, and
a run that is stopped and resumed (``COMATrainer.save_state``) has no generator state to carry.

Under mixed team sizes the same launch maps the rank among the flying transitions to its buffer row (``valid_transitions(W)[perm]``
without the ``nonzero()``).  ``round`` is the trainer's ``train_step`` on entry to ``update()``; in a recorded round the launches read it
from a device counter that the graph advances at its end.

All ranks of a data-parallel run use the SAME permutation over their own rows: the key holds no rank (the ranks' rows differ, their
minibatch positions do not).

``shuffle`` / ``IPPMARL_SHUFFLE`` select the implementation: "torch" (default) or "native".  GPU only: there is no CPU fallback."""
from __future__ import annotations

from typing import Optional

import torch

from . import _ffi, switches

ENV_VAR, MODES = switches.TABLE["shuffle"][:2]
MAX_PASSES = 65536      # data_pass is the 16-bit stage field of the Philox stream word


def resolve_mode(shuffle: Optional[str] = None) -> str:
    """The trainer's minibatch shuffle: the argument, else the environment variable, else "torch"; anything but "torch" / "native" raises."""
    return switches.resolve("shuffle", shuffle)


class NativeShuffle:
    """The native side of a trainer's minibatch order.  It owns the index buffer (int64 [data_passes, capacity]: one row per data pass, at
    fixed addresses, which is what a recorded round needs), the device round counter (int64 [1]) and, for mixed team sizes, the exclusive
    prefix sums of the envs' flying agents (int32 [n_envs + 1]).

    ``n_active`` (integers [n_envs], or None: every agent flies): the team sizes; then ``n`` of ``permutation`` counts flying transitions
    and the indices written are rows of buffers in [blocks, n_envs, n_agents] order."""

    def __init__(self, seed: int, data_passes: int, capacity: int, device, n_active: Optional[torch.Tensor] = None, n_envs: int = 0,
                 n_agents: int = 0):
        self.lib = _ffi.load_library()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _ffi.IppmError("NativeShuffle: the native minibatch shuffle runs on the GPU only (there is no CPU fallback)")
        if not 1 <= int(data_passes) <= MAX_PASSES or not 1 <= int(capacity) < 2 ** 31:
            raise _ffi.IppmError(f"NativeShuffle: data_passes must be in [1, {MAX_PASSES}] and capacity in [1, 2^31), got {data_passes}, {capacity}")
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.data_passes, self.capacity = int(data_passes), int(capacity)
        self.idx = torch.empty(self.data_passes, self.capacity, dtype=torch.int64, device=self.device)
        self.round_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.host_round = 0      # what the device counter holds as far as the host knows (the owner of a recorded round counts its replays)
        self.prefix, self.flying, self.n_envs, self.n_agents = None, 0, 0, 0
        if n_active is not None:
            sizes = [int(v) for v in n_active.reshape(-1).tolist()]
            if len(sizes) != int(n_envs) or int(n_agents) < 1 or any(not 0 <= s <= int(n_agents) for s in sizes) or sum(sizes) < 1:
                raise _ffi.IppmError(f"NativeShuffle: n_active must hold {n_envs} team sizes in [0, {n_agents}], one of them positive")
            prefix = [0]
            for s in sizes:
                prefix.append(prefix[-1] + s)
            self.prefix = torch.tensor(prefix, dtype=torch.int32, device=self.device)
            self.flying, self.n_envs, self.n_agents = prefix[-1], int(n_envs), int(n_agents)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def permutation(self, data_pass: int, n: int, round: Optional[int] = None) -> torch.Tensor:
        """One launch on the current stream: the minibatch order of ``data_pass`` over ``n`` transitions (flying ones under team sizes, a
        multiple of their number per block) -> int64 [n], a view of this object's row ``data_pass`` (overwritten by the next call for that
        pass).  ``round``: the training round by value; None reads the device counter in the kernel (the recorded form)."""
        n = int(n)
        if not 0 <= int(data_pass) < self.data_passes or not 1 <= n <= self.capacity:
            raise _ffi.IppmError(f"NativeShuffle.permutation: data_pass must be in [0, {self.data_passes}) and n in [1, {self.capacity}], "
                                 f"got {data_pass}, {n}")
        if self.prefix is not None and n % self.flying:
            raise _ffi.IppmError(f"NativeShuffle.permutation: n = {n} is not a multiple of the {self.flying} flying agents of a block")
        out = self.idx[int(data_pass), :n]
        _ffi.check(self.lib.ippm_minibatch_permutation(self.seed, 0 if round is None else int(round),
                                                       _ffi.ptr(self.round_dev) if round is None else None, int(data_pass), n,
                                                       _ffi.ptr(self.prefix), self.n_envs, self.n_agents, _ffi.ptr(out), self._stream()),
                   "ippm_minibatch_permutation")
        return out

    def advance(self):
        """The device counter one round on: one launch on the current stream (the last node of a recorded round)."""
        self.round_dev.add_(1)

    def set_round(self, round: int):
        """The device counter as the host counts (after an eager round, after a load)."""
        self.round_dev.fill_(int(round))
        self.host_round = int(round)

    def round(self) -> int:
        """The device counter (synchronises)."""
        return int(self.round_dev.item())
