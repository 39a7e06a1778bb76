"""Opt-in native rollout log: the twelve return / reward statistics of ``metrics.return_scalars`` and the action and altitude counts of
``COMAMission.add_to_tensorboard`` reduced on the device by libippmarl (csrc/rollout_log.hip), instead of three clones per rollout step,
five arrays moved to the host and ~20 host reductions per round.

With ``rollout_log="native"`` one small launch per rollout step writes that step's share of the log into a device blob; the launch is part
of ``COMATrainer._rollout_step``, so ``capture_graphs()`` records it into every step graph and a trainer that keeps the log replays its
recorded rollout.  One closing launch reduces the waves, and ``read()`` is ONE device-to-host copy.

Arithmetic contract (include/ippmarl.h): rewards kept as float32, returns by float32 adds in step order (the trainer's
own ``ret`` bit for bit), statistics in float64 with Chan-merged moments in a fixed tree, exact integer counts, no floating-point atomics --
the same bits whatever the blob held, in whatever order the steps were called.

``rollout_log`` / ``IPPMARL_ROLLOUT_LOG`` select the path: "torch" (default) or "native".  GPU only: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _ffi, switches

ENV_VAR, MODES = switches.TABLE["rollout_log"][:2]
SCALARS = 12        # IPPM_ROLLOUT_SCALARS
COUNTS = 65         # IPPM_ROLLOUT_COUNTS: [0,32) actions, [32,64) altitude levels, [64] entries counted in no bin
ROWS = 1024         # IPPM_ROLLOUT_ROWS: (env, agent) rows of one workgroup of the step launch

# the tag suffixes of metrics.return_scalars, in its order (the mode prefix is applied on read): out[i] of ippm_rollout_log_finalize is KEYS[i]
KEYS = tuple(f"{series}/{stat}" for series in ("Return/Episode", "Rewards/Episode", "Return/Relative(used)/Episode")
             for stat in ("mean", "std", "max", "min"))
assert len(KEYS) == SCALARS


def resolve_mode(rollout_log: Optional[str] = None) -> str:
    """The trainer's rollout-log path: the argument, else the environment variable, else "torch"; anything but "torch" / "native" raises."""
    return switches.resolve("rollout_log", rollout_log)


class NativeRolloutLog:
    """The log of up to ``n_waves`` waves of ``T`` steps of ``E`` envs of ``N`` agents with ``A`` actions and ``n_levels`` altitude levels
    ``min_altitude + k * spacing`` on ``device``.  It owns the blob and ONE 8-byte-element result buffer, of which ``out`` (float64 [12]) and
    ``counts`` (int64 [65]) are views.  All addresses are fixed for the object's life: what a recorded graph needs.  Nothing here
    synchronises but ``read()``."""

    def __init__(self, n_waves: int, T: int, E: int, N: int, A: int, min_altitude: int, spacing: int, n_levels: int, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _ffi.IppmError("NativeRolloutLog: the native rollout log runs on the GPU only (there is no CPU fallback)")
        self.lib = _ffi.load_library()
        self.W, self.T, self.E, self.N, self.A = int(n_waves), int(T), int(E), int(N), int(A)
        self.min_altitude, self.spacing, self.n_levels = int(min_altitude), int(spacing), int(n_levels)
        nbytes = C.c_int64(0)
        _ffi.check(self.lib.ippm_rollout_log_bytes(self.W, self.T, self.E, self.N, C.addressof(nbytes)), "ippm_rollout_log_bytes")
        self.blob = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        self.result = torch.zeros(SCALARS + COUNTS, dtype=torch.int64, device=self.device)
        self.out = self.result[:SCALARS].view(torch.float64)
        self.counts = self.result[SCALARS:]

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _i32(self, x: Optional[torch.Tensor], numel: int, what: str) -> int:
        if x is None:
            return 0
        if x.device != self.device or x.numel() != numel or x.dtype != torch.int32 or not x.is_contiguous():
            raise _ffi.IppmError(f"NativeRolloutLog: {what} must be {numel} contiguous int32 values on {self.device}")
        return x.data_ptr()

    def _f32(self, x: Optional[torch.Tensor], numel: int, what: str) -> int:
        if x is None:
            return 0
        if x.device != self.device or x.numel() != numel or x.dtype != torch.float32 or not x.is_contiguous():
            raise _ffi.IppmError(f"NativeRolloutLog: {what} must be {numel} contiguous float32 values on {self.device}")
        return x.data_ptr()

    def step(self, wave: int, t: int, reward, agent_reward, action, pos, n_active):
        """Step ``t`` of wave ``wave``: reward [E,2]; agent_reward None or [E,N,2] (DeepQ: the last flying agent's row replaces reward[e]);
        action int32 [E,N]; pos int32 [E,N,3]; n_active None or int32 [E].  The arrays are read where they are: no copy, one launch."""
        E, N = self.E, self.N
        _ffi.check(self.lib.ippm_rollout_log_step(
            self.blob.data_ptr(), int(wave), int(t), self.W, self.T, self._f32(reward, 2 * E, "reward"),
            self._f32(agent_reward, 2 * E * N, "agent_reward"), self._i32(action, E * N, "action"), self._i32(pos, 3 * E * N, "pos"),
            self._i32(n_active, E, "n_active"), E, N, self.A, self.min_altitude, self.spacing, self.n_levels, self._stream()),
            "ippm_rollout_log_step")

    def finalize(self, n_waves: int):
        """The closing launch over the first ``n_waves`` waves of the blob."""
        _ffi.check(self.lib.ippm_rollout_log_finalize(self.blob.data_ptr(), int(n_waves), self.T, self.E, self.N, self.out.data_ptr(),
                                                      self.counts.data_ptr(), self._stream()), "ippm_rollout_log_finalize")

    def read(self, mode: str) -> Tuple[Dict[str, float], List[int], Dict[int, int], int]:
        """(the 12 scalars under ``mode``-prefixed tags, the count of every action, {altitude in metres: count} of the levels that occur,
        the entries counted in no bin): one device-to-host read."""
        host = self.result.cpu()
        scalars = dict(zip((mode + k for k in KEYS), host[:SCALARS].view(torch.float64).tolist()))
        counts = host[SCALARS:].tolist()
        altitudes = {self.min_altitude + k * self.spacing: c for k, c in enumerate(counts[32:32 + self.n_levels]) if c}
        return scalars, counts[:self.A], altitudes, counts[64]
