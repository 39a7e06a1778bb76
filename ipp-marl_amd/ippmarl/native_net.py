"""What the native bf16 forwards of the two convnets share on the host (actor_native.NativeActor, critic_native.NativeCritic): the packed
weight blob of a module, the forward's scratch, and the rules that keep the pack current.

``refresh()`` repacks from the module's current parameters (one kernel, capturable).  ``sync()`` repacks when the parameters'
``(data_ptr, _version)`` stamps say that they were written since the last pack, so a ``load_state_dict`` or an eager optimizer step
cannot leave a stale pack behind; a replayed graph changes no counter, which is why the trainer records ``refresh()`` into its update
graph.  A repack that is only recorded during a capture does not count as a pack: ``COMATrainer.capture_graphs`` syncs before it
starts recording.  GPU only: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C

import torch

from . import _ffi

MODES = ("torch", "native")
_LAYERS = ("conv1", "conv2", "conv3", "fc1", "fc3")   # fc2 is never used by the network (networks._ConvTrunk)


class NativeNet:
    """Pack and scratch of ``module`` on ``device``.  A subclass names its C entry points (``PREFIX`` = "ippm_actor" / "ippm_critic"),
    the planes of its input and itself (``WHO``, ``WHAT``: for error messages) and adds the forward."""

    PREFIX = WHO = WHAT = ""
    PLANES = 0

    def __init__(self, module, device):
        self.module = module
        self.device = self._device(device)
        self.lib = _ffi.load_library()
        self.n_actions = int(module.fc3.out_features)
        nbytes = C.c_int64(0)
        self._check(self._fn("pack_bytes")(self.n_actions, C.addressof(nbytes)), "pack_bytes")
        self.packed = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        self.scratch = None
        self._capacity = 0
        self._stamp = None
        self.refresh()

    @classmethod
    def _device(cls, device) -> torch.device:
        device = torch.device(device)
        if device.type != "cuda":
            raise _ffi.IppmError(f"{cls.WHO}: the native {cls.WHAT} forward runs on the GPU only (there is no CPU fallback)")
        return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device

    def _fn(self, name: str):
        return getattr(self.lib, f"{self.PREFIX}_{name}")

    def _check(self, rc: int, name: str):
        _ffi.check(rc, f"{self.PREFIX}_{name}")

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
                raise _ffi.IppmError(f"{self.WHO}: the {self.WHAT}'s parameters must be contiguous float32 tensors on the {self.WHAT}'s device")
        self._check(self._fn("pack")(*[p.data_ptr() for p in params], self.n_actions, self.packed.data_ptr(), self._stream()), "pack")
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
            self._check(self._fn("scratch_bytes")(int(batch), C.addressof(nbytes)), "scratch_bytes")
            if self.scratch is None or nbytes.value > self.scratch.numel():
                self.scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
            self._capacity = int(batch)

    def _input(self, x: torch.Tensor) -> torch.Tensor:
        """The network input as the kernels read it: float32 [B,11,11,PLANES], contiguous, on the device; scratch reserved for B.
        (The caller decides whether the pack needs a ``sync()`` first.)"""
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if x.dtype != torch.float32 or tuple(x.shape[1:]) != (_ffi.FEAT, _ffi.FEAT, self.PLANES) or x.device != self.device:
            raise _ffi.IppmError(f"{self.WHO}: needs float32 inputs [B,11,11,{self.PLANES}] on {self.device}, got {tuple(x.shape)} {x.dtype}")
        x = x.contiguous()
        self.reserve(x.shape[0])
        return x
