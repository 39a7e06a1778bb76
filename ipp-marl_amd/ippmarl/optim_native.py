"""Opt-in native Adam: libippmarl's one-launch optimizer step (csrc/optim.hip, ippm_adam_step) instead of ``torch.optim.Adam``, for the
learners of the COMA update.  One launch steps every managed tensor, clears its gradient and -- with a ``NativeNet`` attached -- rewrites
that net's bf16 inference pack from the new parameters.  The same kernel and the same bits launch by launch and replayed from a graph: the
step counter and the two bias-correction powers live in the state blob and advance inside the launch.

Arithmetic contract (include/ippmarl.h): Adam as the reference configures it (actor/learner.py:32,
critic/learner.py:48), every float32 operation rounded on its own; a contract of this project, not a promise to match a PyTorch build's bits.

``adam`` / ``IPPMARL_ADAM`` select the optimizer of the learners: "torch" (default) or "native".  GPU only: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional

import torch

from . import _ffi, switches
from .native_net import MODES, NativeNet, _LAYERS  # noqa: F401

ENV_VAR = switches.TABLE["adam"].env_var
ZERO_GRAD = 1           # IPPM_ADAM_ZERO_GRAD
MAX_TENSORS = 16        # IPPM_ADAM_MAX_TENSORS
COUNTER_BYTES = 64      # the counters block in front of the moments (the layout is documented in include/ippmarl.h)


def resolve_mode(adam: Optional[str] = None) -> str:
    """The learners' optimizer: the argument, else the environment variable, else "torch"; anything but "torch" / "native" raises."""
    return switches.resolve("adam", adam)


def used_parameters(module):
    """The ten tensors of a convnet that the network uses, in ``native_net._LAYERS`` order (``fc2`` never has a gradient)."""
    out = []
    for name in _LAYERS:
        layer = getattr(module, name)
        out += [layer.weight, layer.bias]
    return out


def _bump_versions(params):
    """The kernel wrote the parameters behind autograd's back: advance their version counters, so that everything that stamps them
    (native_net.NativeNet.sync) sees the write.  ``torch.autograd.graph.increment_version`` where this build has it (no launch); else an
    in-place operation on an empty slice of the parameter, which shares its counter and launches nothing."""
    inc = getattr(torch.autograd.graph, "increment_version", None)
    for p in params:
        if inc is not None:
            inc(p)
        else:
            with torch.no_grad():
                p.view(-1)[0:0].zero_()


def powers(beta: float, steps: int) -> float:
    """beta^steps as the kernel accumulates it: ``steps`` double multiplications, no pow."""
    x = 1.0
    for _ in range(int(steps)):
        x *= beta
    return x


class NativeAdam:
    """``torch.optim.Adam(params, lr)`` (defaults: no weight decay, no amsgrad) through ippm_adam_step, with the surface of a
    ``torch.optim.Optimizer`` where the trainer and the tests touch it.

    ``params``: what ``param_groups[0]["params"]`` lists, in the order given.  ``managed`` (default: all of them) selects the tensors that
    are stepped, at most 16: contiguous float32 tensors on one GPU.  ``state[p]`` exists for managed parameters only and holds VIEWS into
    the state blob: ``exp_avg``, ``exp_avg_sq``, and -- shared by all of them -- the 0-dim counters ``step`` (int64), ``beta1_power`` and
    ``beta2_power`` (float64: beta^step as the kernel accumulated it), so copying one optimizer's state entries onto another's carries
    everything a step reads.

    The gradient rule: ``step()`` clears every managed gradient in the launch that read it, and ``zero_grad()`` launches nothing when the
    previous call on this object was its own ``step()``.  So between a ``step()`` and the next ``zero_grad()`` nothing but this optimizer
    may write the gradients (in the trainer the all-reduce sits between backward and step); ``zero_grad(force=True)`` always fills."""

    def __init__(self, params: Iterable[torch.Tensor], lr: float, betas=(0.9, 0.999), eps: float = 1e-8, managed=None):
        params = list(params)
        managed = params if managed is None else list(managed)
        if not managed or len(managed) > MAX_TENSORS:
            raise _ffi.IppmError(f"NativeAdam: steps 1 to {MAX_TENSORS} tensors, got {len(managed)}")
        for p in managed:
            if not any(p is q for q in params):
                raise _ffi.IppmError("NativeAdam: a managed tensor is not among the parameters")
            if not p.is_cuda:
                raise _ffi.IppmError("NativeAdam: the native Adam step runs on the GPU only (there is no CPU fallback)")
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != managed[0].device:
                raise _ffi.IppmError("NativeAdam: the parameters must be contiguous float32 tensors on one device")
        self.lib = _ffi.load_library()
        self.device = managed[0].device
        self.managed = managed
        self.defaults = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps))
        self.param_groups = [dict(self.defaults, params=params)]
        n = len(managed)
        self._numel = (C.c_int64 * n)(*[p.numel() for p in managed])
        nbytes = C.c_int64(0)
        _ffi.check(self.lib.ippm_adam_state_bytes(self._numel, n, C.addressof(nbytes)), "ippm_adam_state_bytes")
        self.blob = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        _ffi.check(self.lib.ippm_adam_init(self.blob.data_ptr(), self._numel, n, self._stream()), "ippm_adam_init")
        counters = self.blob[:COUNTER_BYTES]
        self._t = counters[0:8].view(torch.int64)[0]
        self._b1p, self._b2p = counters[8:24].view(torch.float64)[0], counters[8:24].view(torch.float64)[1]
        self.state = {}
        off = COUNTER_BYTES
        for p in managed:
            span = (p.numel() + 3) // 4 * 16
            m = self.blob[off:off + 4 * p.numel()].view(torch.float32).view(p.shape)
            v = self.blob[off + span:off + span + 4 * p.numel()].view(torch.float32).view(p.shape)
            self.state[p] = {"step": self._t, "exp_avg": m, "exp_avg_sq": v, "beta1_power": self._b1p, "beta2_power": self._b2p}
            off += 2 * span
        assert off == nbytes.value
        self._p_ptrs = (C.c_void_p * n)(*[p.data_ptr() for p in managed])
        self._g_ptrs = (C.c_void_p * n)()
        self._pack = None
        self._stepped_last = False

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- the pack -------------------------------------------------------------------------------------------------------------------------
    def attach_pack(self, native_net: Optional[NativeNet]):
        """From now on ``step()`` hands ``native_net``'s packed blob and planes to the kernel, which rewrites every byte of the pack from
        the stepped parameters (``None`` detaches).  The managed tensors must be that net's ten parameters, in its order."""
        if native_net is not None:
            theirs = native_net._params()
            if len(theirs) != len(self.managed) or any(a is not b for a, b in zip(theirs, self.managed)):
                raise _ffi.IppmError("NativeAdam.attach_pack: the managed tensors are not that net's ten parameters in native_net._LAYERS order")
        self._pack = native_net

    # ---- the optimizer's surface ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self):
        group = self.param_groups[0]
        for i, p in enumerate(self.managed):
            g = p.grad
            if g is None:
                raise _ffi.IppmError("NativeAdam.step: a managed parameter has no gradient")
            if g.dtype != torch.float32 or not g.is_contiguous() or g.device != self.device:
                raise _ffi.IppmError("NativeAdam.step: gradients must be contiguous float32 tensors on the parameters' device")
            self._g_ptrs[i] = g.data_ptr()          # (read at call time: GradAllReducer.attach replaces the gradients by views)
            self._p_ptrs[i] = p.data_ptr()
        net = self._pack
        _ffi.check(self.lib.ippm_adam_step(self.blob.data_ptr(), self._p_ptrs, self._g_ptrs, self._numel, len(self.managed), group["lr"],
                                           group["betas"][0], group["betas"][1], group["eps"], ZERO_GRAD,
                                           net.PLANES if net is not None else 0, net.n_actions if net is not None else 0,
                                           net.packed.data_ptr() if net is not None else None, self._stream()), "ippm_adam_step")
        self._stepped_last = True
        if not torch.cuda.is_current_stream_capturing():
            # (a launch that is only recorded has written nothing yet: counters and stamps stay, as in NativeNet.refresh)
            _bump_versions(self.managed)
            if net is not None:
                net._stamp = [(p.data_ptr(), p._version) for p in net._params()]

    def zero_grad(self, set_to_none: bool = False, force: bool = False):
        """Clears the managed gradients in place -- and launches nothing when the previous call on this object was ``step()``, which has
        cleared them already (see the class's gradient rule); ``force=True`` always fills.  ``set_to_none=True`` drops them instead."""
        stepped, self._stepped_last = self._stepped_last, False
        if set_to_none:
            for p in self.managed:
                p.grad = None
            return
        if stepped and not force:
            return
        grads = [p.grad for p in self.managed if p.grad is not None]
        if grads:
            torch._foreach_zero_(grads)

    def steps_taken(self) -> int:
        return int(self._t.item())

    def state_dict(self):
        """``torch.optim.Adam``'s format: the moments cloned, ``step`` read back from the device (synchronises)."""
        params = self.param_groups[0]["params"]
        t = self.steps_taken()
        state = {}
        for i, p in enumerate(params):
            if p in self.state:
                state[i] = {"step": torch.tensor(float(t)), "exp_avg": self.state[p]["exp_avg"].clone(),
                            "exp_avg_sq": self.state[p]["exp_avg_sq"].clone()}
        group = dict(torch.optim.Adam([torch.zeros(1)], lr=self.param_groups[0]["lr"], betas=self.param_groups[0]["betas"],
                                      eps=self.param_groups[0]["eps"]).param_groups[0])
        group["params"] = list(range(len(params)))
        return {"state": state, "param_groups": [group]}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Accepts a state dict of this class or of ``torch.optim.Adam`` over the same parameter list: moments copied, the counter set to
        ``step`` and the powers recomputed from it by repeated double multiplication.  Either every managed parameter has an entry, or
        none has (an optimizer that never stepped: the state is reset)."""
        groups = state_dict["param_groups"]
        params = self.param_groups[0]["params"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(params):
            raise ValueError("NativeAdam.load_state_dict: one parameter group over the same parameter list is needed")
        group = groups[0]
        if group.get("weight_decay", 0) or group.get("amsgrad", False) or group.get("maximize", False):
            raise ValueError("NativeAdam.load_state_dict: weight decay, amsgrad and maximize are not part of the native step")
        by_param = {id(params[pos]): state_dict["state"].get(key) for pos, key in enumerate(group["params"])}
        entries = [by_param.get(id(p)) for p in self.managed]
        extra = [k for pos, k in enumerate(group["params"]) if k in state_dict["state"] and not any(params[pos] is p for p in self.managed)]
        if extra:
            raise ValueError("NativeAdam.load_state_dict: the state dict holds moments of a parameter that is not managed")
        present = [e for e in entries if e is not None]
        if present and len(present) != len(entries):
            raise ValueError("NativeAdam.load_state_dict: the state dict steps only some of the managed parameters")
        steps = {int(float(e["step"])) for e in present} or {0}
        if len(steps) != 1:
            raise ValueError("NativeAdam.load_state_dict: the parameters' step counts differ")
        t = steps.pop()
        for k in ("lr", "betas", "eps"):
            if k in group:
                self.param_groups[0][k] = tuple(float(b) for b in group[k]) if k == "betas" else float(group[k])
        b1, b2 = self.param_groups[0]["betas"]
        for p, e in zip(self.managed, entries):
            for k in ("exp_avg", "exp_avg_sq"):
                if e is None:
                    self.state[p][k].zero_()
                else:
                    self.state[p][k].copy_(e[k].to(self.device, torch.float32))
        self._t.fill_(t)
        self._b1p.fill_(powers(b1, t))
        self._b2p.fill_(powers(b2, t))
        self._stepped_last = False
