"""CPU checks of the ``buffer`` switch (ippmarl.replay_native, the trainer's signature) and of the three replay entry points' place in
the header and the binding."""
import inspect
import os
import re

import pytest

from configs import make_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ippm_replay_store", "ippm_td_lambda_buffer", "ippm_replay_gather")


def test_switch_parsing(monkeypatch):
    from ippmarl import replay_native
    monkeypatch.delenv(replay_native.ENV_VAR, raising=False)
    assert replay_native.ENV_VAR == "IPPMARL_BUFFER" and replay_native.MODES == ("torch", "native")
    assert replay_native.resolve_mode() == "torch" and replay_native.resolve_mode(None) == "torch"
    monkeypatch.setenv(replay_native.ENV_VAR, "native")
    assert replay_native.resolve_mode() == "native"
    assert replay_native.resolve_mode("torch") == "torch"                 # the argument wins over the environment
    monkeypatch.setenv(replay_native.ENV_VAR, "")
    assert replay_native.resolve_mode() == "torch"
    for bad in ("hip", "Native", "1"):
        with pytest.raises(ValueError, match="buffer"):
            replay_native.resolve_mode(bad)
        monkeypatch.setenv(replay_native.ENV_VAR, bad)
        with pytest.raises(ValueError, match="buffer"):
            replay_native.resolve_mode()
        assert replay_native.resolve_mode("native") == "native"


def test_trainer_rejects_an_unknown_mode_before_any_gpu_use(monkeypatch):
    """The trainer resolves ``buffer`` before it builds anything that needs the GPU: the env's constructor is never reached."""
    from ippmarl import replay_native, trainer
    built = []
    monkeypatch.setattr(trainer, "VecEnv", lambda *a, **k: built.append(1))
    monkeypatch.delenv(replay_native.ENV_VAR, raising=False)
    with pytest.raises(ValueError, match="buffer"):
        trainer.COMATrainer(make_params("small"), n_envs=1, buffer="hip")
    monkeypatch.setenv(replay_native.ENV_VAR, "both")
    with pytest.raises(ValueError, match="buffer"):
        trainer.COMATrainer(make_params("small"), n_envs=1)
    assert not built


def test_signature():
    from ippmarl.learners import ActorLearner, CriticLearner
    from ippmarl.trainer import COMATrainer
    sig = inspect.signature(COMATrainer.__init__)
    names = list(sig.parameters)
    assert sig.parameters["buffer"].default is None
    assert names[names.index("buffer") + 1] == "actor_inference"
    # the six older switches keep their places behind it
    assert names[names.index("buffer") + 1:] == ["actor_inference", "critic_inference", "adam", "head_update", "conv2_update", "trunk_update"]
    for cls in (CriticLearner, ActorLearner):                 # the learners never see the buffer
        assert "buffer" not in inspect.signature(cls.__init__).parameters


def test_header_declares_and_binding_binds_the_entry_points():
    from ippmarl import _ffi
    header = open(os.path.join(ROOT, "include", "ippmarl.h")).read()
    for name in ENTRY_POINTS:
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M)
        assert decl, f"{name} is not declared in include/ippmarl.h"
        args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
        assert args[-1] == "void* stream", (name, args[-1])                    # the header's convention: the stream comes last
        assert name in _ffi.PROTOTYPES, f"{name} is not bound in _ffi.PROTOTYPES"
        assert len(_ffi.PROTOTYPES[name]) == len(args), (name, len(_ffi.PROTOTYPES[name]), len(args))
        # pointers are bound as pointers, integers by their width
        for arg, bound in zip(args, _ffi.PROTOTYPES[name]):
            want = _ffi.P if "*" in arg else (_ffi.I64 if arg.startswith("int64_t") else _ffi.I32)
            assert bound is want, (name, arg, bound)


def test_native_replay_is_gpu_only():
    import torch
    from ippmarl import _ffi
    from ippmarl.replay_native import NativeReplay

    class Ctx:
        lib = None

    W, T, E, N, A = 1, 2, 1, 2, 6
    bufs = (torch.zeros(W, T, E, N, 11, 11, 7), torch.zeros(W, T, E, N, 11, 11, 12), torch.zeros(W, T, E, N, dtype=torch.int32),
            torch.zeros(W, T, E, N, A, dtype=torch.uint8), torch.zeros(W, T, E))
    with pytest.raises(_ffi.IppmError, match="GPU only"):
        NativeReplay(Ctx(), bufs, tuple(torch.zeros(E) for _ in range(3)), 2)
