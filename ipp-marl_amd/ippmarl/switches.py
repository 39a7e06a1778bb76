"""The opt-in switches of ``COMATrainer``, one row each: constructor argument -> (environment variable, modes, default, the noun its
error message uses).  Every switch resolves the same way: the argument, else the environment variable (empty counts as unset), else the
default; anything outside the modes raises ``ValueError``.  What a switch selects is described where it is implemented (the module
docstrings of rollout_native, metrics_native, replay_native, actor_native, critic_native, optim_native, shuffle_native, the comments
above the three ``*_update`` context managers of networks) and in INTEGRATION.md."""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Tuple


class Switch(NamedTuple):
    env_var: str
    modes: Tuple[str, ...]
    default: str
    noun: str


NATIVE = ("torch", "native")
BF16 = ("float32", "bf16")

# (the order is that of a saved trainer state's "switches")
TABLE = {
    "rollout_log": Switch("IPPMARL_ROLLOUT_LOG", NATIVE, "torch", "rollout_log"),
    "metrics": Switch("IPPMARL_METRICS", NATIVE, "torch", "metrics"),
    "buffer": Switch("IPPMARL_BUFFER", NATIVE, "torch", "buffer"),
    "actor_inference": Switch("IPPMARL_ACTOR_INFERENCE", NATIVE, "torch", "actor inference"),
    "critic_inference": Switch("IPPMARL_CRITIC_INFERENCE", NATIVE, "torch", "critic inference"),
    "adam": Switch("IPPMARL_ADAM", NATIVE, "torch", "adam"),
    "head_update": Switch("IPPMARL_HEAD_UPDATE", BF16, "float32", "head update"),
    "conv2_update": Switch("IPPMARL_CONV2_UPDATE", BF16, "float32", "conv2 update"),
    "trunk_update": Switch("IPPMARL_TRUNK_UPDATE", BF16, "float32", "trunk update"),
    "shuffle": Switch("IPPMARL_SHUFFLE", NATIVE, "torch", "shuffle"),
}


def resolve(name: str, value: Optional[str] = None) -> str:
    """The mode of switch ``name``: ``value``, else its environment variable, else its default; anything outside its modes raises."""
    s = TABLE[name]
    mode = value if value is not None else os.environ.get(s.env_var, "") or s.default
    if mode not in s.modes:
        raise ValueError(f"{s.noun} must be one of {s.modes}, got {mode!r}")
    return mode
