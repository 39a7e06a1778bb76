"""Child process of tests/test_hip_replay.py: whole training rounds with ``buffer="native"`` beside the same rounds with ``buffer="torch"``,
with the convolution library in DETERMINISTIC mode; writes SHA-256 digests of both nets' parameters as JSON to ``sys.argv[1]``:

  "defaults"    two rounds of a buffer="torch" and a buffer="native" trainer from one seed, every other switch at its default;
  "all_six_on"  the same with actor_inference, critic_inference and adam "native" and head_update, conv2_update, trunk_update "bf16";
  "recorded"    graphs=True, adam="native", head_update="bf16", buffer="native": one round launch by launch twice (the premise: two eager
                rounds agree) and once replayed from hipGraphs, all three from identical training state.

Why a process of its own: as tests/adam_recorded_rounds.py -- the library's deterministic mode depends on environment variables that the
library reads once per process, so they are set here before anything is imported."""
import hashlib
import json
import os
import sys

for _v in ("FWD", "BWD", "WRW"):
    os.environ[f"MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_{_v}"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("tests", "oracle", "ipp-marl_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import torch  # noqa: E402

torch.backends.cudnn.deterministic = True

SIX_ON = dict(actor_inference="native", critic_inference="native", adam="native", head_update="bf16", conv2_update="bf16",
              trunk_update="bf16")


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def two_rounds(T, **switches):
    """-> {net: (flat parameters after two rounds with buffer="torch", with buffer="native")}, and the parameters before."""
    after, before = {}, {}
    for mode in ("torch", "native"):
        tr = T._trainer(seed=13, buffer=mode, **switches)
        before = {net: T._flat(getattr(tr, net)).clone() for net in ("critic", "actor")}
        for r in range(2):
            torch.manual_seed(50 + r)
            assert tr.rollout("train")["faults"] == 0
            tr.update()
        assert mode == "torch" or int(tr._replay.bad) == 0
        after[mode] = {net: T._flat(getattr(tr, net)).clone() for net in ("critic", "actor")}
    return {net: (after["torch"][net], after["native"][net]) for net in ("critic", "actor")}, before


def recorded_round(T):
    """tests/test_hip_adam_trainer._run_recorded_rounds with the native buffer in all three trainers."""
    eager, again, rec = (T._trainer(seed=11, graphs=True, head_update="bf16", adam="native", buffer="native") for _ in range(3))
    for tr in (eager, again, rec):       # first round launch by launch (kernel selection, allocator, the replay's output sets)
        torch.manual_seed(12)
        tr.rollout("train")
        tr.update()
    T._copy_training_state(eager, again)
    T._copy_training_state(eager, rec)
    rec.capture_graphs()
    before = {net: T._flat(getattr(eager, net)).clone() for net in ("critic", "actor")}
    for tr in (eager, again, rec):
        torch.manual_seed(20)
        assert tr.rollout("train")["faults"] == 0
        tr.update()
    assert rec._update_graph is not None and again._update_graph is None
    bad = sum(int(tr._replay.bad) for tr in (eager, again, rec))
    return {net: tuple(T._flat(getattr(tr, net)).clone() for tr in (eager, again, rec)) for net in ("critic", "actor")}, before, bad


def summary(nets, before):
    out = {}
    for net, ts in nets.items():
        last = ts[-1]
        out[net] = {"digests": [digest(t) for t in ts], "numel": int(ts[0].numel()), "finite": bool(all(torch.isfinite(t).all() for t in ts)),
                    "differ": int((ts[0] != last).sum()), "premise_differ": int((ts[0] != ts[1]).sum()) if len(ts) == 3 else 0,
                    "moved": float((ts[0] - before[net]).abs().max())}
    return out


def main():
    import test_hip_adam_trainer as T
    for v in T.ALL_ENV + ("IPPMARL_BUFFER",):
        os.environ.pop(v, None)
    result = {}
    nets, before = two_rounds(T)
    result["defaults"] = summary(nets, before)
    nets, before = two_rounds(T, **SIX_ON)
    result["all_six_on"] = summary(nets, before)
    nets, before, bad = recorded_round(T)
    result["recorded"] = summary(nets, before)
    result["recorded_bad_indices"] = bad
    with open(sys.argv[1], "w") as f:
        json.dump(result, f)


if __name__ == "__main__":
    main()
