"""GPU checks of ``metrics="native"`` above the kernels: the trainer's switch, a diagnostics round that keeps every native path, and -- in a
child process with deterministic convolutions (tests/metrics_recorded_rounds.py) -- the native scalars against the float64 restatement on
the torch metrics' own records, and a recorded round against an eager one.  The kernels themselves: tests/test_hip_metrics_native.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_hip_adam_trainer import ALL_ENV, _count_lib, _trainer

pytestmark = pytest.mark.gpu

SWITCHES = ALL_ENV + ("IPPMARL_BUFFER", "IPPMARL_METRICS")
ENTRY_POINTS = ("ippm_metrics_bytes", "ippm_metrics_critic", "ippm_metrics_actor", "ippm_metrics_actor_after", "ippm_metrics_grad_l1",
                "ippm_metrics_finalize")
REAL_GRADIENTS = (13, 14, 15, 16, 18, 26, 27, 28, 29, 31)          # conv1, conv2, conv3, fc1, fc3 of both nets (fc2 has none)


def test_switch_values(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    with pytest.raises(ValueError):
        _trainer(seed=6, n_envs=1, metrics="hip")
    monkeypatch.setenv("IPPMARL_METRICS", "native")
    tr = _trainer(seed=6, n_envs=1)
    assert tr.metrics == tr.critic_learner.metrics == tr.actor_learner.metrics == "native"


def test_default_round_never_touches_the_native_metrics(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    calls = {name: _count_lib(monkeypatch, name) for name in ENTRY_POINTS}
    tr = _trainer(seed=6, n_envs=1)
    assert tr.metrics == tr.critic_learner.metrics == tr.actor_learner.metrics == "torch"
    assert tr.rollout("train")["faults"] == 0
    tr.update()
    assert tr.rollout("train")["faults"] == 0
    stats = tr.update(diagnostics=True)
    assert np.isfinite(stats["critic_loss"]) and len(tr.last_diagnostics) == 32
    assert not any(calls.values()), {k: len(v) for k, v in calls.items()}
    assert tr._metrics is None


def test_diagnostics_round_keeps_every_native_path(monkeypatch):
    """All native switches on: a diagnostics round is computed as a plain one (native head in data pass 0, native gathers plus one gather
    of discounted returns per minibatch, native Adam), and the 32 scalars come back from one read."""
    from ippmarl import metrics_native
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    built = []
    real_init = torch.optim.Adam.__init__
    monkeypatch.setattr(torch.optim.Adam, "__init__", lambda self, *a, **k: (built.append(1), real_init(self, *a, **k))[1])
    tr = _trainer(seed=8, n_envs=2, metrics="native", adam="native", buffer="native", head_update="bf16", trunk_update="bf16",
                  actor_inference="native", critic_inference="native")
    nb, passes = tr.batch_number, tr.data_passes
    counts = {}
    for diag in (False, True):
        assert tr.rollout("train")["faults"] == 0
        heads = _count_lib(monkeypatch, "ippm_head_forward")
        gathers = _count_lib(monkeypatch, "ippm_replay_gather")
        finals = _count_lib(monkeypatch, "ippm_metrics_finalize")
        critics = _count_lib(monkeypatch, "ippm_metrics_critic")
        tr.last_diagnostics = None
        stats = tr.update(diagnostics=diag)
        torch.cuda.synchronize()
        assert np.isfinite(stats["critic_loss"]) and np.isfinite(stats["actor_loss"])
        counts[diag] = dict(heads=len(heads), gathers=len(gathers), finals=len(finals), critics=len(critics))
        assert not tr.critic_learner.collect and not tr.actor_learner.collect
    plain, diag = counts[False], counts[True]
    # the native head ran for both nets in every minibatch of every data pass, pass 0 included
    assert plain["heads"] == diag["heads"] == 2 * passes * nb, counts
    assert plain["gathers"] == passes * nb and diag["gathers"] == plain["gathers"] + nb, counts
    assert plain["finals"] == plain["critics"] == 0 and diag["finals"] == 1 and diag["critics"] == nb, counts
    assert not built                                                   # torch.optim.Adam was never built
    got = tr.last_diagnostics
    assert list(got) == list(metrics_native.KEYS)
    values = np.array(list(got.values()))
    print({k: v for k, v in got.items()})
    assert np.isfinite(values).all(), got
    assert (values[list(REAL_GRADIENTS)] > 0).all() and values[17] == 0.0 and values[30] == 0.0, got
    assert int(tr._replay.bad.item()) == 0


def test_native_against_torch_and_recorded_against_eager(tmp_path):
    """tests/metrics_recorded_rounds.py in a process of its own.  Metrics observe a round and never change it: both nets' parameters are
    bit-identical across metrics="torch" with diagnostics, "native" with diagnostics and "native" without.  On that premise every native
    scalar is within the derived bound (metrics_native_ref.bound: 1e-9 (|ref| + mean |input|)) of the float64 restatement evaluated on the
    torch metrics' own float32 records, and no further from it than the float32 torch value plus that bound.  A native round replayed from
    capture_graphs() gives the eager native round's 32 scalars and parameters bit for bit, over two rounds."""
    out, figures = tmp_path / "result.json", tmp_path / "test_figures.txt"
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "metrics_recorded_rounds.py")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    run = subprocess.run([sys.executable, script, str(out), str(figures)], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]        # (nothing further is started after a failure)
    with open(out) as f:
        result = json.load(f)
    print(figures.read_text())
    one, two = result["one"], result["two"]
    for net, d in one["digests"].items():
        assert d[0] == d[1] == d[2], (net, d)
    ref, bound, native, torch32 = (np.array(one[k]) for k in ("ref", "bound", "native", "torch"))
    assert len(ref) == 32 and np.isfinite(ref).all() and np.isfinite(native).all()
    for i, key in enumerate(one["keys"]):
        assert abs(native[i] - ref[i]) <= bound[i], (key, native[i], ref[i], bound[i])
        assert abs(native[i] - ref[i]) <= abs(torch32[i] - ref[i]) + bound[i], (key, native[i], torch32[i], ref[i])
    assert len(two["rounds"]) == 2 and two["silent"]
    for row in two["rounds"]:
        e, r = row["eager"], row["recorded"]
        assert e["finite"] and r["finite"] and e["keys"] == r["keys"] == one["keys"]
        assert e["scalars"] == r["scalars"], [(k, a, b) for k, a, b in zip(e["keys"], e["scalars"], r["scalars"]) if a != b]
        assert e["critic"] == r["critic"] and e["actor"] == r["actor"]
    assert two["rounds"][0]["eager"]["critic"] != two["rounds"][1]["eager"]["critic"]       # (the rounds moved the parameters)
