"""GPU checks of ``COMATrainer(shuffle=...)`` and of the trainer state above the kernel (tests/test_hip_shuffle.py): the default never
touches the entry point; a native round never calls ``torch.randperm``, launches once per data pass and cuts disjoint minibatches of flying
agents; and -- in a child process with deterministic convolutions (tests/shuffle_resume_rounds.py, run once for the module) -- runs are
reproducible whatever the torch seed, a replayed round is the eager round, a resumed run is the uninterrupted run bit for bit, and a resumed
mission logs what an uninterrupted one logs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_hip_adam_trainer import ALL_ENV, _count_lib, _trainer

pytestmark = pytest.mark.gpu

SWITCHES = ALL_ENV + ("IPPMARL_BUFFER", "IPPMARL_METRICS", "IPPMARL_ROLLOUT_LOG", "IPPMARL_SHUFFLE")
ENTRY = "ippm_minibatch_permutation"


def _clear(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


def test_switch_values(monkeypatch):
    _clear(monkeypatch)
    with pytest.raises(ValueError):
        _trainer(seed=6, n_envs=1, shuffle="hip")
    assert _trainer(seed=6, n_envs=1).shuffle == "torch"
    monkeypatch.setenv("IPPMARL_SHUFFLE", "native")
    assert _trainer(seed=6, n_envs=1).shuffle == "native"


def test_default_trainer_never_calls_the_entry_point(monkeypatch):
    _clear(monkeypatch)
    calls = _count_lib(monkeypatch, ENTRY)
    tr = _trainer(seed=6, n_envs=1)
    assert tr.shuffle == "torch" and tr._shuffle is None
    assert tr.rollout("train")["faults"] == 0
    tr.update()
    assert not calls and tr.train_step == 1


@pytest.mark.parametrize("buffer", ["torch", "native"])
def test_native_round_draws_no_torch_permutation(monkeypatch, buffer):
    _clear(monkeypatch)
    calls = _count_lib(monkeypatch, ENTRY)
    tr = _trainer(seed=6, n_envs=1, shuffle="native", buffer=buffer)
    assert tr.rollout("train")["faults"] == 0

    def refuse(*a, **k):
        raise AssertionError("torch.randperm called inside update() of a shuffle=\"native\" trainer")

    monkeypatch.setattr(torch, "randperm", refuse)
    for rnd in range(2):
        if rnd:
            assert tr.rollout("train")["faults"] == 0
        stats = tr.update()
        assert np.isfinite(stats["critic_loss"]) and np.isfinite(stats["actor_loss"])
        assert len(calls) == (rnd + 1) * tr.data_passes
    n = tr.T * tr.E * tr.N
    # by value: (seed, round = train_step on entry, no device counter, data_pass, n, no prefix)
    assert [(c[0], c[1], c[2], c[3], c[4], c[5]) for c in calls] == \
        [(tr.philox_seed, rnd, None, dp, n, None) for rnd in range(2) for dp in range(tr.data_passes)]
    if buffer == "native":
        assert int(tr._replay.bad.item()) == 0


def test_minibatches_are_disjoint_rows_of_flying_agents(monkeypatch):
    """Mixed team sizes: after a round, the rows of every data pass -- cut into batch_number minibatches as update() cuts them -- are
    distinct rows of ``valid_transitions``, which a native trainer never computes."""
    import shuffle_ref as S
    _clear(monkeypatch)
    tr = _trainer(seed=6, n_envs=3, shuffle="native", team_sizes=[1, 2, 2])
    called = []
    real = tr.valid_transitions
    monkeypatch.setattr(tr, "valid_transitions", lambda w: (called.append(w), real(w))[1])
    assert tr.rollout("train")["faults"] == 0
    stats = tr.update()
    assert not called
    flying = real(1).cpu().numpy()
    nv = flying.size
    assert nv == tr.T * 5 and stats["transitions"] == nv
    bs = nv // tr.batch_number
    for dp in range(tr.data_passes):
        rows = tr._shuffle.idx[dp, :nv].cpu().numpy()
        assert np.array_equal(rows, flying[S.permutation(nv, tr.philox_seed, 0, dp)])
        batches = [rows[b * bs:(b + 1) * bs] for b in range(tr.batch_number)]
        used = np.concatenate(batches)
        assert len(set(used.tolist())) == used.size == tr.batch_number * bs and np.isin(used, flying).all()
        agent, env = used % tr.N, (used // tr.N) % tr.E
        assert (agent < np.array([1, 2, 2])[env]).all()


def test_load_errors_and_the_state_file(monkeypatch, tmp_path):
    from ippmarl import _ffi
    _clear(monkeypatch)
    one, two = _trainer(seed=6, n_envs=1), _trainer(seed=6, n_envs=2)
    state = one.state_dict()
    with pytest.raises(_ffi.IppmError, match="n_envs"):
        two.load_state_dict(state)
    with pytest.raises(_ffi.IppmError, match="adam"):
        _trainer(seed=6, n_envs=1, adam="native").load_state_dict(state)
    path = str(tmp_path / "state.pt")
    one.save_state(path)
    loaded = torch.load(path, weights_only=True)
    assert set(loaded) == {"format", "fingerprint", "switches", "modules", "optimizers", "counters", "rng"}
    assert set(loaded["modules"]) == {"actor", "critic", "target_critic", "frozen_target"}
    assert set(loaded["counters"]) == {"train_step", "wave", "eval_wave", "step_replays", "eps", "shuffle_round"}
    assert len(loaded["switches"]) == 10 and loaded["switches"]["shuffle"] == "torch"
    # all or nothing: an optimizer state over another parameter list is refused before the modules are written
    bad = one.state_dict()
    bad["modules"]["actor"] = {k: torch.zeros_like(v) for k, v in bad["modules"]["actor"].items()}
    bad["optimizers"]["critic"]["param_groups"][0]["params"] = [0]
    with pytest.raises(_ffi.IppmError, match="critic optimizer"):
        one.load_state_dict(bad)
    assert all(torch.equal(p.detach().cpu(), state["modules"]["actor"][k]) for k, p in one.actor.named_parameters())
    assert any(bool(p.any()) for p in one.actor.parameters())
    assert one.rollout("train")["faults"] == 0 and one.filled == 1
    with pytest.raises(_ffi.IppmError, match="filled"):
        one.load_state(path)
    with pytest.raises(_ffi.IppmError, match="filled"):
        one.save_state(path)


# ---- the child process: whole rounds with deterministic convolutions ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rounds(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("shuffle")
    out = tmp / "result.json"
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shuffle_resume_rounds.py")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    run = subprocess.run([sys.executable, script, str(out), str(tmp)], env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]        # (nothing further is started after a failure)
    with open(out) as f:
        return json.load(f)


def test_premise_two_eager_trainers_agree(rounds):
    a, b = rounds["premise"]
    assert a == b and a["train_step"] == 1


def test_native_runs_are_reproducible_whatever_the_torch_seed(rounds):
    a, b = rounds["repro"]["native"]
    assert a["modules"] == b["modules"] and a["optimizers"] == b["optimizers"] and a == b and a["train_step"] == 2
    # (why the switch exists: the default's minibatch order is the device generator's)
    ta, tb = rounds["repro"]["torch"]
    assert ta["modules"]["actor"] != tb["modules"]["actor"] and ta["modules"]["critic"] != tb["modules"]["critic"]
    assert ta["modules"]["frozen_target"] == tb["modules"]["frozen_target"] == a["modules"]["frozen_target"]      # the same initial weights
    assert ta["modules"]["critic"] != a["modules"]["critic"]


def test_replayed_round_is_the_eager_round(rounds):
    rep = rounds["replay"]
    assert rep["first"][0] == rep["first"][1]
    assert rep["replays"] == [0, 2 * rep["T"]]
    assert len(rep["rounds"]) == 2
    for eager, rec in rep["rounds"]:
        assert eager == rec
    assert rep["rounds"][0][0]["modules"]["actor"] != rep["rounds"][1][0]["modules"]["actor"]
    assert rep["counter"] == [3, 3]                    # the graph advanced the device counter with train_step


RESUME = ["torch/torch", "torch/native", "native/torch", "native/native", "graphs", "graphs/torch"]


@pytest.mark.parametrize("case", RESUME)
def test_resumed_run_is_the_uninterrupted_run(rounds, case):
    r = rounds["resume"][case]
    a, c = r["a"], r["c"]
    assert a["train_step"] == c["train_step"] == 4 and a["wave"] == c["wave"] == 4
    for k in ("modules", "optimizers", "eps", "eps_dev", "returns", "filled"):
        assert a[k] == c[k], (case, k, a[k], c[k])
    assert a == c
    assert all(len(v) > 0 for v in a["optimizers"].values())
    assert r["replays"] == (2 * r["T"] if case.startswith("graphs") else 0)
    assert r["saved"]["modules"]["actor"] != a["modules"]["actor"]        # the two rounds after the save trained


@pytest.mark.parametrize("case", RESUME)
def test_frozen_target_and_the_rest_come_from_the_file(rounds, case):
    r = rounds["resume"][case]
    saved, loaded, fresh = r["saved"], r["loaded"], r["fresh"]
    assert loaded["modules"] == saved["modules"] and loaded["optimizers"] == saved["optimizers"]
    assert loaded["wave"] == saved["wave"] == 2 and loaded["train_step"] == 2 and loaded["eps"] == saved["eps"] and loaded["eps_dev"] == saved["eps_dev"]
    assert loaded["modules"]["frozen_target"] != loaded["modules"]["critic"]             # the construction-time copy, not the trained critic
    assert loaded["modules"]["target_critic"] != loaded["modules"]["critic"]             # (copy_rate 3: last synchronised before round 0)
    assert fresh["modules"]["frozen_target"] != saved["modules"]["frozen_target"]        # C was built from other weights


def test_resumed_mission_logs_what_an_uninterrupted_one_logs(rounds):
    m = rounds["mission"]
    whole, parts = m["whole"], m["stopped"] + m["resumed"]
    assert [(tag, step) for tag, _, step in whole] == [(tag, step) for tag, _, step in parts] and len(whole) > 3 * 24
    assert {step for _, _, step in m["resumed"]} == {3}
    differing = [(tag, step) for (tag, v, step), (_, w, _) in zip(whole, parts) if v != w]
    assert differing == [], differing[:10]               # (more than the tags: with deterministic convolutions the values are the same bits)
    assert m["best"][0] == m["best"][1] and m["returns"][0] == m["returns"][1] and len(m["returns"][0]) == 3
    assert m["steps"][0] == m["steps"][1] and m["steps"][0][0] == 3
    assert m["at_resume"][0] == 2 and m["at_resume"][2] == 2
    assert m["state_exists"] and not m["leftovers"]
    # best_model.pth as before: wherever the running mean improved (the resumed half writes one only if its round improved on the file's)
    assert m["best_model"][0] and (m["best_model"][1] or m["best_model"][2])
