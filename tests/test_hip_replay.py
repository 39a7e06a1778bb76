"""GPU checks of the native replay buffer (csrc/replay.hip, ippmarl/replay_native.py, ``COMATrainer(buffer="native")``): the three kernels on
constructed tensors against the tensor operations they replace, compared as BYTES; then the trainer -- the default path never calls
them, the learners are fed the same bytes either way, whole rounds end in the same parameters, and the native path launches less."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from configs import make_params
from test_hip_adam_trainer import ALL_ENV, _count_lib, _params64, _trainer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ENTRY_POINTS = ("ippm_replay_store", "ippm_td_lambda_buffer", "ippm_replay_gather")
SWITCHES = ALL_ENV + ("IPPMARL_BUFFER",)
NAN_BITS = 0x7FC00DAD          # a quiet NaN with a payload: what a buffer element holds before anything stored it
OBS, STATE = 11 * 11 * 7, 11 * 11 * 12


def _lib():
    from ippmarl import _ffi
    return _ffi, _ffi.load_library()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bytes(a), _bytes(b))


def _last_error():
    return _lib()[1].ippm_last_error().decode()


def _rand(gen, *shape):
    return torch.randn(*shape, generator=gen).to(DEV)


# ---- 1. store ---------------------------------------------------------------------------------------------------------------------------------
def _buffers(W, T, E, N, A, deepq):
    f = lambda *s: torch.full(s, NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)  # noqa: E731
    return [f(W, T, E, N, 11, 11, 7), f(W, T, E, N, 11, 11, 12), torch.full((W, T, E, N), NAN_BITS, dtype=torch.int32, device=DEV),
            torch.full((W, T, E, N, A), 0xA5, dtype=torch.uint8, device=DEV), f(W, T, E, N) if deepq else f(W, T, E)]


@pytest.mark.parametrize("form", ["coma", "deepq"])
@pytest.mark.parametrize("E,N", [(3, 2), (2, 2)])
def test_store_equals_the_copies_and_adds(E, N, form):
    """Every (w, t) stored in a scrambled order (E*N*847*4 bytes is no multiple of 16 at E, N = 3, 2: odd slots are misaligned; 2, 2 is
    aligned), one step with store = 0 in between: buffers and accumulators are the bytes of copy_ and += ."""
    ffi, lib = _lib()
    W, T, A = 2, 3, 6
    deepq = form == "deepq"
    assert ((E * N * OBS * 4) % 16 != 0) == ((E, N) == (3, 2))
    gen = torch.Generator().manual_seed(100 * E + N + (7 if deepq else 0))
    want, got = _buffers(W, T, E, N, A, deepq), _buffers(W, T, E, N, A, deepq)
    acc0 = [_rand(gen, E) for _ in range(3)]
    want_acc, got_acc = [a.clone() for a in acc0], [a.clone() for a in acc0]
    last = torch.tensor([0, 1, 1][:E], dtype=torch.int64, device=DEV)
    last32 = last.to(torch.int32)
    last_idx = last.view(E, 1, 1).expand(E, 1, 2).contiguous()
    order = [(1, 1), (0, 2), (1, 0), None, (0, 0), (1, 2), (0, 1)]          # None: the step with store = 0
    p = ffi.ptr
    for slot in order:
        obs, state = _rand(gen, E, N, 11, 11, 7), _rand(gen, E, N, 11, 11, 12)
        action = torch.randint(0, A, (E, N), generator=gen, dtype=torch.int32).to(DEV)
        mask = torch.randint(0, 2, (E, N, A), generator=gen, dtype=torch.uint8).to(DEV)
        reward, agent_reward = _rand(gen, E, 2), _rand(gen, E, N, 2)
        # the tensor operations of COMATrainer._rollout_step
        r = agent_reward.gather(1, last_idx).squeeze(1) if deepq else reward
        if slot is not None:
            w, t = slot
            for buf, x in zip(want, (obs, state, action, mask, agent_reward[..., 0] if deepq else reward[:, 0])):
                buf[w, t].copy_(x)
        want_acc[0] += r[:, 0]
        want_acc[1] += r[:, 1]
        want_acc[2] += reward[:, 0]
        w, t = slot if slot is not None else (0, 0)
        rc = lib.ippm_replay_store(p(obs), p(state), p(action), p(mask), p(reward), p(agent_reward) if deepq else None,
                                   p(last32) if deepq else None, E, N, A, W, T, w, t, 0 if slot is None else 1, *[p(b) for b in got],
                                   *[p(a) for a in got_acc], _stream())
        assert rc == 0, _last_error()
    torch.cuda.synchronize()
    for name, a, b in zip(("obs", "state", "action", "mask", "reward", "ret", "abs_ret", "team_ret"), want + want_acc, got + got_acc):
        assert _same(a, b), (name, int((_bytes(a) != _bytes(b)).sum()))
    assert not bool(torch.isnan(got[0]).any())                                # every slot was stored


def test_store_argument_errors_launch_nothing():
    ffi, lib = _lib()
    E, N, A, W, T = 2, 2, 6, 1, 2
    got = _buffers(W, T, E, N, A, False)
    acc = [torch.zeros(E, device=DEV) for _ in range(3)]
    before = [t.clone() for t in got + acc]
    p = ffi.ptr
    obs, state = torch.ones(E, N, 11, 11, 7, device=DEV), torch.ones(E, N, 11, 11, 12, device=DEV)
    action, mask = torch.ones(E, N, dtype=torch.int32, device=DEV), torch.ones(E, N, A, dtype=torch.uint8, device=DEV)
    reward = torch.ones(E, 2, device=DEV)

    def call(obs=obs, reward=reward, A=A, w=0, t=0, agent=None, last=None):
        return lib.ippm_replay_store(p(obs), p(state), p(action), p(mask), p(reward), p(agent), p(last), E, N, A, W, T, w, t, 1,
                                     *[p(b) for b in got], *[p(a) for a in acc], _stream())

    for kw in (dict(obs=None), dict(reward=None), dict(A=0), dict(A=33), dict(w=1), dict(t=2), dict(t=-1),
               dict(agent=torch.ones(E, N, 2, device=DEV))):
        assert call(**kw) == -1, kw
        assert "ippm_replay_store" in _last_error(), (kw, _last_error())
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(before, got + acc))
    assert call() == 0


# ---- 2. TD(lambda) from buffer order ---------------------------------------------------------------------------------------------------------
def td_lambda_f64(rewards, dones, q_sel, gamma, lam):
    """BatchMemory.build_td_targets (batch_memory.py:120-162) on one chain, restated in float64 NumPy as the reference writes it: for
    every t, the lambda-weighted sum over n of the n-step returns, each summed from scratch; the done flag of the PREVIOUS transition gates
    the accumulation."""
    L = len(rewards)
    td, dr = np.zeros(L), np.zeros(L)
    for t in range(L):
        total = disc = 0.0
        for n in range(1, L - t + 1):
            g, leave = 0.0, False
            for l in range(n):  # noqa: E741
                if t + l == 0 or not dones[t + l - 1]:
                    g += gamma ** l * rewards[t + l]
                else:
                    leave = True
                    break
            disc = g
            if leave:
                total += lam ** n * g
                break
            if t + n < L and not (dones[t + n] or t + n + 1 >= L):
                g += gamma ** n * q_sel[t + n]
            total += lam ** (n - 1) * g
        td[t], dr[t] = (1 - lam) * total, disc
    return td, dr


@pytest.fixture(scope="module")
def ctx():
    from ippmarl import _ffi
    from ippmarl.derived import DerivedConstants
    return _ffi.Context(DerivedConstants(make_params("small")))


@pytest.mark.parametrize("per_agent", [False, True])
@pytest.mark.parametrize("T", [1, 15])
@pytest.mark.parametrize("W", [1, 2])
def test_td_from_buffer_order_is_td_lambda_on_the_chain_layout(ctx, W, T, per_agent):
    """td and dr equal, bit for bit, ippm_td_lambda on the permuted chain layout as COMATrainer.td_targets builds it (buffer="torch"),
    permuted back; W, T = 2, 15 with broadcast rewards also against the float64 restatement at 1e-5 relative."""
    ffi, lib = _lib()
    E, N = 3, 2
    gen = torch.Generator().manual_seed(1000 + 100 * W + 2 * T + per_agent)
    q_buf = _rand(gen, W, T, E, N)
    r_buf = _rand(gen, W, T, E, N) if per_agent else _rand(gen, W, T, E)
    p = ffi.ptr
    # today's path
    q_sel = q_buf.permute(2, 3, 0, 1).reshape(E * N, W * T).contiguous()
    rew = (r_buf if per_agent else r_buf.unsqueeze(-1).expand(W, T, E, N)).permute(2, 3, 0, 1).reshape(E * N, W * T).contiguous()
    done = torch.zeros(W, T, dtype=torch.uint8, device=DEV)
    done[:, T - 1] = 1
    done = done.view(1, W * T).expand(E * N, W * T).contiguous()
    td_c, dr_c = torch.empty_like(rew), torch.empty_like(rew)
    ctx.call("ippm_td_lambda", p(rew), p(done), p(q_sel), p(td_c), p(dr_c), E * N, W * T, _stream())
    to_buf = lambda x: x.view(E, N, W, T).permute(2, 3, 0, 1).reshape(-1)  # noqa: E731
    # from buffer order
    td = torch.full((W * T * E * N,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    dr = td.clone()
    ctx.call("ippm_td_lambda_buffer", p(r_buf), 1 if per_agent else 0, p(q_buf), p(td), p(dr), W, T, E, N, _stream())
    torch.cuda.synchronize()
    assert _same(td, to_buf(td_c)) and _same(dr, to_buf(dr_c))
    if (W, T, per_agent) == (2, 15, False):
        gamma, lam = float(ctx.cfg.gamma), float(ctx.cfg.lambda_)
        q_np, r_np = q_buf.cpu().double().numpy(), r_buf.cpu().double().numpy()
        got_td, got_dr = td.view(W, T, E, N).cpu().numpy(), dr.view(W, T, E, N).cpu().numpy()
        dones = [t == T - 1 for _ in range(W) for t in range(T)]
        for e in range(E):
            for n in range(N):
                want_td, want_dr = td_lambda_f64(r_np[:, :, e].reshape(-1), dones, q_np[:, :, e, n].reshape(-1), gamma, lam)
                np.testing.assert_allclose(got_td[:, :, e, n].reshape(-1), want_td, rtol=1e-5, atol=0)
                np.testing.assert_allclose(got_dr[:, :, e, n].reshape(-1), want_dr, rtol=1e-5, atol=0)


def test_td_buffer_argument_errors(ctx):
    ffi, lib = _lib()
    x = torch.zeros(8, device=DEV)
    out = torch.full((8,), 3.0, device=DEV)
    p = ffi.ptr
    for args in ((None, 0, p(x), p(out), p(out), 1, 2, 2, 2), (p(x), 0, p(x), None, p(out), 1, 2, 2, 2), (p(x), 0, p(x), p(out), p(out), 0, 2, 2, 2),
                 (p(x), 0, p(x), p(out), p(out), 1, 2, 2, -1), (p(x), 0, p(x), p(out), p(out), 1 << 15, 1 << 15, 2, 2)):
        assert lib.ippm_td_lambda_buffer(ctx.handle, *args, _stream()) == -1
        assert "ippm_td_lambda_buffer" in _last_error()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


# ---- 3. gather ---------------------------------------------------------------------------------------------------------------------------------
N_ROWS, A_G = 37, 6


@pytest.fixture(scope="module")
def sources():
    """The five training arrays of n = 37 rows as ONE-ROW-OFFSET views of allocations of n + 2 rows: row 0 of an allocation is in front of
    the view (an obs row is 3388 bytes, so the view's rows start at addresses that are 4-byte aligned only), row n + 1 is a sentinel row
    behind it -- the row an index equal to n would reach."""
    gen = torch.Generator().manual_seed(37)
    full = [_rand(gen, N_ROWS + 2, 11, 11, 12), _rand(gen, N_ROWS + 2, 11, 11, 7),
            torch.randint(0, A_G, (N_ROWS + 2,), generator=gen, dtype=torch.int32).to(DEV),
            torch.randint(1, 3, (N_ROWS + 2, A_G), generator=gen, dtype=torch.uint8).to(DEV), _rand(gen, N_ROWS + 2)]
    views = [t[1:] for t in full]                 # n + 1 rows: the kernel is told n
    assert views[1].data_ptr() % 16 != 0 and views[1][1].data_ptr() % 16 != 0 and views[1].data_ptr() % 4 == 0
    torch.cuda.synchronize()
    return full, views


def _outputs(rows):
    f = lambda *s: torch.full(s, NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)  # noqa: E731
    return [f(rows, 11, 11, 12), f(rows, 11, 11, 7), torch.full((rows,), NAN_BITS, dtype=torch.int32, device=DEV),
            torch.full((rows, A_G), 0xA5, dtype=torch.uint8, device=DEV), f(rows)]


def _gather(views, idx, outs, n=N_ROWS, count=None, A=A_G, bad=None, idx_ptr=True):
    ffi, lib = _lib()
    p = ffi.ptr
    return lib.ippm_replay_gather(*[p(v) for v in views], n, p(idx) if idx_ptr else None, idx.numel() if count is None else count, A,
                                  *[None if o is None else p(o) for o in outs], p(bad), _stream())


@pytest.mark.parametrize("case", ["one", "repeated", "reversed"])
def test_gather_equals_indexing(sources, case):
    _, views = sources
    idx = {"one": [17], "repeated": [3, 3, 36, 0, 3], "reversed": list(range(N_ROWS - 1, -1, -1))}[case]
    idx = torch.tensor(idx, dtype=torch.int64, device=DEV)
    count = idx.numel()
    assert count in (1, 5, 37)
    outs, fresh = _outputs(count + 2), _outputs(count + 2)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert _gather(views, idx, outs, bad=bad) == 0, _last_error()
    torch.cuda.synchronize()
    for name, v, o, f in zip(("states", "obs", "actions", "masks", "td"), views, outs, fresh):
        assert _same(o[:count], v[:N_ROWS][idx]), name                         # torch indexing, byte for byte
        assert _same(o[count:], f[count:]), name + ": rows beyond count"       # ... and the rows beyond count keep their sentinel
    assert int(bad) == 0


def test_gather_skips_null_outputs(sources):
    _, views = sources
    idx = torch.tensor([5, 36, 1], dtype=torch.int64, device=DEV)
    outs = _outputs(3)
    only = [None, outs[1], None, None, outs[4]]
    assert _gather(views, idx, only) == 0, _last_error()
    assert _gather([None, views[1], None, None, views[4]], idx, only) == 0, _last_error()      # a skipped array needs no buffer either
    torch.cuda.synchronize()
    fresh = _outputs(3)
    assert _same(outs[1], views[1][idx]) and _same(outs[4], views[4][idx])
    assert all(_same(outs[k], fresh[k]) for k in (0, 2, 3))


def test_gather_guards_an_index_outside_the_buffer(sources):
    """An index equal to n (and a negative one): the row comes back as zeros and is counted.  The allocations hold a sentinel row at n, so
    whatever the kernel does with that index stays inside them."""
    full, views = sources
    idx = torch.tensor([2, N_ROWS, 5, -1], dtype=torch.int64, device=DEV)
    outs = _outputs(4)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    kept = [t.clone() for t in full]
    assert _gather(views, idx, outs, bad=bad) == 0, _last_error()
    torch.cuda.synchronize()
    assert int(bad) == 2
    for v, o in zip(views, outs):
        assert _same(o[0], v[2]) and _same(o[2], v[5])
        assert not bool(_bytes(o[1]).any()) and not bool(_bytes(o[3]).any())
    assert all(_same(a, b) for a, b in zip(kept, full))
    idx = torch.tensor([N_ROWS], dtype=torch.int64, device=DEV)                 # the issue's case on its own: one index equal to n
    bad.zero_()
    outs = _outputs(1)
    assert _gather(views, idx, outs, bad=bad) == 0
    torch.cuda.synchronize()
    assert int(bad) == 1 and all(not bool(_bytes(o).any()) for o in outs)


def test_gather_argument_errors_leave_the_outputs_untouched(sources):
    _, views = sources
    idx = torch.tensor([1, 2], dtype=torch.int64, device=DEV)
    outs, fresh = _outputs(2), _outputs(2)
    for kw in (dict(idx_ptr=False), dict(count=-1), dict(A=0), dict(A=33), dict(n=0)):
        assert _gather(views, idx, outs, **kw) == -1, kw
        assert "ippm_replay_gather" in _last_error(), (kw, _last_error())
    assert _gather([None] + views[1:], idx, outs) == -1 and "ippm_replay_gather" in _last_error()     # an output without its buffer
    assert _gather(views, idx, outs, count=0) == 0                                                   # nothing to do is no error
    torch.cuda.synchronize()
    assert all(_same(o, f) for o, f in zip(outs, fresh))


# ---- 4. the trainer ----------------------------------------------------------------------------------------------------------------------------
def _clear(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


def test_default_round_never_touches_the_replay_kernels(monkeypatch):
    _clear(monkeypatch)
    calls = {name: _count_lib(monkeypatch, name) for name in ENTRY_POINTS}
    tr = _trainer(seed=6, n_envs=1)
    assert tr.buffer == "torch" and tr._replay is None
    assert tr.rollout("train")["faults"] == 0
    stats = tr.update()
    assert np.isfinite(stats["critic_loss"]) and not any(calls.values()), {k: len(v) for k, v in calls.items()}


def test_environment_variable_selects_the_native_buffer(monkeypatch):
    from ippmarl import replay_native
    _clear(monkeypatch)
    monkeypatch.setenv(replay_native.ENV_VAR, "native")                # the environment variable is how bench.py gets the switch
    calls = {name: _count_lib(monkeypatch, name) for name in ENTRY_POINTS}
    tr = _trainer(seed=6, n_envs=1)
    assert tr.buffer == "native" and type(tr._replay) is replay_native.NativeReplay
    assert tr.rollout("train")["faults"] == 0
    stats = tr.update()
    assert np.isfinite(stats["critic_loss"]) and np.isfinite(stats["actor_loss"])
    assert len(calls["ippm_replay_store"]) == tr.T and len(calls["ippm_td_lambda_buffer"]) == 1
    assert len(calls["ippm_replay_gather"]) == tr.data_passes * tr.batch_number
    assert int(tr._replay.bad) == 0
    assert tr.rollout("eval")["faults"] == 0                            # store = 0: the accumulators only
    assert len(calls["ippm_replay_store"]) == 2 * tr.T and all(c[14] == 0 for c in calls["ippm_replay_store"][tr.T:])
    assert tr.rollout("train")["faults"] == 0                           # a diagnostics round keeps the torch gathers
    gathers = len(calls["ippm_replay_gather"])
    tr.update(diagnostics=True)
    assert tr.last_diagnostics and len(calls["ippm_replay_gather"]) == gathers


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(f"{t.dtype}{tuple(t.shape)}".encode())
        h.update(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


CONFIGS = {"coma": ({}, {}, 1), "deepq": (dict(experiment__missions__type="DeepQ"), {}, 1), "teams": ({}, dict(team_sizes=[1, 2, 2]), 1),
           "waves2": ({}, dict(waves_per_update=2), 2)}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_learners_are_fed_the_same_bytes(monkeypatch, config):
    """Two trainers from one seed, buffer="torch" and buffer="native": after the rollout wave(s) and one update, every tensor the two
    learners' backward() received, the buf_* tensors, the returns, td and dr are identical."""
    _clear(monkeypatch)
    over, kw, waves = CONFIGS[config]
    seen = {}
    for mode in ("torch", "native"):
        tr = _trainer(seed=31, n_envs=3, params=_params64(**over), buffer=mode, **kw)
        # Nothing compared here may depend on what the convolutions do (the library may pick another algorithm for the second trainer's
        # first forward of a shape): the target critic of the TD targets is replaced by a plain function of the state's bytes.
        tr.frozen_target = lambda s, _A=tr.A: (s.reshape(s.shape[0], -1)[:, 40:40 + _A] * 3.0 + s.reshape(s.shape[0], -1)[:, 700:701], None)
        fed = []
        for learner, n_data in ((tr.critic_learner, 3), (tr.actor_learner, 3)):
            real = learner.backward
            learner.backward = (lambda *a, _real=real, _n=n_data, _who=type(learner).__name__:
                                (fed.append((_who, _digest(*a[:_n]))), _real(*a))[1])
        returns = []
        for _ in range(waves):
            assert tr.rollout("train")["faults"] == 0
            returns.append(_digest(tr.ret, tr.abs_ret, tr.team_ret))
        torch.manual_seed(77)                                               # the minibatch permutations
        td, dr = tr.td_targets()
        targets = _digest(td.clone(), dr.clone())
        stats = tr.update()
        torch.cuda.synchronize()
        assert np.isfinite(stats["critic_loss"]) and len(fed) == 2 * tr.data_passes * tr.batch_number
        if mode == "native":
            assert int(tr._replay.bad) == 0
        seen[mode] = dict(fed=fed, returns=returns, targets=targets,
                          buffers=[_digest(b) for b in (tr.buf_obs, tr.buf_state, tr.buf_action, tr.buf_mask, tr.buf_reward)])
    for key in ("buffers", "returns", "targets"):
        assert seen["torch"][key] == seen["native"][key], key
    differ = [i for i, (a, b) in enumerate(zip(seen["torch"]["fed"], seen["native"]["fed"])) if a != b]
    assert not differ, (differ[:5], len(seen["torch"]["fed"]))


@pytest.fixture(scope="module")
def rounds(tmp_path_factory):
    """tests/replay_recorded_rounds.py in a process of its own (the convolution library in deterministic mode), once for the module."""
    out = tmp_path_factory.mktemp("replay") / "digests.json"
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "replay_recorded_rounds.py")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    run = subprocess.run([sys.executable, script, str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]        # (nothing further is started after a failure)
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("config", ["defaults", "all_six_on"])
def test_two_rounds_end_in_the_same_parameters(rounds, config):
    """After two rounds both nets' parameters are identical for buffer="torch" and buffer="native" -- with every other switch at its
    default, and with all six others on."""
    for net, n in rounds[config].items():
        print(f"{config} {net}: {n['differ']} of {n['numel']} parameters differ torch - native; two rounds moved them by up to {n['moved']:.3e}")
    for net, n in rounds[config].items():
        assert n["finite"] and n["moved"] > 0, (net, n)
        assert n["digests"][0] == n["digests"][1] and n["differ"] == 0, (net, n)


def test_recorded_round_equals_eager_round(rounds):
    """graphs=True, adam="native", head_update="bf16", buffer="native": two eager rounds agree (the premise), and the round replayed from
    hipGraphs ends in the eager round's parameters bit for bit."""
    for net, n in rounds["recorded"].items():
        print(f"{net}: {n['differ']} of {n['numel']} parameters differ eager - recorded, {n['premise_differ']} eager - eager; "
              f"the round moved them by up to {n['moved']:.3e}")
    for net, n in rounds["recorded"].items():
        assert n["finite"] and n["moved"] > 0, (net, n)
        assert n["digests"][0] == n["digests"][1] and n["premise_differ"] == 0, (net, n)
        assert n["digests"][0] == n["digests"][2] and n["differ"] == 0, (net, n)
    assert rounds["recorded_bad_indices"] == 0


def _device_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def test_native_buffer_launches_less(monkeypatch):
    """Device launches (kernels and copies, torch.profiler) of one _rollout_step and of one _update_compute round: the native buffer
    issues strictly fewer of both."""
    from ippmarl.parallel import episode_ids
    from ippmarl.vec_env import POLICY_SAMPLE
    _clear(monkeypatch)
    counts = {}
    for mode in ("torch", "native"):
        tr = _trainer(seed=41, n_envs=3, buffer=mode)
        tr.rollout("train")                                # warm-up: kernel selection, allocator, the replay's output sets
        tr.update()
        tr.rollout("train")
        tr.env.reset(episode_ids(tr.first_episode, tr.wave, tr.E, tr.rank, tr.world))
        step =_device_launches(lambda: tr._rollout_step(0, 0, POLICY_SAMPLE, True, tr.eps))
        torch.manual_seed(5)
        update = _device_launches(lambda: tr._update_compute(None, tr.eps, False))
        counts[mode] = (step, update)
    print(f"device launches of one rollout step: torch {counts['torch'][0]}, native {counts['native'][0]}; "
          f"of one update round: torch {counts['torch'][1]}, native {counts['native'][1]}")
    assert 0 < counts["native"][0] < counts["torch"][0]
    assert 0 < counts["native"][1] < counts["torch"][1]
