"""GPU checks of the native bf16 critic inference (csrc/critic_infer.hip behind ippm_critic_pack / ippm_critic_forward, NativeCritic, the
trainer's ``critic_inference="native"``).  The reference of every numerical check is the CPU restatement of the contract
(tests/critic_native_ref.py on actor_native_ref's ``emulate_*``), never the code under test; every tolerance is ``MARGIN`` spreads between
the float32 and the float64 emulation of the same case, the unit of the actor's tests."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import critic_native_ref as R
from configs import make_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE, SLICE = 128, 4096     # rows of a workgroup tile of the layer kernel; samples per internal slice of ippm_critic_forward


def _lib():
    from ippmarl import _ffi
    return _ffi, _ffi.load_library()


def _pack(net, A):
    _ffi, lib = _lib()
    nbytes = C.c_int64(0)
    _ffi.check(lib.ippm_critic_pack_bytes(A, C.addressof(nbytes)), "ippm_critic_pack_bytes")
    packed = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device=DEV)
    dev = [t.to(DEV).contiguous() for name in R.TRUNK + ("fc3",) for t in net[name]]
    _ffi.check(lib.ippm_critic_pack(*[t.data_ptr() for t in dev], A, packed.data_ptr(), torch.cuda.current_stream().cuda_stream), "ippm_critic_pack")
    torch.cuda.synchronize()
    return packed


def _call(packed, states, A, actions=None, want_q=True, want_sel=None):
    """ippm_critic_forward on outputs AND scratch pre-filled with NaN -> (rc, q, q_sel) with the outputs on the CPU (None: passed NULL)."""
    _ffi, lib = _lib()
    states = states.to(DEV).contiguous()
    B = states.shape[0]
    want_sel = actions is not None if want_sel is None else want_sel
    nbytes = C.c_int64(0)
    _ffi.check(lib.ippm_critic_scratch_bytes(B, C.addressof(nbytes)), "ippm_critic_scratch_bytes")
    assert nbytes.value == min(B, SLICE) * 34304         # bounded by the slice, whatever the batch
    scratch = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device=DEV)     # bf16 0xFFFF: NaN
    q = torch.full((B, A), float("nan"), device=DEV) if want_q else None
    q_sel = torch.full((B,), float("nan"), device=DEV) if want_sel else None
    act = None if actions is None else actions.to(DEV, torch.int32).contiguous()
    rc = lib.ippm_critic_forward(packed.data_ptr(), states.data_ptr(), B, A, _ffi.ptr(act), scratch.data_ptr(), _ffi.ptr(q), _ffi.ptr(q_sel),
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, None if q is None else q.cpu(), None if q_sel is None else q_sel.cpu()


def _forward(packed, states, A, actions=None, **kw):
    _ffi, _ = _lib()
    rc, q, q_sel = _call(packed, states, A, actions, **kw)
    _ffi.check(rc, "ippm_critic_forward")
    return q, q_sel


@pytest.fixture(scope="module")
def exact_packs():
    return {A: _pack(R.exact_net(R.EXACT_SEED, A), A) for A in (6, 27)}


# ---- 1. exact network: pins the 12-plane gather, the pack and the head --------------------------------------------------------------
@pytest.mark.parametrize("A", [6, 27])
def test_exact_network_bit_for_bit(exact_packs, A):
    states = R.exact_states(R.EXACT_SEED, R.EXACT_BATCH)
    actions = R.exact_actions(R.EXACT_SEED, R.EXACT_BATCH, A)
    want = R.exact_q(R.EXACT_SEED, R.EXACT_BATCH, A)
    q, q_sel = _forward(exact_packs[A], states, A, actions)
    assert torch.equal(q.double(), want), (A, int((q.double() != want).sum()))
    assert torch.equal(q_sel.double(), R.gather(want, actions)), A


# ---- 2. batch shapes and determinism ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 63, 64, 65, 257, 4097])
def test_batch_shapes_and_determinism(exact_packs, B):
    A = 6
    rows = torch.arange(B) % R.EXACT_BATCH                 # (beyond 300 samples the states repeat: the reference is shared)
    states = R.exact_states(R.EXACT_SEED, R.EXACT_BATCH)[rows]
    actions = R.exact_actions(R.EXACT_SEED, R.EXACT_BATCH, A)[rows]
    want = R.exact_q(R.EXACT_SEED, R.EXACT_BATCH, A)[rows]
    q, q_sel = _forward(exact_packs[A], states, A, actions)               # (scratch and outputs start as 0xFF / NaN: _call)
    assert not torch.isnan(q).any() and not torch.isnan(q_sel).any()
    assert torch.equal(q.double(), want) and torch.equal(q_sel.double(), R.gather(want, actions))
    q2, q_sel2 = _forward(exact_packs[A], states, A, actions)
    assert torch.equal(q, q2) and torch.equal(q_sel, q_sel2)                  # run to run
    # alone == in the batch: the first and last row, the rows on either side of the first tile edge and of the slice boundary
    for r in sorted(r for r in {0, TILE - 1, TILE, 2 * TILE, SLICE - 1, SLICE, B - 2, B - 1} if 0 <= r < B):
        q1, s1 = _forward(exact_packs[A], states[r:r + 1], A, actions[r:r + 1])
        assert torch.equal(q1[0], q[r]) and torch.equal(s1[0], q_sel[r]), (B, r)


def test_position_in_a_dense_batch_does_not_matter():
    """The same on values that do round: a dense sample alone, and at two other positions of a batch of other samples."""
    A, seed = 6, R.DENSE_SEEDS[0]
    packed = _pack(R.dense_net(seed, A), A)
    states = R.dense_states(seed, R.DENSE_BATCH)[:200]
    q, _ = _forward(packed, states, A)
    for r in (0, 77, 199):
        q1, _ = _forward(packed, states[r:r + 1], A)
        assert torch.equal(q1[0], q[r]), r
    perm = torch.arange(199, -1, -1)
    qp, _ = _forward(packed, states[perm], A)
    assert torch.equal(qp, q[perm])


# ---- 3. dense networks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.DENSE_SEEDS)
@pytest.mark.parametrize("A", [6, 27])
def test_dense_network_within_four_spreads(seed, A):
    d, q64 = R.dense_spread(seed, A)
    actions = torch.randint(0, A, (R.DENSE_BATCH,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    q, q_sel = _forward(_pack(R.dense_net(seed, A), A), R.dense_states(seed, R.DENSE_BATCH), A, actions)
    err = float((q.double() - q64).abs().max())
    print(f"seed {seed} A {A}: spread {d:.3e}; device error {err:.3e}")
    assert err <= R.MARGIN * d, (err, d)
    assert torch.equal(q_sel, R.gather(q, actions))


# ---- 4. argument rules ------------------------------------------------------------------------------------------------------------------
def test_argument_rules(exact_packs):
    _ffi, lib = _lib()
    A, B = 6, 40
    states = R.exact_states(R.EXACT_SEED, R.EXACT_BATCH)[:B]
    actions = R.exact_actions(R.EXACT_SEED, R.EXACT_BATCH, A)[:B].clone()
    want = R.exact_q(R.EXACT_SEED, R.EXACT_BATCH, A)[:B]
    q, none = _forward(exact_packs[A], states, A)                                  # q_sel NULL (and no action)
    assert none is None and torch.equal(q.double(), want)
    q, none = _forward(exact_packs[A], states, A, actions, want_sel=False)         # q_sel NULL, action given
    assert none is None and torch.equal(q.double(), want)
    none, q_sel = _forward(exact_packs[A], states, A, actions, want_q=False)       # q NULL
    assert none is None and torch.equal(q_sel.double(), R.gather(want, actions))
    rc, _, _ = _call(exact_packs[A], states, A, actions, want_q=False, want_sel=False)
    assert rc != 0 and "both NULL" in lib.ippm_last_error().decode()
    rc, _, q_sel = _call(exact_packs[A], states, A, None, want_sel=True)
    assert rc != 0 and "action" in lib.ippm_last_error().decode()
    assert bool(torch.isnan(q_sel).all())                                          # nothing was launched
    # an action outside [0, A): NaN in that row only, and the full table is untouched by it
    bad = actions.clone()
    bad[3], bad[17] = -1, A
    q, q_sel = _forward(exact_packs[A], states, A, bad)
    ok = torch.ones(B, dtype=torch.bool)
    ok[3] = ok[17] = False
    assert bool(torch.isnan(q_sel[~ok]).all()) and torch.equal(q.double(), want)
    assert torch.equal(q_sel[ok].double(), R.gather(want, actions)[ok])
    # n_actions outside [1, 32]
    out = C.c_int64(0)
    st, table = states.to(DEV).contiguous(), torch.zeros(B * 33, device=DEV)
    scratch = torch.empty(B * 34304, dtype=torch.uint8, device=DEV)
    weights = [t.to(DEV).contiguous() for name in R.TRUNK + ("fc3",) for t in R.exact_net(R.EXACT_SEED, A)[name]]
    stream = torch.cuda.current_stream().cuda_stream
    for n in (0, 33):
        assert lib.ippm_critic_pack_bytes(n, C.addressof(out)) != 0 and "n_actions" in lib.ippm_last_error().decode(), n
        assert lib.ippm_critic_pack(*[t.data_ptr() for t in weights], n, scratch.data_ptr(), stream) != 0, n
        assert "n_actions" in lib.ippm_last_error().decode(), n
        assert lib.ippm_critic_forward(exact_packs[A].data_ptr(), st.data_ptr(), B, n, None, scratch.data_ptr(), table.data_ptr(), None, stream) != 0, n
        assert "n_actions" in lib.ippm_last_error().decode(), n
    torch.cuda.synchronize()
    assert not bool(table.any())                                                   # nothing was launched
    assert lib.ippm_critic_pack_bytes(32, C.addressof(out)) == 0 and out.value > 0


# ---- 5.-8. trainer ------------------------------------------------------------------------------------------------------------------
def _params64(**kw):
    """2 UAVs on a 64 x 64 grid, as the native actor's trainer tests."""
    return make_params("small", experiment__missions__n_agents=2, sensor__field_of_view__angle_x=99.0, sensor__field_of_view__angle_y=99.0, **kw)


def _trainer(seed=5, n_envs=3, params=None, **kw):
    from ippmarl.trainer import COMATrainer
    torch.manual_seed(seed)
    return COMATrainer(params or _params64(), n_envs=n_envs, first_episode=3, **kw)


def _buffer(tr):
    n = tr.filled * tr.T * tr.E * tr.N
    return tr.buf_state[:tr.filled].reshape(n, 11, 11, 12), tr.buf_action[:tr.filled].reshape(n)


def _td_lambda(tr, q_sel):
    """ippm_td_lambda on one chain per (env, agent), as COMATrainer.td_targets lays them out -> td in buffer order."""
    from ippmarl import _ffi
    W, T, E, N = tr.filled, tr.T, tr.E, tr.N
    q = q_sel.view(W, T, E, N).permute(2, 3, 0, 1).reshape(E * N, W * T).contiguous()
    rew = tr.buf_reward[:W].unsqueeze(-1).expand(W, T, E, N).permute(2, 3, 0, 1).reshape(E * N, W * T).contiguous()
    done = torch.zeros(W, T, dtype=torch.uint8, device=tr.device)
    done[:, T - 1] = 1
    done = done.view(1, W * T).expand(E * N, W * T).contiguous()
    td, dr = torch.empty_like(rew), torch.empty_like(rew)
    tr.env.ctx.call("ippm_td_lambda", _ffi.ptr(rew), _ffi.ptr(done), _ffi.ptr(q), _ffi.ptr(td), _ffi.ptr(dr), E * N, W * T, tr.env.stream)
    torch.cuda.synchronize()
    return td.view(E, N, W, T).permute(2, 3, 0, 1).reshape(-1)


def _within_margin(got, net, states, actions=None):
    """max |got - emulate(float64)| <= MARGIN spreads of ``net`` on ``states``; -> (error, spread, emulate(float64))."""
    d, q64 = R.spread(net, states.cpu())
    want = q64 if actions is None else R.gather(q64, actions.cpu())
    err = float((got.cpu().double() - want).abs().max())
    assert err <= R.MARGIN * d, (err, d)
    return err, d, q64


def test_td_targets_come_from_the_native_target(monkeypatch):
    from ippmarl.critic_native import NativeCritic
    monkeypatch.delenv("IPPMARL_CRITIC_INFERENCE", raising=False)
    tr = _trainer(critic_inference="native")
    assert (tr.env.d.grid_x, tr.env.d.grid_y, tr.E, tr.N, tr.waves_per_update) == (64, 64, 3, 2, 1)
    assert tr.rollout("train")["faults"] == 0
    states, actions = _buffer(tr)
    td, _ = tr.td_targets()
    q_sel = NativeCritic(tr.frozen_target, DEV).forward(states, actions)[1]
    assert torch.equal(td, _td_lambda(tr, q_sel))
    err, d, _ = _within_margin(q_sel, R.module_net(tr.frozen_target), states, actions)
    print(f"frozen target: spread {d:.3e} error {err:.3e}")
    # the frozen copy does not follow the critic
    with torch.no_grad():
        tr.critic.fc3.bias.add_(1.0)
    tr.critic_learner.update_target_network(0, 0)
    assert torch.equal(tr.td_targets()[0], td)


def test_fixed_quirk_targets_follow_a_hard_target_update(monkeypatch):
    from ippmarl.critic_native import NativeCritic
    monkeypatch.delenv("IPPMARL_CRITIC_INFERENCE", raising=False)
    tr = _trainer(seed=6, critic_inference="native", quirks="fixed")
    assert tr.rollout("train")["faults"] == 0
    states, actions = _buffer(tr)
    td1, _ = tr.td_targets()
    target = tr.critic_learner.target_critic
    assert torch.equal(td1, _td_lambda(tr, NativeCritic(target, DEV).forward(states, actions)[1]))
    with torch.no_grad():                            # the critic moves; a hard copy takes the target along
        tr.critic.fc3.weight.mul_(-2.0)
        tr.critic.fc3.bias.add_(0.5)
    tr.critic_learner.update_target_network(0, 0)
    td2, _ = tr.td_targets()
    q_sel = NativeCritic(target, DEV).forward(states, actions)[1]
    _within_margin(q_sel, R.module_net(target), states, actions)
    assert not torch.equal(td1, td2)
    assert torch.equal(td2, _td_lambda(tr, q_sel))          # (a stale pack would still give td1)


def test_post_step_q_follows_the_step(monkeypatch):
    monkeypatch.delenv("IPPMARL_CRITIC_INFERENCE", raising=False)
    tr = _trainer(seed=7, params=_params64(networks__critic__learning_rate=1e-3), critic_inference="native")
    assert tr.rollout("train")["faults"] == 0
    states, actions = (x.clone() for x in _buffer(tr))
    td, _ = tr.td_targets()
    old = R.module_net(tr.critic)
    _, q_new = tr.critic_learner.step(states, actions, td)
    new = R.module_net(tr.critic)
    assert q_new.shape == (states.shape[0], tr.A)
    d_new, q64_new = R.spread(new, states.cpu())
    _, q64_old = R.spread(old, states.cpu())
    moved = float((q64_old - q64_new).abs().max())
    err_new = float((q_new.cpu().double() - q64_new).abs().max())
    err_old = float((q_new.cpu().double() - q64_old).abs().max())
    print(f"spread {d_new:.3e}; the step moved Q by {moved:.3e}; error vs new weights {err_new:.3e}, vs old weights {err_old:.3e}")
    assert moved > 10 * R.MARGIN * d_new            # precondition, on the CPU emulations alone: a stale pack cannot pass
    assert err_new <= R.MARGIN * d_new, (err_new, d_new)
    assert err_old > err_new
    # diagnostics keep the float32 module (the metrics need logp): the hook is not called
    calls = []
    monkeypatch.setattr(tr._native_critic, "after_step", lambda s: calls.append(s))
    tr.critic_learner.collect = True
    _, q_diag = tr.critic_learner.step(states, actions, td)
    assert not calls and q_diag is tr.critic_learner.last["q_new"] and "logp_chosen" in tr.critic_learner.last
    tr.critic_learner.collect = False
    tr.critic_learner.step(states, actions, td)
    assert len(calls) == 1


def _copy_training_state(src, dst):
    with torch.no_grad():
        for net in ("actor", "critic"):
            for p_dst, p_src in zip(getattr(dst, net).parameters(), getattr(src, net).parameters()):
                p_dst.copy_(p_src)
        for learner in ("actor_learner", "critic_learner"):
            src_opt, dst_opt = getattr(src, learner).optimizer, getattr(dst, learner).optimizer
            for g_src, g_dst in zip(src_opt.param_groups, dst_opt.param_groups):
                for p_src, p_dst in zip(g_src["params"], g_dst["params"]):
                    for k, v in src_opt.state.get(p_src, {}).items():
                        dst_opt.state[p_dst][k].copy_(v)
        for p_dst, p_src in zip(dst.critic_learner.target_critic.parameters(), src.critic_learner.target_critic.parameters()):
            p_dst.copy_(p_src)


def _flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()])


def _run_recorded_rounds():
    """Two rounds of a trainer replayed from hipGraphs beside the same rounds run launch by launch (twice: a second eager trainer shows
    how far two launch-by-launch runs are apart), all with critic_inference="native".  Every round starts from identical training state
    (weights, Adam moments and counters, target network), copied in place from the host AFTER the recorded trainer's last pack and --
    for the first round -- before capture_graphs(), so the recorded forwards only see it if the capture synced the packs.
    copy_rate = 2: the second compared round (train step 2) crosses a hard target copy.
    -> per round: the buffers of (eager, recorded) and {net: flat parameters of (eager, second eager, recorded)}."""
    saved = os.environ.pop("IPPMARL_CRITIC_INFERENCE", None)
    try:
        params = _params64(networks__copy_rate=2)
        eager, eager2, rec = (_trainer(seed=11, params=params, graphs=True, critic_inference="native") for _ in range(3))
        for tr in (eager, eager2, rec):          # first round launch by launch (kernel selection, allocator)
            torch.manual_seed(12)
            tr.rollout("train")
            tr.update()
        rounds = []
        for rnd in range(2):
            for tr in (eager2, rec):
                _copy_training_state(eager, tr)
            if rnd == 0:
                rec.capture_graphs()
            assert eager.train_step == rec.train_step == 1 + rnd and (eager.train_step % 2 == 0) == bool(rnd)
            bufs, before = [], {net: _flat(getattr(eager, net)).clone() for net in ("critic", "actor")}
            for tr in (eager, eager2, rec):
                torch.manual_seed(20 + rnd)
                assert tr.rollout("train")["faults"] == 0
                bufs.append({k: getattr(tr, k).clone() for k in ("buf_state", "buf_action", "buf_reward")})
                stats = tr.update()
                assert np.isfinite(stats["critic_loss"]) and np.isfinite(stats["actor_loss"])
            rounds.append(dict(bufs=(bufs[0], bufs[2]),
                               nets={net: tuple(_flat(getattr(tr, net)).clone() for tr in (eager, eager2, rec)) for net in ("critic", "actor")},
                               before=before))
        return rounds
    finally:
        if saved is not None:
            os.environ["IPPMARL_CRITIC_INFERENCE"] = saved


@pytest.fixture(scope="module")
def recorded_rounds(tmp_path_factory):
    """The digests tests/critic_recorded_rounds.py writes: ``_run_recorded_rounds`` in a process of its own, with the convolution library
    in deterministic mode (the default float32 weight-gradient kernels sum with float atomics: two launch-by-launch rounds from the same
    bits then differ in the last bits -- measured 3e-8 ... 2e-4 over a net's parameters -- and a bit-for-bit comparison would say
    nothing about the replay; the mode depends on environment variables the library reads once per process)."""
    out = tmp_path_factory.mktemp("critic_rounds") / "digests.json"
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "critic_recorded_rounds.py")
    env = {k: v for k, v in os.environ.items() if k != "IPPMARL_CRITIC_INFERENCE"}
    run = subprocess.run([sys.executable, script, str(out)], env=env, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with open(out) as f:
        return json.load(f)


def test_recorded_native_critic_round_flies_the_eager_round(recorded_rounds):
    """The replayed rollouts wrote the transitions of the launch-by-launch ones bit for bit (states, actions, rewards), in both rounds
    (the first one on weights that were written from the host just before the capture)."""
    assert len(recorded_rounds) == 2
    for rnd, r in enumerate(recorded_rounds):
        for k, (eager, rec) in r["bufs"].items():
            assert eager == rec, (rnd, k)


def test_recorded_native_critic_round_equals_eager_round(recorded_rounds):
    """The parameters of both nets after each of the two rounds, recorded against launch by launch, bit for bit (equal SHA-256 digests
    of their bytes), with the convolution library in deterministic mode.  Premises, asserted: two launch-by-launch trainers agree bit
    for bit there (so a difference would be the replay's), every parameter is finite, and each round moved both nets."""
    for rnd, r in enumerate(recorded_rounds):
        for net, n in r["nets"].items():
            print(f"round {rnd} {net}: {n['differ_recorded']} of {n['numel']} parameters differ eager - recorded (max {n['max_recorded']:.3e}); "
                  f"{n['differ_eager']} eager - second eager (max {n['max_eager']:.3e}); the round moved them by up to {n['moved']:.3e}")
    for rnd, r in enumerate(recorded_rounds):
        for net, n in r["nets"].items():
            eager, eager2, rec = n["digests"]
            assert n["finite"] and n["moved"] > 0, (rnd, net)
            assert eager == eager2 and n["differ_eager"] == 0, (rnd, net, n)
            assert eager == rec and n["differ_recorded"] == 0, (rnd, net, n)


def test_weights_written_before_a_capture_reach_the_critic_forwards(monkeypatch):
    """Critic parameters written from the host between the last executed pack and capture_graphs(): the forwards after the capture run on
    the NEW weights; and with quirks="fixed" a replayed update leaves the target's pack equal to a fresh pack of the target network (the
    hard copy is a host-side write ahead of the replay)."""
    from ippmarl.critic_native import NativeCritic
    monkeypatch.delenv("IPPMARL_CRITIC_INFERENCE", raising=False)
    tr = _trainer(seed=13, params=_params64(networks__copy_rate=1), graphs=True, critic_inference="native", quirks="fixed")
    torch.manual_seed(14)
    tr.rollout("train")
    tr.update()
    tr.rollout("train")
    states, actions = (x.clone() for x in _buffer(tr))
    old = R.module_net(tr.critic)
    tr._native_critic.forward(states)                # the pack is current for the old weights
    with torch.no_grad():                            # (what a load_state_dict does: in-place copies)
        tr.critic.fc3.weight.copy_(-3.0 * tr.critic.fc3.weight)
        tr.critic.fc3.bias.copy_(tr.critic.fc3.bias + 0.5)
    tr.capture_graphs()
    got = tr._native_critic._forward(states, None, True)[0]          # (no version check: what a recorded launch would read)
    new = R.module_net(tr.critic)
    err, d, q64 = _within_margin(got, new, states)
    stale = float((R.emulate(old, states.cpu(), torch.float64) - q64).abs().max())
    print(f"spread {d:.3e} error vs the new weights {err:.3e}; the old weights are {stale:.3e} away")
    assert stale > 2 * R.MARGIN * d
    # a replayed round: the hard copy ahead of the replay reaches the target's pack, the recorded repacks reach the critic's
    tr.update()
    for native, module in ((tr._native_target, tr.critic_learner.target_critic), (tr._native_critic, tr.critic)):
        assert native.module is module
        fresh = NativeCritic(module, DEV).forward(states, actions)
        held = native._forward(states, actions, True)
        assert torch.equal(held[0], fresh[0]) and torch.equal(held[1], fresh[1])
    _within_margin(tr._native_critic._forward(states, None, True)[0], R.module_net(tr.critic), states)


def _spy(monkeypatch, module):
    """Records (input, output) of every forward of ``module`` from here on."""
    seen, forward = [], module.forward

    def spy(x):
        out = forward(x)
        seen.append((x, out))
        return out

    monkeypatch.setattr(module, "forward", spy)
    return seen


def test_default_is_pytorch(monkeypatch):
    """Switch off: no NativeCritic exists, and the TD targets and the post-step Q are the bits the float32 modules returned -- their
    own outputs are taken at the call (two float32 forwards of one module need not agree in the last bit: the library may choose
    another kernel for the second)."""
    monkeypatch.delenv("IPPMARL_CRITIC_INFERENCE", raising=False)
    tr = _trainer(seed=15)
    assert tr.critic_inference == "torch" and tr._native_critic is None and tr._native_target is None and tr.critic_learner.inference is None
    assert tr.rollout("train")["faults"] == 0
    states, actions = (x.clone() for x in _buffer(tr))
    target_calls = _spy(monkeypatch, tr.frozen_target)
    td, _ = tr.td_targets()
    assert len(target_calls) == 1 and torch.equal(target_calls[0][0], states)
    q = target_calls[0][1][0]
    assert q.dtype == torch.float32 and q.shape == (states.shape[0], tr.A)
    assert torch.equal(td, _td_lambda(tr, R.gather(q, actions)))
    critic_calls = _spy(monkeypatch, tr.critic)
    _, q_new = tr.critic_learner.step(states, actions, td)
    assert len(critic_calls) == 2 and q_new is critic_calls[1][1][0]          # (the loss' forward, then the post-step one)
    assert torch.equal(critic_calls[1][0], states)
    assert tr._native_critic is None and tr._native_target is None
    with pytest.raises(ValueError, match="critic inference"):
        _trainer(critic_inference="fast")
    monkeypatch.setenv("IPPMARL_CRITIC_INFERENCE", "bf16")
    with pytest.raises(ValueError, match="critic inference"):
        _trainer()
    monkeypatch.setenv("IPPMARL_CRITIC_INFERENCE", "native")
    tr = _trainer()
    assert tr.critic_inference == "native" and tr.actor_inference == "torch" and tr._native_critic is not None
