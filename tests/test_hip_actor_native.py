"""GPU checks of the native bf16 actor inference (csrc/actor_infer.hip behind ippm_actor_pack / ippm_actor_forward, NativeActor, the
trainer's ``actor_inference="native"``).  The reference of every numerical check is the CPU restatement of the contract in
tests/actor_native_ref.py (``emulate``), never the code under test."""
import ctypes as C

import functools

import numpy as np
import pytest
import torch

import actor_native_ref as R
from configs import make_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = 128            # rows of a workgroup tile of the layer kernel: batch rows next to its edges are the ones worth sampling


@functools.lru_cache(maxsize=None)
def _slice():
    """Samples per internal slice of ippm_actor_forward, read off the library: the batch at which the scratch stops growing."""
    from ippmarl import _ffi
    lib = _ffi.load_library()

    def nbytes(batch):
        out = C.c_int64(0)
        _ffi.check(lib.ippm_actor_scratch_bytes(batch, C.addressof(out)), "ippm_actor_scratch_bytes")
        return out.value

    per_sample, most = nbytes(1), nbytes(1 << 40)
    n = most // per_sample
    assert most == n * per_sample and nbytes(n) == most and nbytes(n - 1) < most and n <= 8192
    return n


def _pack(net, A):
    from ippmarl import _ffi
    lib = _ffi.load_library()
    nbytes = C.c_int64(0)
    _ffi.check(lib.ippm_actor_pack_bytes(A, C.addressof(nbytes)), "ippm_actor_pack_bytes")
    packed = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device=DEV)
    dev = [t.to(DEV).contiguous() for name in R.TRUNK + ("fc3",) for t in net[name]]
    _ffi.check(lib.ippm_actor_pack(*[t.data_ptr() for t in dev], A, packed.data_ptr(), torch.cuda.current_stream().cuda_stream), "ippm_actor_pack")
    torch.cuda.synchronize()
    return packed


def _forward(packed, obs, A, eps=0.0, eps_dev=None, want_logits=True):
    """ippm_actor_forward on outputs AND scratch pre-filled with NaN -> (probs, logits) on the CPU."""
    from ippmarl import _ffi
    lib = _ffi.load_library()
    obs = obs.to(DEV).contiguous()
    B = obs.shape[0]
    nbytes = C.c_int64(0)
    _ffi.check(lib.ippm_actor_scratch_bytes(B, C.addressof(nbytes)), "ippm_actor_scratch_bytes")
    assert nbytes.value <= _slice() * 34304         # bounded by the slice, whatever the batch
    scratch = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device=DEV)     # bf16 0xFFFF: NaN
    probs = torch.full((B, A), float("nan"), device=DEV)
    logits = torch.full((B, A), float("nan"), device=DEV) if want_logits else None
    _ffi.check(lib.ippm_actor_forward(packed.data_ptr(), obs.data_ptr(), B, A, float(eps), _ffi.ptr(eps_dev), scratch.data_ptr(),
                                      probs.data_ptr(), _ffi.ptr(logits), torch.cuda.current_stream().cuda_stream), "ippm_actor_forward")
    torch.cuda.synchronize()
    return probs.cpu(), None if logits is None else logits.cpu()


@pytest.fixture(scope="module")
def exact_packs():
    return {A: _pack(R.exact_net(R.EXACT_SEED, A), A) for A in (6, 27)}


# ---- 1. exact network: pins every index ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [6, 27])
def test_exact_network_bit_for_bit(exact_packs, A):
    obs = R.exact_obs(R.EXACT_SEED, R.EXACT_BATCH)
    want = R.exact_logits(R.EXACT_SEED, R.EXACT_BATCH, A)
    for eps in (0.0, 0.3):
        ref = R.mix(want, eps)
        for through_dev in (False, True):
            eps_dev = torch.full((), eps, dtype=torch.float32, device=DEV) if through_dev else None
            probs, logits = _forward(exact_packs[A], obs, A, eps=-1.0 if through_dev else eps, eps_dev=eps_dev)
            assert torch.equal(logits.double(), want), (A, eps, through_dev, int((logits.double() != want).sum()))
            err = float((probs.double() - ref).abs().max())
            assert err <= 1e-6, (A, eps, through_dev, err)
    probs, none = _forward(exact_packs[A], obs, A, want_logits=False)      # logits may be NULL
    assert none is None and float((probs.double() - R.mix(want, 0.0)).abs().max()) <= 1e-6


# ---- 2. batch shapes and determinism ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 63, 64, 65, 257, "slice + 1"])
def test_batch_shapes_and_determinism(exact_packs, B):
    A = 6
    B = _slice() + 1 if B == "slice + 1" else B
    base_obs, base = R.exact_obs(R.EXACT_SEED, R.EXACT_BATCH), R.exact_logits(R.EXACT_SEED, R.EXACT_BATCH, A)
    rows = torch.arange(B) % R.EXACT_BATCH                 # (beyond 300 samples the observations repeat: the reference is shared)
    obs, want = base_obs[rows], base[rows]
    probs, logits = _forward(exact_packs[A], obs, A, eps=0.3)
    assert not torch.isnan(probs).any() and not torch.isnan(logits).any()
    assert torch.equal(logits.double(), want)
    assert float((probs.double() - R.mix(want, 0.3)).abs().max()) <= 1e-6
    probs2, logits2 = _forward(exact_packs[A], obs, A, eps=0.3)
    assert torch.equal(probs, probs2) and torch.equal(logits, logits2)           # run to run
    # alone == in the batch: the first and last row, the rows on either side of the first tile edge and of the slice boundary
    for r in sorted(r for r in {0, TILE - 1, TILE, 2 * TILE, _slice() - 1, _slice(), B - 2, B - 1} if 0 <= r < B):
        p1, l1 = _forward(exact_packs[A], obs[r:r + 1], A, eps=0.3)
        assert torch.equal(p1[0], probs[r]) and torch.equal(l1[0], logits[r]), (B, r)


# ---- 3. dense network ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense_runs():
    cache = {}

    def run(seed, A):
        if (seed, A) not in cache:
            net = R.dense_net(seed, A)
            cache[seed, A] = _forward(_pack(net, A), R.dense_obs(seed, R.DENSE_BATCH), A)
        return cache[seed, A]

    return run


@pytest.mark.parametrize("seed", R.DENSE_SEEDS)
@pytest.mark.parametrize("A", [6, 27])
def test_dense_network_within_four_spreads(dense_runs, seed, A):
    d_logits, d_probs, l64, p64 = R.spreads(seed, A)
    probs, logits = dense_runs(seed, A)
    e_logits, e_probs = float((logits.double() - l64).abs().max()), float((probs.double() - p64).abs().max())
    # information: where the float32 PyTorch module (the default path) sits against the same reference
    from ippmarl.networks import ActorNetwork
    module = ActorNetwork(make_params("small", experiment__constraints__num_actions=A))
    with torch.no_grad():
        for name, (w, b) in R.dense_net(seed, A).items():
            getattr(module, name).weight.copy_(w)
            getattr(module, name).bias.copy_(b)
        module = module.to(DEV)
        p_mod = module(R.dense_obs(seed, R.DENSE_BATCH).to(DEV), 0.0)[0].cpu()
    print(f"seed {seed} A {A}: spread logits {d_logits:.3e} probs {d_probs:.3e}; device error logits {e_logits:.3e} probs {e_probs:.3e}; "
          f"float32 module vs reference probs {float((p_mod.double() - p64).abs().max()):.3e}")
    assert e_logits <= R.MARGIN * d_logits, (e_logits, d_logits)
    assert e_probs <= R.MARGIN * d_probs, (e_probs, d_probs)


# ---- 4. decisions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.DENSE_SEEDS)
def test_decisions_follow_the_reference(dense_runs, seed):
    from ippmarl import _ffi
    from ippmarl.derived import DerivedConstants
    A = 6
    _, d_probs, _, p64 = R.spreads(seed, A)
    probs, _ = dense_runs(seed, A)
    params = make_params("small", experiment__missions__n_agents=2)
    d = DerivedConstants(params)
    assert d.n_actions == A
    ctx = _ffi.Context(d)
    E = R.DENSE_BATCH // 2
    # mid-altitude interior lattice points, far apart: every action of both agents is valid
    z = d.min_altitude + d.spacing
    pos = torch.tensor([[2 * d.spacing, 2 * d.spacing, z], [5 * d.spacing, 5 * d.spacing, z]], dtype=torch.int32).repeat(E, 1, 1).to(DEV).contiguous()
    episode = torch.arange(1, E + 1, dtype=torch.int64, device=DEV)
    mask = torch.zeros(E, 2, A, dtype=torch.uint8, device=DEV)
    action = torch.full((E, 2), -1, dtype=torch.int32, device=DEV)
    fault = torch.zeros(E, dtype=torch.int32, device=DEV)
    p_dev = probs.to(DEV).view(E, 2, A).contiguous()
    ctx.call("ippm_mask_act_move", episode.data_ptr(), pos.data_ptr(), p_dev.data_ptr(), None, 3, 0, mask.data_ptr(), action.data_ptr(),
             fault.data_ptr(), E, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool(mask.all()) and not bool(fault.any())
    chosen = action.view(-1).cpu().long()
    want = p64.argmax(dim=1)
    pinned = R.top2_gap(p64) >= 2 * R.MARGIN * d_probs
    excused = 1.0 - float(pinned.double().mean())
    print(f"seed {seed}: excused {excused:.3%}, disagreements among them {int((chosen != want)[~pinned].sum())}")
    assert excused <= R.EXCUSED_CAP
    assert torch.equal(chosen[pinned], want[pinned]), int((chosen != want)[pinned].sum())


# ---- 5. trainer ---------------------------------------------------------------------------------------------------------------------
def _params64():
    """2 UAVs on a 64 x 64 grid: the 50 m world and its 11 x 11 lattice (the networks need it) at a 99 degree field of view, whose cell
    is 0.78 m."""
    return make_params("small", experiment__missions__n_agents=2, sensor__field_of_view__angle_x=99.0, sensor__field_of_view__angle_y=99.0)


def _trainer(seed=5, **kw):
    from ippmarl.trainer import COMATrainer
    torch.manual_seed(seed)
    return COMATrainer(_params64(), n_envs=4, first_episode=3, **kw)


def test_trainer_flies_the_emulated_argmax(monkeypatch):
    from ippmarl.vec_env import POLICY_EXPLICIT
    monkeypatch.delenv("IPPMARL_ACTOR_INFERENCE", raising=False)
    tr = _trainer(actor_inference="native")
    assert (tr.env.d.grid_x, tr.env.d.grid_y, tr.E, tr.N) == (64, 64, 4, 2)
    episodes = [21, 22, 23, 24]
    curves = tr.curves_on(episodes, "actor")
    returns = tr.returns_on(episodes, "actor")
    flown = curves["actions"]                                                    # [T,E,N]
    assert int(curves["faults"].abs().sum()) == 0
    np.testing.assert_allclose(returns["episode_return"], float(curves["episode_return"].mean()), rtol=1e-6)
    # replay on the oracle side: follow the flown trajectory, predict every decision from emulate(float64) on the observations of the step
    net = R.module_net(tr.actor)
    env = tr.env
    env.reset(torch.as_tensor(episodes, dtype=torch.int64))
    checked = excused = 0
    for t in range(tr.T):
        obs = env.build_observations(t).view(-1, 11, 11, 7).cpu()
        p64 = R.mix(R.emulate(net, obs, torch.float64), 0.0)
        p32 = R.mix(R.emulate(net, obs, torch.float32), 0.0)
        d_probs = float((p32.double() - p64).abs().max())
        env.steps(t, policy=POLICY_EXPLICIT, actions=flown[t], features=False)
        masked = p64 * env.mask.view(-1, tr.A).cpu().double()
        pinned = R.top2_gap(masked) >= 2 * R.MARGIN * d_probs
        got = flown[t].view(-1).cpu().long()
        assert torch.equal(got[pinned], masked.argmax(dim=1)[pinned]), t
        checked += int(pinned.numel())
        excused += int((~pinned).sum())
    print(f"excused {excused} of {checked} decisions")
    assert excused <= R.EXCUSED_CAP * checked


def test_native_probs_follow_the_update(monkeypatch):
    monkeypatch.delenv("IPPMARL_ACTOR_INFERENCE", raising=False)
    tr = _trainer(actor_inference="native")
    tr.rollout("train")
    obs = tr.buf_obs[0, 3].clone()                                                 # [E,N,11,11,7] of a flown step
    old = R.module_net(tr.actor)
    before = tr._act(obs, 0.25).cpu()
    tr.update()
    after = tr._act(obs, 0.25).cpu()
    new = R.module_net(tr.actor)
    o = obs.view(-1, 11, 11, 7).cpu()
    p64, p32 = R.mix(R.emulate(new, o, torch.float64), 0.25), R.mix(R.emulate(new, o, torch.float32), 0.25)
    d = float((p32.double() - p64).abs().max())
    stale = float((R.mix(R.emulate(old, o, torch.float64), 0.25) - p64).abs().max())
    err = float((after.double() - p64).abs().max())
    print(f"spread {d:.3e} error vs updated weights {err:.3e}; the old weights are {stale:.3e} away")
    assert stale > 2 * R.MARGIN * d          # the update moved the policy by more than the tolerance: a stale pack cannot pass
    assert err <= R.MARGIN * d, (err, d)
    assert not torch.equal(before, after)


def test_recorded_native_round_equals_eager_round(monkeypatch):
    monkeypatch.delenv("IPPMARL_ACTOR_INFERENCE", raising=False)
    eager, rec = (_trainer(seed=11, graphs=True, actor_inference="native") for _ in range(2))
    for tr in (eager, rec):          # first round launch by launch (kernel selection, allocator)
        torch.manual_seed(12)
        tr.rollout("train")
        tr.update()
    with torch.no_grad():            # identical training state (as test_hip_learning.test_recorded_round_equals_eager_round)
        for net in ("actor", "critic"):
            for p_dst, p_src in zip(getattr(rec, net).parameters(), getattr(eager, net).parameters()):
                p_dst.copy_(p_src)
        for learner in ("actor_learner", "critic_learner"):
            src_opt, dst_opt = getattr(eager, learner).optimizer, getattr(rec, learner).optimizer
            for g_src, g_dst in zip(src_opt.param_groups, dst_opt.param_groups):
                for p_src, p_dst in zip(g_src["params"], g_dst["params"]):
                    for k, v in src_opt.state.get(p_src, {}).items():
                        dst_opt.state[p_dst][k].copy_(v)
        for p_dst, p_src in zip(rec.critic_learner.target_critic.parameters(), eager.critic_learner.target_critic.parameters()):
            p_dst.copy_(p_src)
    rec.capture_graphs()
    bufs = []
    for tr in (eager, rec):
        torch.manual_seed(20)
        assert tr.rollout("train")["faults"] == 0
        bufs.append({k: getattr(tr, k).clone() for k in ("buf_action", "buf_reward")})
        stats = tr.update()
        assert np.isfinite(stats["critic_loss"]) and np.isfinite(stats["actor_loss"])
    assert torch.equal(bufs[0]["buf_action"], bufs[1]["buf_action"])
    assert torch.equal(bufs[0]["buf_reward"], bufs[1]["buf_reward"])
    # the replayed update repacked: the native probabilities of the recorded trainer follow ITS new weights
    obs = rec.buf_obs[0, 2].clone()
    o = obs.view(-1, 11, 11, 7).cpu()
    net = R.module_net(rec.actor)
    p64, p32 = R.mix(R.emulate(net, o, torch.float64), 0.0), R.mix(R.emulate(net, o, torch.float32), 0.0)
    err = float((rec._act(obs, 0.0).cpu().double() - p64).abs().max())
    assert err <= R.MARGIN * float((p32.double() - p64).abs().max()), err


def test_weights_written_before_a_capture_reach_eager_forwards(monkeypatch):
    """Parameters written from the host between the last executed pack and capture_graphs(): the eager forwards after the capture
    (returns_on, evaluate, _act) run on the NEW weights -- a repack that the captured steps merely record packs nothing."""
    monkeypatch.delenv("IPPMARL_ACTOR_INFERENCE", raising=False)
    tr = _trainer(seed=13, graphs=True, actor_inference="native")
    torch.manual_seed(14)
    tr.rollout("train")
    tr.update()
    obs = tr.buf_obs[0, 4].clone()
    o = obs.view(-1, 11, 11, 7).cpu()
    old = R.module_net(tr.actor)
    tr._act(obs, 0.0)                                # the pack is current for the old weights
    with torch.no_grad():                            # (what a load_state_dict does: in-place copies)
        tr.actor.fc3.weight.copy_(-3.0 * tr.actor.fc3.weight)
        tr.actor.fc3.bias.copy_(-3.0 * tr.actor.fc3.bias)
    tr.capture_graphs()
    got = tr._act(obs, 0.0).cpu().double()
    new = R.module_net(tr.actor)
    p64, p32 = R.mix(R.emulate(new, o, torch.float64), 0.0), R.mix(R.emulate(new, o, torch.float32), 0.0)
    d = float((p32.double() - p64).abs().max())
    stale = float((R.mix(R.emulate(old, o, torch.float64), 0.0) - p64).abs().max())
    err = float((got - p64).abs().max())
    print(f"spread {d:.3e} error vs the new weights {err:.3e}; the old weights are {stale:.3e} away")
    assert stale > 2 * R.MARGIN * d
    assert err <= R.MARGIN * d, (err, d)
    # ... and the recorded steps read the same pack: a replayed round after the capture still runs
    assert tr.rollout("train")["faults"] == 0
    tr.update()
    net = R.module_net(tr.actor)
    q64, q32 = R.mix(R.emulate(net, o, torch.float64), 0.0), R.mix(R.emulate(net, o, torch.float32), 0.0)
    assert float((tr._act(obs, 0.0).cpu().double() - q64).abs().max()) <= R.MARGIN * float((q32.double() - q64).abs().max())


def test_default_switch_is_torch_and_leaves_no_state(monkeypatch):
    monkeypatch.delenv("IPPMARL_ACTOR_INFERENCE", raising=False)
    tr = _trainer()
    assert tr.actor_inference == "torch"
    episodes = [31, 32, 33, 34]
    first = tr.returns_on(episodes, "actor")
    second = tr.returns_on(episodes, "actor")
    assert first == second
    assert tr._native is None
    monkeypatch.setenv("IPPMARL_ACTOR_INFERENCE", "native")
    assert _trainer().actor_inference == "native"


# ---- deployment class -------------------------------------------------------------------------------------------------------------
def test_deployment_honours_the_switch(golden, monkeypatch):
    """actor_native.deployment(..., actor_inference="native"): COMATest flies the recorded reference run (actions forced, so the
    observations are the recording's) with its forward passes in the native kernels, and its own greedy choices are the recorded ones, to
    the standard test_hip_dropin holds the float32 path to (a rare near-tie of the untrained actor may fall the other way)."""
    from conftest import unpack_correctness
    from ippmarl.actor_native import DeployedActor, deployment
    from ippmarl.coma_wrapper import ReplayHooks
    from ippmarl.networks import ActorNetwork
    monkeypatch.delenv("IPPMARL_ACTOR_INFERENCE", raising=False)
    fx = golden("comatest_small3_e9")
    params = make_params("small", experiment__missions__n_agents=3)
    n, corr = 3, unpack_correctness(fx)
    torch.manual_seed(int(fx["net_seed"]))
    net = ActorNetwork(params)
    plain = deployment(params, None, int(fx["episode"]))
    assert plain.actor_inference == "torch" and plain.net is None
    monkeypatch.setenv("IPPMARL_ACTOR_INFERENCE", "native")
    ct = deployment(params, None, int(fx["episode"]))
    assert ct.actor_inference == "native" and isinstance(ct.net, DeployedActor)
    ct.net = DeployedActor(net)
    ct.replay = ReplayHooks(correctness=lambda i, stage: corr[stage * n + i], action=lambda i, t: int(fx["actions"][t * n + i]))
    _, positions, altitudes, _, _, _ = ct.execute("random", int(fx["episode"]))
    assert np.array_equal(np.array(positions), fx["positions"]) and np.array_equal(np.array(altitudes), fx["altitudes"])
    assert np.mean(np.array(ct.greedy_actions) == fx["actions"]) >= 0.9
