"""K1 on the device (csrc/ippm_k1.h::k1_env) against the constructed scenes of tests/k1_scenes.py, whose expected masks, actions, positions
and fault words come from the oracle alone (census: tests/test_k1_scenes_cpu.py).  Every comparison is bit for bit.

Two launch forms of the same device code:
  alone     ``ippm_mask_act_move`` on a bare context (``IPPM_STEP_MOVE`` only; touches no map): every scene, the ones whose move leaves the
            lattice included (policy 3 when every valid action has probability 0);
  combined  ``VecEnv.steps`` without ``build_observations`` (``COMM | GLOBAL | MOVE`` in one launch, K1 beside the planning wavefront and
            the tile builders, ``track_area=False``): the explicit and the uniform policy -- ``steps`` admits a learned policy only after
            ``build_observations``, which makes its launch the MOVE-only one again.
The policy and t are arguments of a launch: the scenes of an action set run as one batch per (team capacity, policy, t)."""
import numpy as np
import pytest

import k1_scenes as K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(x, dtype=None):
    return None if x is None else torch.as_tensor(x, dtype=dtype).contiguous().to(DEV)


def _alone(A, N, policy, t, arr, teams=False):
    from ippmarl import _ffi
    from ippmarl.derived import DerivedConstants
    ctx = _ffi.Context(DerivedConstants(K.params_for(A, N), philox_seed=K.SEED))
    try:
        E = len(arr["pos"])
        stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
        episode, pos, fault = _dev(arr["episode"]), _dev(arr["pos"]), _dev(arr["fault0"])
        probs, actions = _dev(arr["probs"]), _dev(arr["actions"])
        n_active = _dev(arr["n_active"]) if teams else None
        mask = torch.full((E, N, A), 0xA5, dtype=torch.uint8, device=DEV)
        action = torch.full((E, N), -7, dtype=torch.int32, device=DEV)
        assert pos.shape == (E, N, 3) and (probs is None or probs.shape == (E, N, A)) and (actions is None or actions.shape == (E, N))
        if teams:
            ctx.call("ippm_set_team_sizes", _ffi.ptr(n_active))
        ctx.call("ippm_mask_act_move", _ffi.ptr(episode), _ffi.ptr(pos), _ffi.ptr(probs), _ffi.ptr(actions), policy, t, _ffi.ptr(mask),
                 _ffi.ptr(action), _ffi.ptr(fault), E, stream)
        torch.cuda.synchronize()
        return dict(mask=mask.cpu().numpy(), action=action.cpu().numpy(), pos=pos.cpu().numpy(), fault=fault.cpu().numpy())
    finally:
        ctx.close()


def _combined(A, N, policy, t, arr, teams=False):
    from ippmarl.vec_env import VecEnv
    E = len(arr["pos"])
    env = VecEnv(K.params_for(A, N), E, philox_seed=K.SEED, track_area=False, team_sizes=arr["n_active"] if teams else None)
    env.reset(np.arange(1, E + 1), start_positions=torch.from_numpy(arr["pos"]))
    env.episode.copy_(torch.from_numpy(arr["episode"]))          # (ids beyond what the start-state generator admits: K1 only keys Philox with them)
    env.fault.copy_(torch.from_numpy(arr["fault0"]))
    env.steps(t, policy=policy, actions=None if arr["actions"] is None else torch.from_numpy(arr["actions"]), features=False)
    torch.cuda.synchronize()
    assert env.counters()["work_list_rejects"] == 0
    return dict(mask=env.mask.cpu().numpy(), action=env.action.cpu().numpy(), pos=env.pos.cpu().numpy(), fault=env.fault.cpu().numpy())


def _check(got, arr, tag):
    fly = arr["flying"]
    for name, want in (("pos", arr["want_pos"]), ("fault", arr["want_fault"])):
        bad = np.flatnonzero((got[name] != want).reshape(len(want), -1).any(axis=1))
        assert bad.size == 0, (tag, name, bad[:8].tolist(), got[name][bad[0]].tolist(), want[bad[0]].tolist())
    # (rows of agents that do not fly are not written: not compared)
    bad = np.flatnonzero(((got["mask"] != arr["want_mask"]) & fly[:, :, None]).any(axis=(1, 2)))
    assert bad.size == 0, (tag, "mask", bad[:8].tolist(), got["mask"][bad[0]].tolist(), arr["want_mask"][bad[0]].tolist())
    bad = np.flatnonzero(((got["action"] != arr["want_action"]) & fly).any(axis=1))
    assert bad.size == 0, (tag, "action", bad[:8].tolist(), got["action"][bad[0]].tolist(), arr["want_action"][bad[0]].tolist())


def _same(a, b, arr, tag):
    fly = arr["flying"]
    assert np.array_equal(a["pos"], b["pos"]) and np.array_equal(a["fault"], b["fault"]), tag
    assert not ((a["mask"] != b["mask"]) & fly[:, :, None]).any() and not ((a["action"] != b["action"]) & fly).any(), tag


@pytest.mark.parametrize("A", K.ACTION_SETS)
def test_k1_alone_matches_the_oracle_on_every_scene(A):
    seen = 0
    for (N, policy, t), idx in sorted(K.groups(A).items()):
        arr = K.batch_arrays(A, "all", idx)
        _check(_alone(A, N, policy, t, arr), arr, (A, N, policy, t))
        seen += len(idx)
    assert seen == len(K.scenes(A))      # no scene is left out


@pytest.mark.parametrize("A", K.ACTION_SETS)
def test_k1_in_the_combined_launch_matches_the_oracle_and_the_alone_form(A):
    seen = 0
    for (N, policy, t), idx in sorted(K.groups(A).items()):
        if policy not in (K.POLICY_EXPLICIT, K.POLICY_UNIFORM):
            continue
        arr = K.batch_arrays(A, "all", idx)
        assert all(K.on_lattice(A, p) for p in arr["want_pos"])     # (this form projects the footprints of the new positions)
        got = _combined(A, N, policy, t, arr)
        _check(got, arr, (A, N, policy, t))
        _same(got, _alone(A, N, policy, t, arr), arr, (A, N, policy, t))
        seen += len(idx)
    assert seen == sum(sc.policy in (K.POLICY_EXPLICIT, K.POLICY_UNIFORM) for sc in K.scenes(A))


@pytest.mark.parametrize("A", [6, 27])
def test_k1_with_team_sizes(A):
    """n_active[e] < N: the agents that do not fly keep their positions and raise no fault bit, in both launch forms."""
    for (N, policy, t), idx in sorted(K.groups(A, "teams").items()):
        arr = K.batch_arrays(A, "teams", idx)
        assert N == 4 and set(arr["n_active"]) == {1, 2, 3, 4}
        alone = _alone(A, N, policy, t, arr, teams=True)
        _check(alone, arr, (A, "teams", policy, t))
        # (the alone form leaves the rows of the others untouched)
        assert (alone["mask"][~arr["flying"]] == 0xA5).all() and (alone["action"][~arr["flying"]] == -7).all()
        got = _combined(A, N, policy, t, arr, teams=True)
        _check(got, arr, (A, "teams", policy, t))
        _same(got, alone, arr, (A, "teams", policy, t))
