"""CPU side of the native critic inference checks: the constructions the GPU tests rely on (tests/test_hip_critic_native.py) hold by the
emulation alone, and the critic's inference switch parses as documented."""
import pytest

torch = pytest.importorskip("torch")

import critic_native_ref as R  # noqa: E402


def test_exact_network_is_exact_and_varied():
    """Sparse integer weights, {0,1} biases and states: every activation of every layer is an integer of magnitude <= 255 (exact in
    bf16, and in float32 in any summation order), so emulate(float32) == emulate(float64) bit for bit -- and the Q rows differ from
    sample to sample."""
    a32 = R.exact_activations(R.EXACT_SEED, R.EXACT_BATCH, torch.float32)
    a64 = R.exact_activations(R.EXACT_SEED, R.EXACT_BATCH, torch.float64)
    for layer, (h32, h64) in enumerate(zip(a32, a64)):
        assert torch.equal(h32.double(), h64), layer
        assert torch.equal(h64, h64.round()) and float(h64.abs().max()) <= 255, (layer, float(h64.abs().max()))
    assert float(a64[-1].max()) > 1
    for A in (6, 27):
        q32 = R.exact_q(R.EXACT_SEED, R.EXACT_BATCH, A, torch.float32)
        q64 = R.exact_q(R.EXACT_SEED, R.EXACT_BATCH, A, torch.float64)
        assert torch.equal(q32.double(), q64), A
        assert torch.equal(q64, q64.round()) and float(q64.abs().max()) <= 255, A
        assert len({tuple(r.tolist()) for r in q64}) >= 0.9 * R.EXACT_BATCH, A
        acts = R.exact_actions(R.EXACT_SEED, R.EXACT_BATCH, A)
        assert int(acts.min()) == 0 and int(acts.max()) == A - 1


def test_exact_network_uses_every_plane_and_kernel_row():
    """conv1's non-zeros reach every input plane, every kernel row and column: a gather that mixed up the 60-float kernel rows, the
    132-float row stride or the channel order would read other states."""
    w = R.exact_net(R.EXACT_SEED, 6)["conv1"][0]
    assert w.shape == (256, 12, 5, 5)
    nz = w.ne(0)
    assert bool(nz.any(dim=0).any(dim=1).any(dim=1).all())      # planes
    assert bool(nz.any(dim=0).any(dim=0).all())                  # taps


@pytest.mark.parametrize("seed", R.DENSE_SEEDS)
def test_dense_spread_is_a_usable_unit(seed):
    """The float32 / float64 spread comes from activations that round to the other bf16 neighbour (relative step 2^-8): it is not
    zero, and it stays below two such steps of the largest Q (one flip each way), so MARGIN spreads still tell a wrong forward from a right one."""
    for A in (6, 27):
        d, q64 = R.dense_spread(seed, A)
        print(f"seed {seed} A {A}: spread {d:.3e}, |Q| up to {float(q64.abs().max()):.3f}")
        assert 0 < d < 2.0 ** -7 * float(q64.abs().max())


def test_critic_switch_parsing(monkeypatch):
    import inspect

    from ippmarl import actor_native
    from ippmarl.critic_native import ENV_VAR, resolve_mode
    from ippmarl.trainer import COMATrainer
    assert ENV_VAR == "IPPMARL_CRITIC_INFERENCE"
    monkeypatch.delenv(ENV_VAR, raising=False)
    monkeypatch.delenv(actor_native.ENV_VAR, raising=False)
    assert resolve_mode() == "torch" and resolve_mode(None) == "torch"
    assert resolve_mode("native") == "native" and resolve_mode("torch") == "torch"
    monkeypatch.setenv(ENV_VAR, "native")
    assert resolve_mode() == "native"
    assert resolve_mode("torch") == "torch"          # the argument wins over the environment
    assert actor_native.resolve_mode() == "torch"    # the two switches are independent
    monkeypatch.setenv(ENV_VAR, "")
    assert resolve_mode() == "torch"
    monkeypatch.setenv(ENV_VAR, "bf16")
    with pytest.raises(ValueError, match="critic inference"):
        resolve_mode()
    with pytest.raises(ValueError, match="critic inference"):
        resolve_mode("fast")
    assert inspect.signature(COMATrainer.__init__).parameters["critic_inference"].default is None


def test_native_critic_is_gpu_only():
    from ippmarl import _ffi
    from ippmarl.critic_native import NativeCritic
    with pytest.raises(_ffi.IppmError, match="GPU only"):
        NativeCritic(object(), "cpu")
