"""CPU side of the native actor inference checks: the constructions the GPU tests rely on (tests/test_hip_actor_native.py) hold by the
emulation alone, and the inference switch parses as documented."""
import pytest

torch = pytest.importorskip("torch")

import actor_native_ref as R  # noqa: E402


def test_exact_network_is_exact_and_varied():
    """Sparse integer weights, {0,1} biases and observations: every layer input is a small integer, exact in bf16 and in float32 in any
    summation order, so emulate(float32) == emulate(float64) bit for bit -- and the logit rows differ from sample to sample."""
    for A in (6, 27):
        l32 = R.exact_logits(R.EXACT_SEED, R.EXACT_BATCH, A, torch.float32)
        l64 = R.exact_logits(R.EXACT_SEED, R.EXACT_BATCH, A, torch.float64)
        assert torch.equal(l32.double(), l64), A
        assert torch.equal(l64, l64.round()) and float(l64.abs().max()) <= 256, A
        assert len({tuple(r.tolist()) for r in l64}) >= 0.9 * R.EXACT_BATCH, A
    h = R.exact_hidden(R.EXACT_SEED, R.EXACT_BATCH, torch.float64)
    assert float(h.max()) <= 256 and float(h.max()) > 1     # fc1's activation: integers that bf16 holds exactly


@pytest.mark.parametrize("seed", R.DENSE_SEEDS)
def test_decision_excuses_stay_under_the_cap(seed):
    """The decision test excuses a row whose reference top-2 gap is below 2 * MARGIN * d_probs; with A = 6 that is at most 10 % of the
    rows, so the test keeps its power."""
    d_logits, d_probs, _, p64 = R.spreads(seed, 6)
    excused = float((R.top2_gap(p64) < 2 * R.MARGIN * d_probs).double().mean())
    print(f"seed {seed}: d_logits {d_logits:.3e} d_probs {d_probs:.3e} excused {excused:.3%}")
    assert 0 < d_probs < 0.05 and 0 < d_logits
    assert excused <= R.EXCUSED_CAP, excused


def test_inference_switch_parsing(monkeypatch):
    from ippmarl.actor_native import ENV_VAR, resolve_mode
    monkeypatch.delenv(ENV_VAR, raising=False)
    assert resolve_mode() == "torch" and resolve_mode(None) == "torch"
    assert resolve_mode("native") == "native" and resolve_mode("torch") == "torch"
    monkeypatch.setenv(ENV_VAR, "native")
    assert resolve_mode() == "native"
    assert resolve_mode("torch") == "torch"          # the argument wins over the environment
    monkeypatch.setenv(ENV_VAR, "")
    assert resolve_mode() == "torch"
    monkeypatch.setenv(ENV_VAR, "triton")
    with pytest.raises(ValueError, match="actor inference"):
        resolve_mode()
    with pytest.raises(ValueError, match="actor inference"):
        resolve_mode("fast")
    import inspect

    from ippmarl.actor_native import deployment
    from ippmarl.trainer import COMATrainer
    for fn in (COMATrainer.__init__, deployment):
        assert inspect.signature(fn).parameters["actor_inference"].default is None
