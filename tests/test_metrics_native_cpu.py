"""CPU checks of the native metrics' float64 restatement (tests/metrics_native_ref.py) -- the reference the GPU tests hold csrc/metrics.hip to
-- against ``ippmarl.metrics`` and the golden coma_step fixture, its zero and NaN rules, and the switch's resolver."""
import numpy as np
import pytest
import torch

import metrics_native_ref as R
from configs import make_params, synthetic_minibatch


def _critic_records(golden):
    """The critic's step on the golden coma_step minibatch (tests/test_learning_cpu.py's) -> (record, critic, actions, fixture)."""
    from ippmarl.learners import CriticLearner
    from ippmarl.networks import ActorNetwork, CriticNetwork
    fx = golden("coma_step")
    params = make_params("c2")
    torch.manual_seed(int(fx["net_seed"]))
    ActorNetwork(params)
    critic = CriticNetwork(params)
    _, state, actions, _, td = synthetic_minibatch(60, 6, int(fx["mb_seed"]))
    learner = CriticLearner(params, critic, torch.device("cpu"))
    learner.collect = True
    learner.step(torch.tensor(state), torch.tensor(actions), torch.tensor(td))
    return dict(learner.last, discounted=torch.zeros(60)), critic, actions, fx


def _used_grads(net):
    return [getattr(getattr(net, layer), kind).grad.numpy() for layer in ("conv1", "conv2", "conv3", "fc1", "fc3") for kind in ("weight", "bias")]


def test_restatement_on_the_golden_critic_step(golden):
    """rtol=2e-4, atol=1e-7: what tests/test_learning_cpu.py holds ippmarl.metrics to on this fixture."""
    from ippmarl import metrics, metrics_native
    rec, critic, actions, fx = _critic_records(golden)
    mine = R.critic_scalars([rec["loss"].numpy()], [rec["q_chosen"].numpy()], [rec["td"].numpy()], [rec["discounted"].numpy()],
                            [rec["q_new"].numpy()], [actions]) + R.grad_figures(_used_grads(critic))
    theirs = metrics.critic_metrics([rec], critic)
    assert list(theirs) == list(metrics_native.KEYS[:19])
    np.testing.assert_allclose(mine, [theirs[k] for k in metrics_native.KEYS[:19]], rtol=2e-4, atol=1e-7)
    np.testing.assert_allclose(mine, fx["critic_metrics"], rtol=2e-4, atol=1e-7)


def test_restatement_of_the_actor_scalars_against_the_module():
    from ippmarl import metrics, metrics_native
    rng = np.random.RandomState(3)
    nb, B, A = 3, 17, 6
    probs = [torch.softmax(torch.tensor(rng.standard_normal((B, A)), dtype=torch.float32), 1) for _ in range(nb)]
    after = [torch.softmax(torch.tensor(rng.standard_normal((B, A)), dtype=torch.float32), 1) for _ in range(nb)]
    action = [rng.randint(0, A, size=B) for _ in range(nb)]
    adv = [torch.tensor(rng.standard_normal(B), dtype=torch.float32) for _ in range(nb)]
    loss = [torch.tensor(rng.standard_normal(), dtype=torch.float32) for _ in range(nb)]
    hidden = [torch.tensor(rng.random_sample(256), dtype=torch.float32) for _ in range(nb)]
    actor = torch.nn.Module()
    for name in metrics.LAYERS:
        layer = torch.nn.Linear(3, 2)
        for p in layer.parameters():
            p.grad = torch.tensor(rng.standard_normal(tuple(p.shape)), dtype=torch.float32)
        setattr(actor, name, layer)
    steps = [dict(loss=loss[s], adv=adv[s], log_probs=torch.log(probs[s]), hidden0=hidden[s],
                  log_chosen=torch.log(probs[s]).gather(1, torch.tensor(action[s]).view(-1, 1)).squeeze(1)) for s in range(nb)]
    theirs = metrics.actor_metrics(steps, actor, after)
    assert list(theirs) == list(metrics_native.KEYS[19:])
    grads = [getattr(getattr(actor, layer), kind).grad.numpy() for layer in ("conv1", "conv2", "conv3", "fc1", "fc3") for kind in ("weight", "bias")]
    mine = R.actor_scalars([x.numpy() for x in loss], [x.numpy() for x in adv], [x.numpy() for x in probs], action,
                           [x.numpy() for x in hidden], [x.numpy() for x in after]) + R.grad_figures(grads)
    np.testing.assert_allclose(mine, [theirs[k] for k in metrics_native.KEYS[19:]], rtol=2e-4, atol=1e-7)
    assert mine[-2] == 0.0 and theirs["Parameters/Actor/FC2 gradients"] == 0.0


def test_explained_variance_zero_rules():
    from ippmarl import metrics
    const = np.full(8, 3.0)
    for y_true, y_pred, want in ((const, const, 1.0), (const, const - 2.0, 1.0), (const, np.arange(8.0), 0.0)):
        assert R.explained_variance(y_true, y_pred) == want == metrics.explained_variance(torch.tensor(y_true), torch.tensor(y_pred))
    got = R.explained_variance([1.0, 2.0, 4.0], [1.0, 2.5, 3.5])
    assert got == pytest.approx(1 - np.var([0, -0.5, 0.5]) / np.var([1, 2, 4]))


def test_nan_cases():
    """A std over one element is NaN, 0 log 0 is NaN, a NaN input reaches the scalars it enters and no other."""
    one = R.critic_scalars([1.0], [np.array([0.5])], [np.array([2.0])], [np.array([1.0])], [np.array([[1.0, 2.0]])], [np.array([1])])
    assert np.isnan(one[2]) and np.isnan(one[9]) and np.isnan(one[11]) and one[1] == 2.0 and not np.isnan(one[6])
    assert float(torch.tensor([2.0]).std()) != float(torch.tensor([2.0]).std())          # torch's rule, which the definition follows
    probs = np.array([[0.0, 1.0], [0.5, 0.5]])
    a = R.actor_scalars([0.0], [np.array([1.0, 2.0])], [probs], [np.array([1, 0])], [np.ones(256)], [probs])
    assert np.isnan(a[4]) and np.isnan(a[5]) and not np.isnan(a[3]) and a[6] == 1.0
    rng = np.random.RandomState(1)
    td = rng.standard_normal(9)
    args = dict(loss=[0.25], q_chosen=[rng.standard_normal(9)], disc=[rng.standard_normal(9)], q_new=[rng.standard_normal((9, 4))],
                action=[rng.randint(0, 4, 9)])
    clean = np.array(R.critic_scalars(td=[td], **args))
    td[4] = np.nan
    dirty = np.array(R.critic_scalars(td=[td], **args))
    hit = np.isnan(dirty)
    assert list(np.nonzero(hit)[0]) == [1, 2, 7] and np.array_equal(clean[~hit], dirty[~hit])


def test_resolve_mode(monkeypatch):
    from ippmarl import metrics_native
    monkeypatch.delenv(metrics_native.ENV_VAR, raising=False)
    assert metrics_native.resolve_mode() == "torch" and metrics_native.resolve_mode("native") == "native"
    monkeypatch.setenv(metrics_native.ENV_VAR, "native")
    assert metrics_native.resolve_mode() == "native" and metrics_native.resolve_mode("torch") == "torch"
    for bad in ("", "hip", "Native"):
        with pytest.raises(ValueError):
            metrics_native.resolve_mode(bad)
    monkeypatch.setenv(metrics_native.ENV_VAR, "gpu")
    with pytest.raises(ValueError):
        metrics_native.resolve_mode()
    assert len(metrics_native.KEYS) == R.N_SCALARS == metrics_native.SCALARS
