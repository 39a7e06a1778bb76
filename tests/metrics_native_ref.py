"""The 32 per-training-step scalars of ``ippmarl.metrics`` restated in float64 NumPy over lists of per-minibatch ("slot") arrays: the
reference the native metrics (csrc/metrics.hip) are judged against.  Straight definitions, no streaming: stack the slots, convert to
float64, reduce with NumPy (two-pass std).  Order and names: ``ippmarl.metrics_native.KEYS``.

``bound(ref, scale)`` is the derived error bound of the GPU tests: the inputs are exact in double, reordering a sum of n <= 7e4 terms
moves it by at most n 2^-53 ~ 8e-12 of sum |x|, Chan merges and a 1-2 ulp log / exp stay inside two orders of margin -> 1e-9 (|ref| +
mean |input|), with ``scales`` naming, per scalar, the mean magnitude of the inputs that enter it."""
import numpy as np

N_SCALARS = 32


def _f64(xs):
    return np.stack([np.asarray(x, dtype=np.float64) for x in xs])


def explained_variance(y_true, y_pred):
    """sklearn's explained_variance_score for one output: population variances; a zero variance of y_true gives 1 if the residual's
    variance is zero too, else 0."""
    y_true, y_pred = np.asarray(y_true, np.float64).ravel(), np.asarray(y_pred, np.float64).ravel()
    diff = y_true - y_pred
    num = np.mean((diff - diff.mean()) ** 2)
    den = np.mean((y_true - y_true.mean()) ** 2)
    if den == 0.0:
        return 1.0 if num == 0.0 else 0.0
    return float(1.0 - num / den)


def _std(x):
    with np.errstate(all="ignore"):
        return float(np.std(x, ddof=1)) if x.size > 1 else float("nan")      # one element: NaN, as torch


def critic_scalars(loss, q_chosen, td, disc, q_new, action):
    """Lists over slots: loss (scalar), q_chosen / td / disc [B], q_new [B,A] (post-step), action [B] -> the 13 critic scalars."""
    with np.errstate(all="ignore"):
        loss, qc, td, disc, q = _f64(loss), _f64(q_chosen), _f64(td), _f64(disc), _f64(q_new)
        nb, B, A = q.shape
        qc, td, disc = qc.reshape(nb, B), td.reshape(nb, B), disc.reshape(nb, B)
        act = np.stack([np.asarray(a).reshape(B).astype(np.int64) for a in action])
        dev = np.abs(disc - qc)
        mx = q.max(axis=1, keepdims=True)
        logp = q - (mx + np.log(np.exp(q - mx).sum(axis=1, keepdims=True)))         # log-softmax over the BATCH axis of each slot
        ok = (act >= 0) & (act < A)
        chosen = np.where(ok, np.take_along_axis(logp, np.clip(act, 0, A - 1)[..., None], axis=2)[..., 0], np.nan)
        return [float(loss.mean()), float(td.mean()), _std(td), float(qc.mean()), float(q.mean()), float(q.min()), _std(q),
                explained_variance(disc, td), float(disc.mean()), _std(disc), float(dev.mean()), _std(dev), float(chosen.mean())]


def actor_scalars(loss, adv, probs, action, hidden0, probs_after):
    """Lists over slots: loss, adv [B], probs [B,A] (pre-step), action [B], hidden0 [256], probs_after [B,A] -> the 7 actor scalars."""
    with np.errstate(all="ignore"):
        loss, adv, p, h, after = _f64(loss), _f64(adv), _f64(probs), _f64(hidden0), _f64(probs_after)
        nb, B, A = p.shape
        act = np.stack([np.asarray(a).reshape(B).astype(np.int64) for a in action])
        logp = np.log(p)
        ok = (act >= 0) & (act < A)
        chosen = np.where(ok, np.take_along_axis(logp, np.clip(act, 0, A - 1)[..., None], axis=2)[..., 0], np.nan)
        entropy = -(p * logp).sum(-1)
        kl = (p * (logp - after)).sum(0)                 # log(p_old / exp(p_after)), summed over the minibatch axis
        return [float(loss.mean()), float(adv.mean()), _std(adv.reshape(nb, B)), float(chosen.mean()), float(entropy.mean()),
                float(kl.mean()), float(np.mean([np.mean(x.ravel() ** 2) for x in h]))]


def grad_figures(grads):
    """The ten gradients of a net (conv1.w, conv1.b, ..., fc1.w, fc1.b, fc3.w, fc3.b) -> the six figures (fc2: 0)."""
    l1 = [float(np.abs(np.asarray(g, np.float64)).sum()) for g in grads]
    layer = [(l1[2 * i] + l1[2 * i + 1]) / 2.0 for i in range(5)]
    return layer[:4] + [0.0, layer[4]]


def all_scalars(c, a, critic_grads, actor_grads):
    """``c``: dict of critic_scalars' lists, ``a``: of actor_scalars' -> the 32 values in KEYS order."""
    return np.array(critic_scalars(**c) + grad_figures(critic_grads) + actor_scalars(**a) + grad_figures(actor_grads), dtype=np.float64)


def _mag(*lists):
    with np.errstate(all="ignore"):
        vals = np.concatenate([np.abs(np.asarray(x, np.float64)).ravel() for xs in lists for x in xs])
        return float(np.nanmean(vals[np.isfinite(vals)])) if np.isfinite(vals).any() else 0.0


def scales(c, a, critic_grads, actor_grads):
    """Per scalar, the mean magnitude of the (finite) inputs that enter it."""
    td, disc, qc, q = _mag(c["td"]), _mag(c["disc"]), _mag(c["q_chosen"]), _mag(c["q_new"])
    p = _mag(a["probs"], a["probs_after"])
    crit = [_mag(c["loss"]), td, td, qc, q, q, q, _mag(c["td"], c["disc"]), disc, disc, _mag(c["disc"], c["q_chosen"]),
            _mag(c["disc"], c["q_chosen"]), q]

    def g(grads):
        m = [_mag([x]) for x in grads]
        layer = [max(m[2 * i], m[2 * i + 1]) for i in range(5)]
        return layer[:4] + [0.0, layer[4]]

    act = [_mag(a["loss"]), _mag(a["adv"]), _mag(a["adv"]), p, p, p, _mag(a["hidden0"])]
    return np.array(crit + g(critic_grads) + act + g(actor_grads), dtype=np.float64)


def bound(ref, scale):
    return 1e-9 * (np.abs(ref) + scale)
