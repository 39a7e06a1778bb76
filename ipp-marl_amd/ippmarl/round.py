"""The three seams of ``COMATrainer._update_compute``: where a minibatch's rows come from (``buffer``), where a data pass's order comes
from (``shuffle``) and who watches the round (``metrics``, under ``update(diagnostics=True)``).  Each has a torch form and a native form
with the same methods, chosen once per round, so the round loop itself is the reference's cadence and nothing else."""
from __future__ import annotations

import torch

from . import metrics, optim_native


# ---- minibatch source ------------------------------------------------------------------------------------------------------------------
class TorchBatches:
    """buffer="torch": the flat views of the buffer indexed lazily, three index kernels per side."""

    def __init__(self, trainer, W: int, td: torch.Tensor):
        n = W * trainer.T * trainer.E * trainer.N
        self.obs = trainer.buf_obs[:W].reshape(n, 11, 11, 7)
        self.states = trainer.buf_state[:W].reshape(n, 11, 11, 12)
        self.actions = trainer.buf_action[:W].reshape(n)
        self.masks = trainer.buf_mask[:W].reshape(n, trainer.A)
        self.td = td
        self.rows = []

    def begin_pass(self, perm: torch.Tensor, bs: int, batch_number: int):
        """Cuts the pass's order into the rows of its minibatches (views of ``perm``)."""
        self.rows = [perm[b * bs:(b + 1) * bs] for b in range(batch_number)]

    def critic(self, b: int):
        """(states, actions, td) of minibatch ``b``."""
        i = self.rows[b]
        return self.states[i], self.actions[i], self.td[i]

    def actor(self, b: int):
        """(obs, actions, masks) of minibatch ``b``."""
        i = self.rows[b]
        return self.obs[i], self.actions[i], self.masks[i]

    def values(self, src: torch.Tensor, b: int, out: torch.Tensor) -> torch.Tensor:
        """The float32 ``src`` at minibatch ``b``'s rows into ``out``."""
        return out.copy_(src[self.rows[b]])


class NativeBatches(TorchBatches):
    """buffer="native": ONE gather per minibatch b fills output set b % 2 of the replay (states, obs, actions, masks, td), issued by
    ``critic(b)`` right before critic_learner.backward(b); the critic side and the actor side of minibatch b are views of that set.
    Why two alternating sets are enough: set b % 2 is next written by the gather of minibatch b + 2 (or of a later data pass).  The
    readers of minibatch b are critic.backward(b) (its saved tensors are released inside the call), critic.apply() of b (the post-step Q
    of the same states; the learner drops its reference there) and actor.backward(b).  In the round loop all three are issued -- on the
    one stream everything there runs on -- before the gather of b + 1, hence before that of b + 2: actor.backward(b) comes first in
    iteration b, then gather(b + 1), critic.backward(b + 1) and the two apply() calls, none of which reads minibatch b.  The second set
    is what keeps minibatch b intact while b + 1 is being gathered and used beside it.
    A diagnostics round of metrics="torch" takes TorchBatches for the whole round: its records hold minibatch tensors across minibatches.
    metrics="native" keeps nothing (the learners hand each minibatch's arrays to the accumulator when they have them)."""

    def __init__(self, trainer, W: int, td: torch.Tensor):
        super().__init__(trainer, W, td)
        self.replay = trainer._replay
        self.cur = [None, None]

    def critic(self, b: int):
        s = self.cur[b % 2] = self.replay.minibatch(self.rows[b], b % 2)
        return s[0], s[2], s[4]

    def actor(self, b: int):
        s = self.cur[b % 2]
        return s[1], s[2], s[3]

    def values(self, src: torch.Tensor, b: int, out: torch.Tensor) -> torch.Tensor:
        return self.replay.gather_values(src, self.rows[b], out)     # (one more gather launch)


# ---- permutation source ----------------------------------------------------------------------------------------------------------------
class TorchOrder:
    """shuffle="torch": ``torch.randperm`` from the device generator; a recorded round reads rows of ``perms``, which ``before_replay``
    refills from the host.  Mixed team sizes: the order is drawn over the flying transitions and mapped through
    ``valid_transitions``."""

    def __init__(self, trainer):
        self.trainer, self.perms, self.flying = trainer, None, None

    def begin_round(self, W: int) -> int:
        """-> the number of rows a data pass of this round orders (mixed team sizes: those of agents that fly)."""
        tr = self.trainer
        self.flying = tr.valid_transitions(W)
        return W * tr.T * tr.E * tr.N if self.flying is None else int(self.flying.numel())

    def order(self, data_pass: int, nv: int, recorded) -> torch.Tensor:
        """The order of ``data_pass`` over ``nv`` rows, as buffer rows; ``recorded``: None (eager) or what ``capture`` returned."""
        perm = torch.randperm(nv, device=self.trainer.device) if recorded is None else recorded[data_pass]
        return perm if self.flying is None else self.flying[perm]

    def capture(self, n: int) -> torch.Tensor:
        """Before the round is recorded: the fixed buffer its data passes read."""
        tr = self.trainer
        self.perms = torch.stack([torch.randperm(n, device=tr.device) for _ in range(tr.data_passes)])
        return self.perms

    def end_capture(self):
        """The last thing recorded into the round."""

    def before_replay(self, n: int):
        for row in self.perms:
            row.copy_(torch.randperm(n, device=self.trainer.device))

    def after_replay(self):
        pass

    def load(self, counters, rng):
        if rng is not None:      # (the process-wide generator: only for who draws from it)
            torch.cuda.set_rng_state(rng.to("cpu", torch.uint8), self.trainer.device)


class NativeOrder:
    """shuffle="native": one ``NativeShuffle.permutation`` launch per data pass, keyed by the round by value (eager: train_step on
    entry) or by the device counter (recorded: the launches are nodes of the graph, whose last node advances the counter).  Under
    mixed team sizes the same launch maps ranks to buffer rows, so ``valid_transitions`` is never computed."""

    def __init__(self, trainer, shuffle):
        self.trainer, self.shuffle, self.round0 = trainer, shuffle, 0

    def begin_round(self, W: int) -> int:
        tr = self.trainer
        self.round0 = tr.train_step          # (the eager round counts train_step up as it goes)
        return W * tr.T * (tr.E * tr.N if tr.env.n_active is None else self.shuffle.flying)

    def order(self, data_pass: int, nv: int, recorded) -> torch.Tensor:
        return self.shuffle.permutation(data_pass, nv, self.round0 if recorded is None else None)

    def capture(self, n: int) -> torch.Tensor:
        self.shuffle.set_round(self.trainer.train_step)
        return self.shuffle.idx

    def end_capture(self):
        self.shuffle.advance()

    def before_replay(self, n: int):
        if self.shuffle.host_round != self.trainer.train_step:
            self.shuffle.set_round(self.trainer.train_step)      # (eager rounds since the last replay: they take the round by value)

    def after_replay(self):
        self.shuffle.host_round = self.trainer.train_step + 1

    def load(self, counters, rng):
        self.shuffle.set_round(int(counters["shuffle_round"]))


# ---- round observer --------------------------------------------------------------------------------------------------------------------
class Unobserved:
    """Nobody watches: every hook of the round loop is a no-op.  Also what the observing forms hand out for data passes > 0."""

    def __init__(self, trainer):
        self.trainer = trainer

    def begin_pass(self, data_pass: int):
        """-> the observer of this data pass."""
        self._collect(False)
        return self

    def _collect(self, on: bool):
        self.trainer.critic_learner.collect = self.trainer.actor_learner.collect = on

    def critic_reduced(self, b: int):
        """After the critic's backward and all-reduce of minibatch ``b``."""

    def critic_applied(self, b: int):
        """After the critic's step on minibatch ``b``."""

    def before_actor(self, b: int):
        pass

    def after_actor(self, b: int):
        """After the actor's backward on minibatch ``b``."""

    def actor_reduced(self, b: int):
        """After the all-reduce that carried the actor's gradients of minibatch ``b``, before its step."""

    def end_pass(self, eps):
        pass


class TorchObserver(Unobserved):
    """metrics="torch": the learners keep per-minibatch records of data pass 0 (``collect``), ippmarl.metrics reduces them at its end,
    launch by launch, with one extra float32 actor forward per minibatch for the KL figure."""

    def __init__(self, trainer, batches, dr: torch.Tensor):
        super().__init__(trainer)
        self.batches, self.dr, self.idle = batches, dr, Unobserved(trainer)
        self.crit_rec, self.act_rec = [], []

    def begin_pass(self, data_pass: int):
        if data_pass:
            return self.idle.begin_pass(data_pass)
        self._collect(True)
        return self

    def critic_applied(self, b: int):
        self.crit_rec.append(dict(self.trainer.critic_learner.last, discounted=self.dr[self.batches.rows[b]]))

    def after_actor(self, b: int):
        self.act_rec.append(self.trainer.actor_learner.last)

    def end_pass(self, eps):
        tr, bt = self.trainer, self.batches
        with torch.no_grad():
            after = [tr.actor(bt.obs[rows], eps)[0] for rows in bt.rows]
        tr.last_diagnostics = dict(metrics.critic_metrics(self.crit_rec, tr.critic))
        tr.last_diagnostics.update(metrics.actor_metrics(self.act_rec, tr.actor, after))
        self._collect(False)


class NativeObserver(Unobserved):
    """metrics="native": the learners hand each minibatch's arrays of data pass 0 to ``sink`` (a NativeMetrics) through their
    ``observe``; the gradient figures are the last minibatch's, after the all-reduce, before the step clears them."""

    def __init__(self, trainer, batches, dr: torch.Tensor, sink):
        super().__init__(trainer)
        self.batches, self.dr, self.sink, self.idle = batches, dr, sink, Unobserved(trainer)
        self.last = trainer.batch_number - 1

    def begin_pass(self, data_pass: int):
        self._collect(False)
        return self.idle if data_pass else self

    def _grad_l1(self, which: int, net, b: int):
        if b == self.last:
            self.sink.grad_l1(which, [p.grad for p in optim_native.used_parameters(net)])

    def critic_reduced(self, b: int):
        # the discounted returns of minibatch b into the accumulator's own buffer
        disc = self.batches.values(self.dr, b, self.sink.disc[b])
        self.trainer.critic_learner.observe = (self.sink, b, disc)
        self._grad_l1(0, self.trainer.critic, b)

    def before_actor(self, b: int):
        self.trainer.actor_learner.observe = (self.sink, b)

    def actor_reduced(self, b: int):
        self._grad_l1(1, self.trainer.actor, b)

    def end_pass(self, eps):
        # the KL figure: the updated actor on the pass's minibatches, through the configured no-grad path, then the closing launch
        tr, bt = self.trainer, self.batches
        tr.critic_learner.observe = tr.actor_learner.observe = None
        for b, rows in enumerate(bt.rows):
            self.sink.actor_after(b, tr._act_rows(bt.obs[rows], eps))
        self.sink.finalize()
