"""One policy network per UE (D3-CoMP, the reference's ``--separate-agent-nns``: env_setup.py:295 keys the policy map by UE) on the
device (include/dcomp_policy_set.h): a set over FcnetActors run in ONE launch, and one PPO learner per policy.

    members = [FcnetActor('multi', U, B, weights[p], value_weights=value_weights[p]) for p in range(U)]
    actor = PerUEActor(members)                                  # UE slot u -> members[u]; slot_policy=[...] maps otherwise
    learner = PerUELearner(actor, lr=5e-5, max_rows=rows_per_policy_minibatch)
    for _ in range(iters):
        batch = collect(env, actor, num_steps=50, gamma=0.99, lam=0.95, dist_inputs=True)
        stats = learner.update(batch, num_sgd_iter=30, minibatch_rows=rows_per_policy_minibatch)      # one dict per policy

D3-CoMP differs from DD-CoMP (one shared network, FcnetActor alone) only in which weights a decision row goes through.  The set's
launch gives each wavefront 32 envs of ONE UE slot with that slot's weights and writes every output where the shared launch has it,
so ``sampler.collect``, the advantages and the env step are the shared policy's.  The set copies no weights: it holds pointers into
its members' device images, and a member's learner rewrites those in place -- the set's next launch runs the trained weights.

Members are ``multi`` actors of one shape (UE slots, stations, hidden width, activation, device), all without a value function or
all with a value trunk of their own; attach value functions BEFORE building the set -- its table holds the trunks the members have then,
and once a member gets one afterwards every call on the set raises ValueError (build a new set).  Central members (one network by construction) and a shared value function are refused
(NotImplementedError), and so is ``act`` on an env with UE arrival / departure: slots shift on departure, a slot is not one UE there.
"""
import ctypes

import torch

from . import _lib
from .actor import FcnetActor, _ActorLaunch
from .learner import INPUT, INPUTS, PPOLearner, close_out, field_pointers, fill, flatten_batch, minibatch_plan, sgd_epochs, standardize


def default_slot_policy(num_ue, num_policies):
    """include/dcomp_policy_set.h's default: slot u -> u % P."""
    return [u % int(num_policies) for u in range(int(num_ue))]


def policy_rows(num_rows, num_ue, slot_policy, num_policies, device=None):
    """The row split of a flattened multi-agent sample batch ([T][E][U]: source row s is UE slot s % num_ue): per policy p the
    ascending int64 tensor of the source rows whose slot maps to p.  The tensors are disjoint and together cover the batch."""
    sp = torch.as_tensor(list(slot_policy), dtype=torch.int64, device=device)
    if sp.numel() != int(num_ue):
        raise ValueError(f"slot_policy has {sp.numel()} entries, the env {num_ue} UE slots")
    of_row = sp[torch.arange(int(num_rows), device=device) % int(num_ue)]
    return [torch.nonzero(of_row == p).reshape(-1) for p in range(int(num_policies))]


class PerUEActor(_ActorLaunch):
    """A set of FcnetActors, one per UE slot (or per group of slots), running as one HIP kernel launch.  ``actions``, ``value`` and
    ``act`` are FcnetActor's: same arguments, same checks, same [E, U] outputs."""
    _ACTIONS, _ACTIONS_V = 'dcomp_policy_set_actions', 'dcomp_policy_set_actions_v'

    def __init__(self, actors, slot_policy=None):
        self._h = None
        actors = list(actors)
        if not actors or not all(isinstance(a, FcnetActor) for a in actors):
            raise ValueError("actors must be a non-empty list of FcnetActors")
        first = actors[0]
        self.members = actors                                    # (the set holds pointers into their device images: they stay alive with it)
        self.kind, self.U, self.B = first.kind, first.U, first.B
        self.heads, self.num_logits, self.num_in = first.heads, first.num_logits, first.num_in
        self.hidden, self.activation, self.device = first.hidden, first.activation, first.device
        self._L = first._L
        self._has_value = first.value_weights is not None        # the value form the set's table is written for, fixed here
        P = len(actors)
        if slot_policy is None:
            self.slot_policy = default_slot_policy(self.U, P)
        else:
            self.slot_policy = [int(x) for x in slot_policy]
            if len(self.slot_policy) != self.U:
                raise ValueError(f"slot_policy has {len(self.slot_policy)} entries, the members {self.U} UE slots")
        handles = (ctypes.c_void_p * P)(*[a._h.value for a in actors])
        slots = (ctypes.c_int32 * self.U)(*self.slot_policy)
        cfg = _lib.DcompPolicySetCfg(ctypes.sizeof(_lib.DcompPolicySetCfg), P, handles, slots)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._L.dcomp_policy_set_create(ctypes.byref(cfg), ctypes.byref(h)))      # agreement, refusals, slot range: checked there
        self._h = h

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self._L.dcomp_policy_set_destroy(h)
            self._h = None

    @property
    def num_policies(self):
        return len(self.members)

    @property
    def weights(self):
        return [m.weights for m in self.members]

    @property
    def value_weights(self):
        """The members' value weights, one entry per policy; None iff the members had no value function when the set was built (a
        set_value on a member since does not reach the set's table: every launch is then refused)."""
        return [m.value_weights for m in self.members] if self._has_value else None

    @classmethod
    def random(cls, num_ue, num_bs, hidden=256, activation='tanh', seed=0, bias_std=0.0, device='cuda', num_policies=None, slot_policy=None,
               value=True):
        """Random-init members (policy p from seed + p, as FcnetActor.random_weights / random_value_weights) for tools and tests."""
        P = int(num_ue) if num_policies is None else int(num_policies)
        members = [FcnetActor('multi', num_ue, num_bs, FcnetActor.random_weights('multi', num_ue, num_bs, hidden, seed + p, bias_std), activation, device,
                              value_weights=FcnetActor.random_value_weights('multi', num_ue, num_bs, hidden, seed + p, bias_std) if value else None)
                   for p in range(P)]
        return cls(members, slot_policy)

    def member_of(self, slot):
        return self.members[self.slot_policy[int(slot)]]

    def reference_logits(self, obs_rows_of_slot, slot, form='bf16'):
        """FcnetActor.reference_logits of the slot's member, on observation rows of that slot."""
        return self.member_of(slot).reference_logits(obs_rows_of_slot, form)

    def reference_value(self, obs_rows_of_slot, slot, form='bf16'):
        return self.member_of(slot).reference_value(obs_rows_of_slot, form)

    def act(self, env, sample=True, obs=None, compact=False, out=None, logp=None, vf=None, logits=None):
        """FcnetActor.act with every UE slot's own policy."""
        if env.dynamic:
            raise NotImplementedError("envs with UE arrival / departure: slots shift on departure, a slot is not one UE and has no policy of its own")
        return super().act(env, sample=sample, obs=obs, compact=compact, out=out, logp=logp, vf=vf, logits=logits)


class PerUELearner:
    """PPO for a PerUEActor: one PPOLearner per member, each with its own Adam state and its own kl_coeff -- RLlib likewise gives each
    policy its own batch, its own advantage standardisation and its own KL coefficient.  Every update lands in the member's handle,
    which the set's next launch reads.

    ppo_kwargs are PPOLearner's.  minibatch_rows and max_rows are PER POLICY, and the workspaces are P times one learner's: max_rows
    should be a policy's minibatch, not the batch.  ``update`` runs the P updates one after the other, P x minibatches x (gathers +
    four launches), so small per-policy batches are bound by launches; ``update(grouped=True)`` trains all policies in one launch
    round per minibatch round (include/dcomp_learner_group.h) and leaves every learner in the same state, bit for bit.  The two can
    be mixed with each other and with calls on a member learner."""

    def __init__(self, actor, **ppo_kwargs):
        if not isinstance(actor, PerUEActor):
            raise ValueError("actor must be a PerUEActor")
        self.actor, self.device = actor, actor.device
        if len({id(m) for m in actor.members}) != len(actor.members):
            raise ValueError("the same FcnetActor is a member twice: two learners would train one handle with two Adam states -- list it once and "
                             "map its slots to it with slot_policy")
        self.learners = [PPOLearner(m, **ppo_kwargs) for m in actor.members]
        self._split = {}
        self._group = None                                       # dcomp_learner_group over the learners: built by the first grouped update

    def __del__(self):
        g = getattr(self, '_group', None)
        if g is not None and g.value:                            # (before the learners its table points into)
            self._group = None
            try:
                self.actor._L.dcomp_learner_group_destroy(g)
            except Exception:                                    # interpreter shutdown: the actor or the library is gone already
                pass

    def rows_of(self, num_rows):
        """policy_rows() for this set on the device, kept per batch size."""
        if num_rows not in self._split:
            a = self.actor
            self._split = {num_rows: policy_rows(num_rows, a.U, a.slot_policy, a.num_policies, self.device)}
        return self._split[num_rows]

    def update(self, batch, num_sgd_iter=30, minibatch_rows=None, seed=0, grouped=False):
        """PPO's SGD phase on one collect(env, per_ue_actor, ..., dist_inputs=True) batch, rows or compact record: policy p's
        PPOLearner.update on the source rows whose UE slot maps to p (rows=), with seed + p.  Returns one statistics dict per policy
        (None for a policy no slot maps to, whose state stays untouched).

        grouped=True: the same update with all policies in one launch round per minibatch round.  Every policy keeps its own
        advantage standardisation, its own permutations (a generator seeded seed + p), its own minibatch boundaries, Adam state and
        kl_coeff; round k hands every policy its k-th minibatch through one [P, rows] index into the batch where it lies (both batch
        formats), and a policy with fewer minibatches sits the later rounds out.  One synchronisation at the end.  The learners'
        states and the returned statistics are those of grouped=False, bit for bit."""
        rows = self.rows_of(int(batch['actions'].numel()))
        if grouped:
            return self._update_grouped(batch, rows, int(num_sgd_iter), minibatch_rows, int(seed))
        return [ln.update(batch, num_sgd_iter=num_sgd_iter, minibatch_rows=minibatch_rows, seed=int(seed) + p, rows=rows[p], check_rows=False)
                if rows[p].numel() else None                     # (check_rows: policy_rows() built them, distinct and in range)
                for p, ln in enumerate(self.learners)]

    def _group_handle(self):
        if self._group is None:
            P = len(self.learners)
            handles = (ctypes.c_void_p * P)(*[ln._h.value for ln in self.learners])
            cfg = _lib.DcompLearnerGroupCfg(ctypes.sizeof(_lib.DcompLearnerGroupCfg), P, handles)
            h = ctypes.c_void_p()
            with torch.cuda.device(self.device):
                _lib.check(self.actor._L.dcomp_learner_group_create(ctypes.byref(cfg), ctypes.byref(h)))
            self._group = h
        return self._group

    def _update_grouped(self, batch, rows, num_sgd_iter, minibatch_rows, seed):
        L, dev = self.actor._L, self.device
        first, P = self.learners[0], len(self.learners)
        src, N, compact = flatten_batch(first.actor, batch)
        obs, fmt, _ = first._source_obs(src)
        live = [p for p in range(P) if rows[p].numel()]
        # every policy's advantages standardised over its own rows (PPOLearner.update's rule), back in source order in ONE tensor: the
        # row sets are disjoint
        adv = torch.zeros_like(src['advantages'])
        n_of, mb_of = [int(rows[p].numel()) for p in range(P)], [0] * P
        for p in live:
            mb_of[p] = minibatch_plan(n_of[p], minibatch_rows, self.learners[p].max_rows)[0]
            adv.index_copy_(0, rows[p], standardize(src['advantages'].index_select(0, rows[p])))
        ptr = field_pointers(first.actor, dict({n: src[n] for n in INPUTS}, advantages=adv), {INPUT: N})
        # round k: positions [k step, k step + mb_p) of every policy that has that many.  A policy's minibatch is `step` rows unless
        # it has fewer rows than that -- then it is its one minibatch, in round 0
        step = max(mb_of)
        taken = {p: (n_of[p] + mb_of[p] - 1) // mb_of[p] for p in live}
        rounds = max(taken.values())
        stride = max(n_of)
        index = torch.zeros((P, stride), dtype=torch.int32, device=dev)
        stats = torch.zeros((rounds, P, _lib.PPO_NUM_STATS), dtype=torch.float32, device=dev)
        epochs = {p: sgd_epochs(n_of[p], num_sgd_iter, seed + p, dev) for p in live}
        hyper = (_lib.DcompPpoHyper * P)(*[ln._hyper_struct() for ln in self.learners])
        lr = (ctypes.c_float * P)(*[ln.lr for ln in self.learners])
        round_rows = [(ctypes.c_int64 * P)(*[max(0, min(mb_of[p], n_of[p] - k * step)) if mb_of[p] else 0 for p in range(P)]) for k in range(rounds)]
        round_active = [(ctypes.c_int32 * P)(*[1 if r else 0 for r in rr]) for rr in round_rows]
        g = self._group_handle()
        b = fill(_lib.DcompGroupBatch, obs_format=fmt, source_rows=N, obs=obs.data_ptr(), index_stride=stride, **ptr)
        with torch.cuda.device(dev):
            stream = first.actor._stream()
            for _ in range(num_sgd_iter):
                for p in live:
                    index[p, :n_of[p]] = rows[p].index_select(0, next(epochs[p]))
                for k in range(rounds):
                    b.index, b.rows = index.data_ptr() + 4 * k * step, round_rows[k]
                    _lib.check(L.dcomp_learner_group_grads(g, ctypes.byref(b), hyper, ctypes.c_void_p(stats[k].data_ptr()), stream))
                    _lib.check(L.dcomp_learner_group_apply(g, lr, round_active[k], stream))
        # a policy's mean over the rounds it took part in: PPOLearner.update's own reduction of its own [minibatches, 5] tensor
        out = [None] * P
        for p, st in zip(live, close_out([self.learners[p] for p in live], torch.stack([stats[:taken[p], p].contiguous().mean(0) for p in live]))):
            out[p] = st
        return out

    def get_weights(self):
        """[(weights, value_weights)] per policy; refreshes the members' host copies (PPOLearner.get_weights)."""
        return [ln.get_weights() for ln in self.learners]

    def to_rllib_weights(self, prefix='policy_{}/'):
        """One RLlib weight dict per policy; prefix is formatted with the policy's number."""
        return [ln.to_rllib_weights(prefix.format(p)) for p, ln in enumerate(self.learners)]

    def state_dict(self):
        return [ln.state_dict() for ln in self.learners]

    def load_state_dict(self, states):
        states = list(states)
        if len(states) != len(self.learners):
            raise ValueError(f"{len(states)} states for {len(self.learners)} policies")
        for ln, st in zip(self.learners, states):
            ln.load_state_dict(st)


__all__ = ['PerUEActor', 'PerUELearner', 'policy_rows', 'default_slot_policy']
