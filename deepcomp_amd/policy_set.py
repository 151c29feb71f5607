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

``update(grouped=True)`` trains all policies in one launch round per minibatch round (include/dcomp_learner_group.h), and
``update(micro_rows=, grad_clip=)`` trains minibatches larger than the handles micro-batch by micro-batch and clips each policy's
gradient by its global norm, sequential or grouped (include/dcomp_learner_group_accum.h: the policies' accumulators are one [P, flat]
and one [P, 8] tensor, a micro-batch round and a finish are one launch round each).  ``group_plan`` lays the policies' minibatches and
micro-batches side by side; ``PerUELearner.grouped_phases`` is the one grouped SGD loop, which ``update`` drains and
deepcomp_amd.dp_learner.DataParallelPerUELearner drives across the ranks of a data-parallel set.

Members are ``multi`` actors of one shape (UE slots, stations, hidden width, activation, device), all without a value function or
all with a value trunk of their own; attach value functions BEFORE building the set -- its table holds the trunks the members have then,
and once a member gets one afterwards every call on the set raises ValueError (build a new set).  Central members (one network by construction) and a shared value function are refused
(NotImplementedError), and so is ``act`` on an env with UE arrival / departure: slots shift on departure, a slot is not one UE there.

Envs with UE arrival / departure take the second kind of set, keyed by UE ID (include/dcomp_policy_set_uid.h; the reference keys its
policy map by ue.id and builds a policy for every UE the episode will ever see, env.max_id here): ``PerIdActor(members)`` runs the
row at (env, slot) through member id - 1, the id read from the env's uid word of that slot, and ``PerIdLearner`` trains member p on the
counted rows of the UE with id p + 1 (``policy_rows_by_id``):

    actor = PerIdActor([FcnetActor('multi', env.U, B, weights[p], value_weights=value_weights[p]) for p in range(env.max_id)])
    learner = PerIdLearner(actor, lr=5e-5, max_rows=rows_per_policy_minibatch)
    batch = collect(env, actor, num_steps=50, gamma=0.99, lam=0.95, dist_inputs=True, by_ue=True)
    stats = learner.update(batch, num_sgd_iter=30, minibatch_rows=rows_per_policy_minibatch)
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .actor import FcnetActor, _ActorLaunch
from .tape import uid_fields
from .learner import INPUT, INPUTS, SUM, PPOLearner, close_out, field_pointers, fill, flatten_batch, minibatch_plan, sgd_epochs, standardize


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


def group_plan(n_of, minibatch_rows, max_rows_of, micro_rows=None, grad_clip=None, accumulate=False, **wording):
    """The launch rounds of a grouped SGD iteration over P policies with n_of[p] rows each: minibatch_plan() per policy (its checks,
    its refusals; wording: its noun / hint), then the policies' minibatches and micro-batches side by side.  Returns (accumulated,
    taken, rounds): whether the minibatches go through the accumulators (micro_rows, grad_clip or accumulate given); per policy the
    minibatch rounds it takes part in (0: a policy without rows); and per minibatch round k the pair (rows, micro) -- rows[p] the
    positions of policy p's k-th minibatch (0: it has none left and sits the round out), micro the round's launches, each (offset,
    rows): policy p trains positions [offset, offset + rows[p]) of its own permutation.  Policy p's positions are the ones its own
    PPOLearner.update(rows=..., micro_rows=...) takes: minibatch k at k mb_p, micro-batch j of it at j micro_p behind that.  One offset
    serves all policies because a policy's minibatch is the common `step` rows unless it has fewer rows than that (then it is its one
    minibatch, in round 0), and its micro-batch the common one unless its minibatch is smaller (then it is its one micro-batch)."""
    P = len(n_of)
    mb_of, micro_of, accumulated = [0] * P, [0] * P, bool(accumulate)
    for p in range(P):
        if n_of[p]:
            mb_of[p], micro_of[p], acc_p = minibatch_plan(n_of[p], minibatch_rows, max_rows_of[p], micro_rows, grad_clip, **wording)
            accumulated = accumulated or acc_p
    step, micro_step = max(mb_of), max(micro_of)
    taken = [(n_of[p] + mb_of[p] - 1) // mb_of[p] if mb_of[p] else 0 for p in range(P)]
    rounds = []
    for k in range(max(taken)):
        rows = [max(0, min(mb_of[p], n_of[p] - k * step)) if mb_of[p] else 0 for p in range(P)]
        launches = max((rows[p] + micro_of[p] - 1) // micro_of[p] for p in range(P) if rows[p])
        rounds.append((rows, [(k * step + j * micro_step, [max(0, min(micro_of[p], rows[p] - j * micro_step)) if rows[p] else 0 for p in range(P)])
                              for j in range(launches)]))
    return accumulated, taken, rounds


class _PolicySet(_ActorLaunch):
    """What the two kinds of set share: the dcomp_policy_set handle over the members, and the members' weights."""

    def _create(self, actors, slot_policy):
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

    @staticmethod
    def _random_members(num_ue, num_bs, hidden, activation, seed, bias_std, device, num_policies, value):
        return [FcnetActor('multi', num_ue, num_bs, FcnetActor.random_weights('multi', num_ue, num_bs, hidden, seed + p, bias_std), activation, device,
                           value_weights=FcnetActor.random_value_weights('multi', num_ue, num_bs, hidden, seed + p, bias_std) if value else None)
                for p in range(num_policies)]


class PerUEActor(_PolicySet):
    """A set of FcnetActors, one per UE slot (or per group of slots), running as one HIP kernel launch.  ``actions``, ``value`` and
    ``act`` are FcnetActor's: same arguments, same checks, same [E, U] outputs."""
    _ACTIONS, _ACTIONS_V = 'dcomp_policy_set_actions', 'dcomp_policy_set_actions_v'

    def __init__(self, actors, slot_policy=None):
        self._create(actors, slot_policy)

    @classmethod
    def random(cls, num_ue, num_bs, hidden=256, activation='tanh', seed=0, bias_std=0.0, device='cuda', num_policies=None, slot_policy=None,
               value=True):
        """Random-init members (policy p from seed + p, as FcnetActor.random_weights / random_value_weights) for tools and tests."""
        P = int(num_ue) if num_policies is None else int(num_policies)
        return cls(cls._random_members(num_ue, num_bs, hidden, activation, seed, bias_std, device, P, value), slot_policy)

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


_STATIC_WORDS = {}


def static_uid_words(num_envs, num_ue, device):
    """The uid words of a static env, where slot s is UE s + 1 throughout: int16 [num_envs, num_ue], held once per device and width (a
    prefix of the largest batch asked for so far)."""
    key = (torch.device(device), int(num_ue))
    held = _STATIC_WORDS.get(key)
    if held is None or held.shape[0] < num_envs:
        held = _STATIC_WORDS[key] = torch.arange(1, int(num_ue) + 1, dtype=torch.int16, device=device).repeat(int(num_envs), 1)
    return held[:int(num_envs)]


class PerIdActor(_PolicySet):
    """A set of FcnetActors keyed by UE ID, running as one HIP kernel launch (include/dcomp_policy_set_uid.h): member p is the policy
    of the UE with id p + 1, wherever that UE stands in an env's list.  The launch for envs with UE arrival / departure; on a static
    env, where slot s is UE s + 1, it is PerUEActor with the identity map, bit for bit.  ``actions`` and ``value`` take the uid words
    the observations stand in (``uid=``, int16 [E, U]: env.uid); ``act`` takes them from the env.  Slots whose word is 0 get action 0
    and 0.0 in every other output.  Not a PerUEActor: what refuses a slot-keyed set keeps refusing exactly that."""

    def __init__(self, actors):
        self._create(actors, None)                               # (the handle's slot table plays no part in the launch by id)

    @classmethod
    def random(cls, num_ue, num_bs, num_policies, hidden=256, activation='tanh', seed=0, bias_std=0.0, device='cuda', value=True):
        """Random-init members (policy p from seed + p, as PerUEActor.random) for tools and tests; num_policies: env.max_id."""
        return cls(cls._random_members(num_ue, num_bs, hidden, activation, seed, bias_std, device, int(num_policies), value))

    def member_of_id(self, ue_id):
        """The member that decides for the UE with this 1-based id (the id field of its uid word)."""
        if not 1 <= int(ue_id) <= self.num_policies:
            raise ValueError(f"UE id {ue_id} outside 1 ... {self.num_policies}")
        return self.members[int(ue_id) - 1]

    def check_env(self, env):
        """The set has a policy for every UE the env will ever list (the device's rule for ids beyond the set, zeros, is for C callers)."""
        if env.kind != self.kind or env.U != self.U or env.B != self.B:
            raise ValueError("the env's kind / UE slots / stations differ from the actor's")
        if env.max_id > self.num_policies:
            raise ValueError(f"the env lists UE ids up to {env.max_id} (env.max_id), the set has {self.num_policies} policies: build one member per id")

    def uid_of(self, env):
        """The env's uid words as the launch takes them: env.uid on a dynamic env, the constant words 1 ... U on a static one."""
        return env.uid.view(env.E, env.U) if env.uid is not None else static_uid_words(env.E, env.U, self.device)

    def actions(self, obs, *, uid, compact=False, sample=True, seed=0, step=0, row_base=0, out=None, logits=None, logp=None, vf=None):
        """FcnetActor.actions with the row at (env, slot) going through member (uid[env, slot]'s id) - 1; uid: int16 [E, U]."""
        return self._launch_uid(obs, uid, compact, sample, seed, step, row_base, out, logits, logp, vf, True)

    def value(self, obs, *, uid, compact=False, out=None):
        """FcnetActor.value, every row through the value trunk of its UE's member."""
        E, rows = self._batch(obs, compact)
        if out is None:
            out = torch.empty(rows, dtype=torch.float32, device=self.device)
        self._launch_uid(obs, uid, compact, False, 0, 0, 0, None, None, None, out, False)
        return out

    def _launch_uid(self, obs, uid, compact, sample, seed, step, row_base, out, logits, logp, vf, policy):
        E, out, run = self._checked_run(obs, compact, sample, seed, step, row_base, None, out, logits, logp, vf, policy)
        self._check(uid, torch.int16, E * self.U, 'uid')
        with torch.cuda.device(self.device):
            _lib.check(self._L.dcomp_policy_set_actions_uid(self._h, ctypes.byref(run), ctypes.c_void_p(obs.data_ptr()), ctypes.c_void_p(uid.data_ptr()),
                                                            ctypes.c_void_p(out.data_ptr()) if policy else None,
                                                            ctypes.c_void_p(vf.data_ptr()) if vf is not None else None, self._stream()))
        return out

    def act(self, env, sample=True, obs=None, compact=False, out=None, logp=None, vf=None, logits=None):
        """FcnetActor.act with every UE's own policy, the UE known by the id in env.uid: draws keyed as there."""
        self.check_env(env)
        return self.actions(env.obs if obs is None else obs, uid=self.uid_of(env), compact=compact, sample=sample, seed=env.seed_value,
                            step=env.time + max(env.episode, 0) * env.episode_length, row_base=env.env_id_base * self.U, out=out, logp=logp, vf=vf,
                            logits=logits)


def policy_rows_by_id_reference(batch, num_policies):
    """The specification of policy_rows_by_id, in numpy: per policy p the ascending int64 array of the source rows t E U + e U + s of a
    collect(..., by_ue=True) batch with live = 1 whose uid word holds id p + 1 (bit 15, "arrived during the episode", is not part of
    the id).  batch: anything with 'uid' and 'live' of T E U elements each."""
    ids, _ = uid_fields(np.asarray(torch.as_tensor(batch['uid']).cpu()).reshape(-1))
    live = np.asarray(torch.as_tensor(batch['live']).cpu()).reshape(-1)
    if ids.size != live.size:
        raise ValueError(f"uid has {ids.size} words, live {live.size} rows")
    rows = [[] for _ in range(int(num_policies))]
    for s in range(live.size):
        if live[s] and 1 <= ids[s] <= int(num_policies):
            rows[int(ids[s]) - 1].append(s)
    return [np.asarray(r, dtype=np.int64) for r in rows]


def policy_rows_by_id(batch, num_policies):
    """The row split of a collect(..., by_ue=True) batch by UE id: per policy p the ascending int64 tensor, on the batch's device, of
    the source rows with live = 1 whose uid word holds id p + 1.  The tensors are disjoint and together are live_rows(batch) (every
    id of a counted row being one of the set's: collect() holds env.max_id to that).  One stable sort by policy key and ONE host read,
    of the P counts."""
    P = int(num_policies)
    ids, _ = uid_fields(batch['uid'].reshape(-1))
    live = batch['live'].reshape(-1)
    if ids.numel() != live.numel():
        raise ValueError(f"uid has {ids.numel()} words, live {live.numel()} rows")
    key = torch.where((live != 0) & (ids >= 1) & (ids <= P), ids - 1, torch.full_like(ids, P))      # P: a row of no policy
    order = torch.sort(key, stable=True).indices
    counts = torch.bincount(key, minlength=P + 1)[:P].tolist()
    return list(torch.split(order[:sum(counts)], counts))


class PerUELearner:
    """PPO for a PerUEActor: one PPOLearner per member, each with its own Adam state and its own kl_coeff -- RLlib likewise gives each
    policy its own batch, its own advantage standardisation and its own KL coefficient.  Every update lands in the member's handle,
    which the set's next launch reads.

    ppo_kwargs are PPOLearner's.  minibatch_rows and max_rows are PER POLICY, and the workspaces are P times one learner's: max_rows
    should be a policy's minibatch, not the batch.  ``update`` runs the P updates one after the other, P x minibatches x (gathers +
    four launches), so small per-policy batches are bound by launches; ``update(grouped=True)`` trains all policies in one launch
    round per minibatch round (include/dcomp_learner_group.h) and leaves every learner in the same state, bit for bit.  The two can
    be mixed with each other and with calls on a member learner.  ``update(micro_rows=, grad_clip=)`` are PPOLearner.update's, per
    policy, on both paths: grouped, the policies' accumulators are one [P, flat] and one [P, 8] tensor and a micro-batch round is one
    launch round (include/dcomp_learner_group_accum.h); with micro_rows the workspaces are sized by the micro-batch, P times over."""

    _ACTOR = PerUEActor

    def __init__(self, actor, **ppo_kwargs):
        if not isinstance(actor, self._ACTOR):
            raise ValueError(f"actor must be a {self._ACTOR.__name__}")
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

    def _batch_rows(self, batch):
        """Per policy the source rows of the batch it trains on."""
        return self.rows_of(int(batch['actions'].numel()))

    def update(self, batch, num_sgd_iter=30, minibatch_rows=None, seed=0, grouped=False, micro_rows=None, grad_clip=None):
        """PPO's SGD phase on one collect(env, per_ue_actor, ..., dist_inputs=True) batch, rows or compact record: policy p's
        PPOLearner.update on the source rows whose UE slot maps to p (rows=), with seed + p.  Returns one statistics dict per policy
        (None for a policy no slot maps to, whose state stays untouched).

        grouped=True: the same update with all policies in one launch round per minibatch round.  Every policy keeps its own
        advantage standardisation, its own permutations (a generator seeded seed + p), its own minibatch boundaries, Adam state and
        kl_coeff; round k hands every policy its k-th minibatch through one [P, rows] index into the batch where it lies (both batch
        formats), and a policy with fewer minibatches sits the later rounds out.  One synchronisation at the end.  The learners'
        states and the returned statistics are those of grouped=False, bit for bit.

        micro_rows / grad_clip (both None: the paths above, unchanged) are PPOLearner.update's, per policy: a minibatch is trained as
        zeroed accumulators, one accumulate per micro-batch of micro_rows positions, finish (1 / N of the policy's minibatch, the
        global-norm clip of that policy's gradient) and apply; a policy's minibatch may then be larger than max_rows.  Sequential,
        the two are handed to every member's update.  Grouped, a minibatch round zeroes the [P, flat] / [P, 8] accumulators, makes one
        dcomp_learner_group_accumulate per micro-batch round (a policy whose minibatch is exhausted sits it out), one
        dcomp_learner_group_accum_finish and one dcomp_learner_group_apply: the sequential update with the same arguments, bit for
        bit."""
        rows = self._batch_rows(batch)
        if grouped:
            return self._update_grouped(batch, rows, int(num_sgd_iter), minibatch_rows, int(seed), micro_rows, grad_clip)
        return [ln.update(batch, num_sgd_iter=num_sgd_iter, minibatch_rows=minibatch_rows, seed=int(seed) + p, rows=rows[p], check_rows=False,
                          micro_rows=micro_rows, grad_clip=grad_clip)
                if rows[p].numel() else None                     # (check_rows: _batch_rows() built them, distinct and in range)
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

    # ------------------------------------------------------------------ the group's calls (include/dcomp_learner_group.h, dcomp_learner_group_accum.h)
    @property
    def flat_size(self):
        """Elements of a member's flat gradient array (the members have one shape)."""
        return self.learners[0].flat_size

    def new_accumulators(self):
        """(acc float32 [P, flat_size], sums float64 [P, 8]) on the set's device, zeroed: row p is policy p's PPOLearner.new_accumulators()."""
        P = len(self.learners)
        return (torch.zeros((P, self.flat_size), dtype=torch.float32, device=self.device),
                torch.zeros((P, _lib.ACCUM_SUMS), dtype=torch.float64, device=self.device))

    def _accumulators(self, acc, sums):
        P, a = len(self.learners), self.learners[0].actor
        a._check(acc, torch.float32, P * self.flat_size, 'acc')
        a._check(sums, torch.float64, P * _lib.ACCUM_SUMS, 'sums')
        return ctypes.c_void_p(acc.data_ptr()), ctypes.c_void_p(sums.data_ptr())

    def _per_policy(self, ctype, values, what):
        """A host array [P] of a per-policy argument: one number for all, or one per policy."""
        P = len(self.learners)
        values = [values] * P if not isinstance(values, (list, tuple)) else list(values)
        if len(values) != P:
            raise ValueError(f"{what} has {len(values)} entries for {P} policies")
        return (ctype * P)(*values)

    def group_batch(self, source, index):
        """The batch of the group's calls: source a dict of the flattened sample-batch tensors as PPOLearner.grads_indexed takes it
        ('obs' or 'obs_compact', and the six per-row inputs, the advantages standardised by the caller), index a contiguous int32
        [P, stride] device tensor: row p holds policy p's positions -> source rows.  The tensors must outlive the calls made with it."""
        first = self.learners[0]
        obs, fmt, N = first._source_obs(source)
        if not isinstance(index, torch.Tensor) or index.dim() != 2 or index.shape[0] != len(self.learners) or index.shape[1] < 1:
            raise ValueError(f"index must be a contiguous int32 [{len(self.learners)}, stride] device tensor")
        first.actor._check(index, torch.int32, index.numel(), 'index')
        ptr = field_pointers(first.actor, {n: source.get(n) for n in INPUTS}, {INPUT: N})
        return fill(_lib.DcompGroupBatch, obs_format=fmt, source_rows=N, obs=obs.data_ptr(), index=index.data_ptr(), index_stride=int(index.shape[1]), **ptr)

    def _hypers(self):
        """The HOST array of the policies' hyper-parameters as they are now (kl_coeff adapts per policy, at the end of an update)."""
        return (_lib.DcompPpoHyper * len(self.learners))(*[ln._hyper_struct() for ln in self.learners])

    def _active(self, active):
        return active if active is None or isinstance(active, ctypes.Array) else self._per_policy(ctypes.c_int32, [1 if x else 0 for x in active], 'active')

    def _group_call(self, entry, gb, rows, offset, *args, hyper=None):
        """grads or accumulate on positions [offset, offset + rows[p]) of every policy's index row."""
        rows = rows if isinstance(rows, ctypes.Array) else self._per_policy(ctypes.c_int64, [int(r) for r in rows], 'rows')
        if offset < 0 or offset + max(rows) > gb.index_stride:
            raise ValueError(f"offset {offset} + rows reaches past the index's stride {gb.index_stride}")
        b = type(gb).from_buffer_copy(gb)                        # (the stride stays: policy p's row begins p strides behind the pointer)
        b.index, b.rows = gb.index + 4 * int(offset), rows
        with torch.cuda.device(self.device):
            _lib.check(getattr(self.actor._L, entry)(self._group_handle(), ctypes.byref(b), hyper or self._hypers(), *args, self.learners[0].actor._stream()))

    def accumulate_grouped(self, gb, rows, acc, sums, offset=0, hyper=None):
        """PPOLearner.accumulate_indexed for every policy with rows[p] > 0, in one launch round: policy p's positions [offset, offset
        + rows[p]) of its row of the index of gb (group_batch()) are added to acc[p] / sums[p].  Nothing else is written."""
        self._group_call('dcomp_learner_group_accumulate', gb, rows, offset, *self._accumulators(acc, sums), hyper=hyper)

    def finish_grouped(self, acc, sums, grad_clip=None, active=None, stats=None, grad_norm=None, hyper=None):
        """PPOLearner.finish for every policy with active[p] (None: all), in one launch round: policy p's gradients from acc[p] /
        sums[p], clipped by grad_clip (a number for all or one per policy; None / 0: no clipping), its statistics into stats[p] (a
        float32 [P, 5] device tensor, returned; allocated when None), its gradient norm into grad_norm[p] (float32 [P], optional).
        An inactive policy keeps its gradients, its row of stats and its entry of grad_norm.  acc and sums are read only."""
        P, a = len(self.learners), self.learners[0].actor
        clip = grad_clip
        if not isinstance(clip, ctypes.Array):
            each = grad_clip if isinstance(grad_clip, (list, tuple)) else [grad_clip] * P
            clip = self._per_policy(ctypes.c_float, [0.0 if c is None else float(c) for c in each], 'grad_clip')
        if not all(c >= 0.0 for c in clip):
            raise ValueError(f"grad_clip {grad_clip!r} must be >= 0 (None or 0: no clipping)")
        pa, ps = self._accumulators(acc, sums)
        if stats is None:
            stats = torch.zeros((P, _lib.PPO_NUM_STATS), dtype=torch.float32, device=self.device)
        a._check(stats, torch.float32, P * _lib.PPO_NUM_STATS, 'stats')
        if grad_norm is not None:
            a._check(grad_norm, torch.float32, P, 'grad_norm')
        with torch.cuda.device(self.device):
            _lib.check(self.actor._L.dcomp_learner_group_accum_finish(self._group_handle(), pa, ps, hyper or self._hypers(), clip, self._active(active), ctypes.c_void_p(stats.data_ptr()),
                                                                      ctypes.c_void_p(grad_norm.data_ptr()) if grad_norm is not None else None, a._stream()))
        return stats

    def apply_grouped(self, active=None, lr=None):
        """PPOLearner.apply for every policy with active[p] (None: all), each with its own lr, in one launch."""
        lr = lr or self._per_policy(ctypes.c_float, [ln.lr for ln in self.learners], 'lr')
        with torch.cuda.device(self.device):
            _lib.check(self.actor._L.dcomp_learner_group_apply(self._group_handle(), lr, self._active(active), self.learners[0].actor._stream()))

    # ------------------------------------------------------------------ the grouped training step
    def grouped_phases(self, src, rows, adv, plan, num_sgd_iter, seeds, grad_clip=None, lap=lambda name=None: None):
        """The grouped SGD phase as a generator: src the flattened batch (flatten_batch()), rows the policies' source rows, adv every
        policy's standardised advantages in source order, plan = group_plan(...), seeds[p] the seed of policy p's permutations.  Per
        minibatch round of an accumulated plan: zeroed accumulators, one accumulate_grouped per micro-batch round, then (acc, SUM) and
        (sums, SUM) are yielded -- where the ranks of a data-parallel set add theirs together; one set just goes on -- then
        finish_grouped and apply_grouped with the round's active mask.  A plan that is not accumulated makes one
        dcomp_learner_group_grads and one apply per round and yields nothing.  Returns update()'s result."""
        dev, P = self.device, len(self.learners)
        accumulated, taken, rounds = plan
        n_of = [int(rows[p].numel()) for p in range(P)]
        live = [p for p in range(P) if n_of[p]]
        index = torch.zeros((P, max(n_of)), dtype=torch.int32, device=dev)
        gb = self.group_batch(dict(src, advantages=adv), index)
        stats = torch.zeros((len(rounds), P, _lib.PPO_NUM_STATS), dtype=torch.float32, device=dev)
        epochs = {p: sgd_epochs(n_of[p], num_sgd_iter, seeds[p], dev) for p in live}
        as_rows = lambda rr: (ctypes.c_int64 * P)(*rr)         # noqa: E731
        round_active = [(ctypes.c_int32 * P)(*[1 if r else 0 for r in rr]) for rr, _ in rounds]
        launches = [[(off, as_rows(rr)) for off, rr in micro] for _, micro in rounds]
        hyper, lr = self._hypers(), self._per_policy(ctypes.c_float, [ln.lr for ln in self.learners], 'lr')
        if accumulated:
            acc, sums = self.new_accumulators()
            grad_clip = self._per_policy(ctypes.c_float, 0.0 if grad_clip is None else float(grad_clip), 'grad_clip')
        for _ in range(num_sgd_iter):
            for p in live:
                index[p, :n_of[p]] = rows[p].index_select(0, next(epochs[p]))
            for k in range(len(rounds)):
                lap()
                if accumulated:
                    acc.zero_()
                    sums.zero_()
                    for off, rr in launches[k]:
                        self.accumulate_grouped(gb, rr, acc, sums, off, hyper)
                    lap('accumulate')
                    yield acc, SUM
                    yield sums, SUM
                    lap('reduce')
                    self.finish_grouped(acc, sums, grad_clip, round_active[k], stats[k], hyper=hyper)
                    lap('finish')
                else:
                    (off, rr), = launches[k]
                    self._group_call('dcomp_learner_group_grads', gb, rr, off, ctypes.c_void_p(stats[k].data_ptr()), hyper=hyper)
                self.apply_grouped(round_active[k], lr)
                lap('apply')
        # a policy's mean over the rounds it took part in: PPOLearner.update's own reduction of its own [minibatches, 5] tensor
        out = [None] * P
        for p, st in zip(live, close_out([self.learners[p] for p in live], torch.stack([stats[:taken[p], p].contiguous().mean(0) for p in live]))):
            out[p] = st
        return out

    def _update_grouped(self, batch, rows, num_sgd_iter, minibatch_rows, seed, micro_rows=None, grad_clip=None):
        first, P = self.learners[0], len(self.learners)
        src, N, compact = flatten_batch(first.actor, batch)
        # every policy's advantages standardised over its own rows (PPOLearner.update's rule), back in source order in ONE tensor: the
        # row sets are disjoint
        adv = torch.zeros_like(src['advantages'])
        plan = group_plan([int(rows[p].numel()) for p in range(P)], minibatch_rows, [ln.max_rows for ln in self.learners], micro_rows, grad_clip)
        for p in range(P):
            if rows[p].numel():
                adv.index_copy_(0, rows[p], standardize(src['advantages'].index_select(0, rows[p])))
        phases = self.grouped_phases(src, rows, adv, plan, num_sgd_iter, [seed + p for p in range(P)], grad_clip)
        try:
            while True:
                next(phases)                                     # (one set: nothing to add together)
        except StopIteration as stop:
            return stop.value

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


class PerIdLearner(PerUELearner):
    """PPO for a PerIdActor: PerUELearner with the policies' rows picked by UE ID.  ``update`` takes a collect(env, per_id_actor, ...,
    dist_inputs=True, by_ue=True) batch and trains member p on the counted rows (live = 1) of the UE with id p + 1
    (policy_rows_by_id: one sort and one host read per update).  Everything behind the rows is PerUELearner's: sequential and
    grouped=True, micro_rows=, grad_clip=, every policy's own standardisation, seed + p, None for a policy without rows -- a UE
    that was never listed in the batch -- whose state stays untouched.  Data-parallel training of an id-keyed set is not supported."""
    _ACTOR = PerIdActor

    def rows_of(self, num_rows):
        raise NotImplementedError("an id-keyed set has no row split by batch size (its rows depend on the batch's uid words: policy_rows_by_id), and "
                                  "data-parallel training of an id-keyed set is not supported")

    def _batch_rows(self, batch):
        if 'uid' not in batch or 'live' not in batch:
            raise ValueError("the batch has no uid / live: collect it with by_ue=True")
        return policy_rows_by_id(batch, self.actor.num_policies)


__all__ = ['PerUEActor', 'PerUELearner', 'PerIdActor', 'PerIdLearner', 'policy_rows', 'policy_rows_by_id', 'policy_rows_by_id_reference',
           'default_slot_policy', 'group_plan']
