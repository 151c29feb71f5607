"""The data-parallel PPO learner: one rank's PPOLearner on one rank's shard of the sample batch.

Every rank collects on its own env shard (deepcomp_amd.sharded.make_sharded_env, sampler.collect) and trains where the batch lies.
Per minibatch a rank accumulates the UNNORMALISED gradient of its rows (PPOLearner.accumulate, include/dcomp_learner_accum.h), the
ranks add their sums together (one all-reduce of the flat gradient, one of the eight loss sums), and every rank finishes with
1 / N of the GLOBAL row count, the global-norm clip and Adam on identical numbers: the ranks' weights stay identical without ever
being broadcast.  ``check_sync`` holds them to that.

    dp = DataParallelLearner(PPOLearner(actor, max_rows=micro_rows), group=dist.group.WORLD)
    stats = dp.update(batch, num_sgd_iter=30, minibatch_rows=global_minibatch, micro_rows=micro_rows, seed=s, grad_clip=40.0)
    dp.check_sync()

The update is written once, as local phases separated by all-reduce points: ``update_phases`` is a generator that yields
``(tensor, op)`` wherever the ranks meet and goes on once the tensor holds the reduction.  ``update`` drives it with the process
group's all-reduce (``nccl``: the device tensor in place; ``gloo``: staged through the host; no group: the identity, torch.distributed
is not touched); ``run_lockstep`` drives R of them in ONE process, summing each yielded tensor in rank order and writing the sum back
to every rank -- the same code the ranks run, testable on one GPU.

``DataParallelPerUELearner`` is the same for a per-UE policy set (deepcomp_amd.policy_set.PerUELearner, D3-CoMP): one rank's set on
one rank's shard, the same phases through the same drivers.  The policies' accumulators are one [P, flat] and one [P, 8] tensor
(include/dcomp_learner_group_accum.h), so the ranks meet exactly twice per minibatch round whatever P is, and a round is the grouped
update's launch round.  No run on more than one GPU exists yet for either class: lockstep ranks and gloo ranks on one device are what
has been run."""
import hashlib
import math
import time

import numpy as np
import torch

from .learner import ARRAYS, SUM, close_out, flatten_batch, minibatch_plan, minibatch_stats, sgd_epochs, standardize
from .policy_set import group_plan

MIN, MAX = 'min', 'max'


# ---------------------------------------------------------------------------------------------- the phases that need no learner
def advantage_moments(adv):
    """float64 [3] on adv's device: the local sum, sum of squares and count of the advantages -- what the ranks add together."""
    a = adv.reshape(-1).double()
    return torch.stack((a.sum(), (a * a).sum(), torch.tensor(float(a.numel()), dtype=torch.float64, device=a.device)))


def standardize_with(adv, moments):
    """RLlib's standardisation with the moments of the GLOBAL batch: mean = s1 / n, var = max(0, s2 / n - mean^2),
    ((a - mean) / max(1e-4, sqrt(var))) in float64, rounded to float32 once."""
    s1, s2, n = moments.tolist()
    mean = s1 / n
    std = math.sqrt(max(0.0, s2 / n - mean * mean))
    return ((adv.double() - mean) / max(1e-4, std)).float()


def standardize_phases(adv):
    """The advantages standardised over the global batch, as phases: one SUM of the three moments."""
    m = advantage_moments(adv)
    yield m, SUM
    return standardize_with(adv, m)


def shard_agreement_phases(local_rows, minibatch_rows, world, device=None, policies=False):
    """Every rank holds the same number of rows and the GLOBAL minibatch divides by the world size: ValueError otherwise, on every
    rank.  One small SUM: of (n, n^2) -- the ranks agree exactly when world x sum n^2 == (sum n)^2 (exact in float64 below 2^26
    rows).  Returns the rows of this rank's share of a minibatch.  policies: local_rows is a list, the rows of every policy of a
    per-UE set on this rank (0: a policy without slots, on every rank); the one SUM is of a [P, 2] tensor, the policy that differs
    is named, and the share returned is the common one, before a policy's own row count caps it (None: whole batches)."""
    ns = [int(n) for n in local_rows] if policies else [int(local_rows)]
    for n in ns:
        if n < (0 if policies else 1) or n >= 1 << 26:
            raise ValueError(f"a rank's shard has {n} rows: outside [1, 2^26)")
    t = torch.tensor([[float(n), float(n) * float(n)] for n in ns], dtype=torch.float64, device=device)
    t = t if policies else t[0]
    yield t, SUM
    for p, (n, (s1, s2)) in enumerate(zip(ns, t.reshape(-1, 2).tolist())):
        if world * s2 != s1 * s1:
            raise ValueError(f"the ranks hold different numbers of rows{f' of policy {p}' if policies else ''} (this rank {n}, mean {s1 / world:g}): "
                             "a data-parallel update needs equal shards")
    if minibatch_rows is None:
        return None if policies else ns[0]
    mb = int(minibatch_rows)
    if mb < world or mb % world:
        raise ValueError(f"minibatch_rows {mb} is the GLOBAL minibatch: it must be a positive multiple of the world size {world}")
    return mb // world if policies else min(mb // world, ns[0])


def drive(phases, reduce):
    """Run a generator of phases to its end: every yielded (tensor, op) goes through reduce(tensor, op), which leaves the reduction
    in the tensor.  Returns what the generator returns."""
    try:
        item = next(phases)
        while True:
            reduce(*item)
            item = next(phases)
    except StopIteration as stop:
        return stop.value


def group_reduce(group):
    """reduce(tensor, op) over a torch.distributed process group: nccl reduces the device tensor in place; any other backend (gloo)
    gets it staged through the host.  group None: the identity, torch.distributed is not imported."""
    if group is None:
        return lambda t, op: t
    import torch.distributed as dist
    ops = {SUM: dist.ReduceOp.SUM, MIN: dist.ReduceOp.MIN, MAX: dist.ReduceOp.MAX}
    direct = dist.get_backend(group) == 'nccl'

    def reduce(t, op):
        if direct or not t.is_cuda:
            dist.all_reduce(t, op=ops[op], group=group)
        else:
            host = t.cpu()                                   # (synchronises with the stream that wrote t)
            dist.all_reduce(host, op=ops[op], group=group)
            t.copy_(host)
        return t
    return reduce


def weights_checksum(arrays):
    """sha256 over the twelve master-weight arrays' bytes, in ARRAYS' order."""
    h = hashlib.sha256()
    for n in ARRAYS:
        h.update(np.ascontiguousarray(arrays[n], dtype=np.float32).tobytes())
    return h.hexdigest()


class DataParallelLearner:
    """One rank of a data-parallel PPO learner.  learner: this rank's PPOLearner (every rank built from the same weights and
    hyper-parameters).  group: the torch.distributed process group the ranks meet in (dist.group.WORLD for the default one); None: no
    process group -- one rank, or a rank of run_lockstep, which gives rank and world itself."""

    def __init__(self, learner, group=None, rank=None, world=None):
        self.learner, self.group = learner, group
        if group is not None:
            import torch.distributed as dist
            self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        else:
            self.rank, self.world = int(rank or 0), int(world or 1)
        if not 0 <= self.rank < self.world:
            raise ValueError(f"rank {self.rank} outside [0, {self.world})")
        self._reduce = group_reduce(group)
        self.profile = False                                 # True: synchronise around every phase and add its seconds to self.seconds
        self.seconds = {'accumulate': 0.0, 'reduce': 0.0, 'finish': 0.0, 'apply': 0.0}
        self._lap_start = 0.0

    def _lap(self, name=None):
        """profile: synchronise and add the seconds since the last lap to self.seconds[name]."""
        if self.profile:
            torch.cuda.synchronize(self.learner.device)
            now = time.perf_counter()
            if name is not None:
                self.seconds[name] += now - self._lap_start
            self._lap_start = now

    def update_phases(self, batch, num_sgd_iter=30, minibatch_rows=None, micro_rows=None, seed=0, grad_clip=None):
        """update() as a generator of local phases: yields (tensor, op) at every all-reduce point and expects the reduction in the
        tensor when it is resumed.  Returns update()'s result."""
        L = self.learner
        src, N, compact = flatten_batch(L.actor, batch)
        mb = yield from shard_agreement_phases(N, minibatch_rows, self.world, L.device)
        mb, micro, _ = minibatch_plan(N, mb, L.max_rows, micro_rows, grad_clip, "a rank's share of a minibatch is {} rows", ": give micro_rows")
        src['advantages'] = yield from standardize_phases(src['advantages'])
        acc, sums = L.new_accumulators()
        starts, stats = minibatch_stats(N, mb, L.device)
        for perm in sgd_epochs(N, num_sgd_iter, int(seed) + self.rank, L.device):      # each rank shuffles its own rows
            picks = perm.to(torch.int32) if compact else perm
            for i, s in enumerate(starts):
                self._lap()
                yield from L.accumulated_step(src, compact, picks[s:s + mb], micro, acc, sums, grad_clip, stats[i], lap=self._lap)
        # the statistics come from the reduced sums: the same numbers, and so the same kl_coeff, on every rank
        return close_out([L], stats.mean(0)[None])[0]

    def update(self, batch, num_sgd_iter=30, minibatch_rows=None, micro_rows=None, seed=0, grad_clip=None):
        """PPO's SGD phase on this rank's shard of a collect(..., dist_inputs=True) batch (rows or the compact record), in step with
        the other ranks.  The ranks must hold equally many rows; minibatch_rows is the GLOBAL minibatch (a multiple of the world
        size; default: the whole batch), of which each rank trains its 1 / world; micro_rows as in PPOLearner.update, per rank.  The
        advantages are standardised over the global batch; each rank permutes its own rows with a generator seeded seed + rank;
        per minibatch: zeroed accumulators, accumulate, all-reduce of acc and of sums, finish (1 / N global, grad_clip), apply.
        kl_coeff is adapted from the global statistics.  Returns the last iteration's mean statistics and the new kl_coeff."""
        return drive(self.update_phases(batch, num_sgd_iter, minibatch_rows, micro_rows, seed, grad_clip), self._reduce)

    def check_sync_phases(self):
        """MIN and MAX over the ranks of a checksum of the master weights (four 62-bit words of their sha256): RuntimeError where they
        differ -- the ranks' weights are no longer the same bits."""
        digest = bytes.fromhex(weights_checksum(self.learner.read('weights')))
        words = [int.from_bytes(digest[8 * i:8 * i + 8], 'little') >> 2 for i in range(4)]
        lo = torch.tensor(words, dtype=torch.int64, device=self.learner.device)
        hi = lo.clone()
        yield lo, MIN
        yield hi, MAX
        if not torch.equal(lo, hi):
            raise RuntimeError(f"rank {self.rank}: the ranks' master weights differ (checksum words min {lo.tolist()} max {hi.tolist()})")
        return digest.hex()

    def check_sync(self):
        """Raise RuntimeError when the ranks' master weights differ; returns this rank's sha256 of them."""
        return drive(self.check_sync_phases(), self._reduce)


class DataParallelPerUELearner(DataParallelLearner):
    """One rank of a data-parallel per-UE policy set.  per_ue_learner: this rank's PerUELearner (every rank built from the same
    weights and hyper-parameters); group, rank, world as DataParallelLearner takes them.  The same drivers run it: update() with the
    process group's all-reduce, run_lockstep() R of them in one process."""

    def __init__(self, per_ue_learner, group=None, rank=None, world=None):
        super().__init__(per_ue_learner, group, rank, world)
        self.set = per_ue_learner

    def update_phases(self, batch, num_sgd_iter=30, minibatch_rows=None, micro_rows=None, seed=0, grad_clip=None):
        """update() as a generator of local phases (DataParallelLearner.update_phases).  Returns update()'s result."""
        S, dev = self.set, self.set.device
        P, first = len(S.learners), S.learners[0]
        src, N, compact = flatten_batch(first.actor, batch)
        rows = S.rows_of(N)
        n_of = [int(r.numel()) for r in rows]
        share = yield from shard_agreement_phases(n_of, minibatch_rows, self.world, dev, policies=True)
        plan = group_plan(n_of, share, [ln.max_rows for ln in S.learners], micro_rows, grad_clip, accumulate=True,
                          noun="a rank's share of a policy's minibatch is {} rows", hint=": give micro_rows")
        adv = torch.zeros_like(src['advantages'])
        mine = [src['advantages'].index_select(0, rows[p]) for p in range(P)]
        if self.world == 1:                                      # nobody to add moments with: the set's own rule, the grouped update's bits
            done = [standardize(a) if a.numel() else a for a in mine]
        else:                                                    # per policy over the global rows: ONE SUM of the [P, 3] moments
            moments = torch.stack([advantage_moments(a) for a in mine])
            yield moments, SUM
            done = [standardize_with(a, m) if a.numel() else a for a, m in zip(mine, moments.cpu())]
        for p in range(P):
            adv.index_copy_(0, rows[p], done[p])
        # each rank shuffles its own rows of each policy; the statistics come from the reduced sums: the same numbers, and so the
        # same kl_coeff per policy, on every rank
        seeds = [int(seed) + p + P * self.rank for p in range(P)]
        return (yield from S.grouped_phases(src, rows, adv, plan, int(num_sgd_iter), seeds, grad_clip, lap=self._lap))

    def update(self, batch, num_sgd_iter=30, minibatch_rows=None, micro_rows=None, seed=0, grad_clip=None):
        """PerUELearner.update(grouped=True) on this rank's shard of a collect(env, per_ue_actor, ..., dist_inputs=True) batch, in
        step with the other ranks.  Per policy the ranks must hold equally many rows; minibatch_rows is the GLOBAL per-policy
        minibatch (a multiple of the world size; default: a policy's whole batch), of which each rank trains its 1 / world;
        micro_rows as in PerUELearner.update, per rank.  The advantages are standardised per policy over the global rows (one SUM of
        a [P, 3] moments tensor); policy p on rank r permutes its rows with a generator seeded seed + p + P r -- a world of one is
        the grouped update, bit for bit, and standardises as it does; per minibatch round: zeroed [P, flat] / [P, 8] accumulators,
        one grouped accumulate per micro-batch round, all-reduce of acc and of sums, grouped finish (1 / N of the global count per
        policy, grad_clip per policy's gradient), grouped apply.  kl_coeff is adapted per policy from the global statistics.  Returns
        one dict per policy (None for a policy no slot maps to)."""
        return drive(self.update_phases(batch, num_sgd_iter, minibatch_rows, micro_rows, seed, grad_clip), self._reduce)

    def check_sync_phases(self):
        """One MIN and one MAX over the ranks of [P, 4] checksum words (62 bits each of the sha256 of a policy's master weights):
        RuntimeError naming the policies whose weights differ.  Returns this rank's sha256 per policy."""
        digests = [bytes.fromhex(weights_checksum(ln.read('weights'))) for ln in self.set.learners]
        lo = torch.tensor([[int.from_bytes(d[8 * i:8 * i + 8], 'little') >> 2 for i in range(4)] for d in digests], dtype=torch.int64, device=self.set.device)
        hi = lo.clone()
        yield lo, MIN
        yield hi, MAX
        differ = torch.nonzero((lo != hi).any(1)).reshape(-1).tolist()
        if differ:
            raise RuntimeError(f"rank {self.rank}: the ranks' master weights differ for policy {', '.join(map(str, differ))}")
        return [d.hex() for d in digests]


def run_lockstep(dp_learners, batches=None, *, phases='update', host_staged=False, seconds=None, **kw):
    """Drive R DataParallelLearners (ranks 0 ... R - 1, built with rank= and world=R, no process group) in ONE process: rank r runs
    update_phases(batches[r], **kw) (phases='check_sync': check_sync_phases()); at every all-reduce point the R yielded tensors are
    reduced in rank order -- a SUM as ((t0 + t1) + t2) + ... -- and the result is written back to every rank.  host_staged: the
    tensors are summed on the host, as the gloo backend has them (the same bits: IEEE additions in the same order).  seconds: a dict
    whose 'reduce' entry receives the time spent in the reductions, synchronised (a rank's own 'reduce' clock also sees the other
    ranks' phases here).  Returns the ranks' results."""
    R = len(dp_learners)
    if any(d.group is not None or d.world != R or d.rank != r for r, d in enumerate(dp_learners)):
        raise ValueError("run_lockstep takes ranks 0 ... R - 1 of world R in order, none of them with a process group")
    if phases == 'update':
        if batches is None or len(batches) != R:
            raise ValueError("one batch per rank")
        gens = [d.update_phases(b, **kw) for d, b in zip(dp_learners, batches)]
    elif phases == 'check_sync':
        gens = [d.check_sync_phases() for d in dp_learners]
    else:
        raise ValueError("phases is 'update' or 'check_sync'")
    results = [None] * R
    while True:
        items, done = [], 0
        for r, g in enumerate(gens):
            try:
                items.append(next(g))
            except StopIteration as stop:
                results[r] = stop.value
                done += 1
        if done == R:
            return results
        if done or len({op for _, op in items}) != 1 or len({(tuple(t.shape), t.dtype) for t, _ in items}) != 1:
            raise RuntimeError("the ranks left lockstep: they reached different all-reduce points")
        op, first = items[0][1], items[0][0]
        if seconds is not None and first.is_cuda:
            torch.cuda.synchronize(first.device)
        t0 = time.perf_counter()
        where = torch.device('cpu') if host_staged else first.device
        if op == SUM:
            total = first.to(where, copy=True)
            for t, _ in items[1:]:
                total += t.to(where)
        else:
            stack = torch.stack([t.to(where) for t, _ in items])
            total = stack.amin(0) if op == MIN else stack.amax(0)
        for t, _ in items:
            t.copy_(total)
        if seconds is not None:
            if first.is_cuda:
                torch.cuda.synchronize(first.device)
            seconds['reduce'] = seconds.get('reduce', 0.0) + time.perf_counter() - t0
