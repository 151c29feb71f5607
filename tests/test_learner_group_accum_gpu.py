"""GPU tests of the grouped accumulated gradients (include/dcomp_learner_group_accum.h; PerUELearner.update(micro_rows=, grad_clip=),
new_accumulators / accumulate_grouped / finish_grouped / apply_grouped; deepcomp_amd.dp_learner.DataParallelPerUELearner;
tools/dp_train.py --per-ue).

The reference everywhere is the existing per-member path -- PPOLearner.accumulate_indexed / finish / apply and PPOLearner.update(rows=,
micro_rows=, grad_clip=) -- which tests/test_learner_accum_gpu.py holds to the float64 model.  A policy's arithmetic is the
per-learner kernels' own text and every order of summation depends on that policy's row count alone, so the comparisons are EXACT:
torch.equal on accumulators, np.array_equal on state_dict() and gradients, == on the statistics dicts.  The one place where two
DIFFERENT paths are compared (test 5: accumulated against unaccumulated) says what is exact there and why the rest is not.

Shapes: tests/group_cases.py's tables (tests/test_learner_group_accum_cpu.py shows what they reach).  A sample batch is collected once per
shape and left unchanged."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fcnet_support as fs
from tests import group_cases as ac
from tests.fcnet_cases import HYPER
from tests.fcnet_support import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = ac.CHUNK
PATTERN = 0x5A5A5A5A                                      # as float32 1.536e16: finite, so a gradient can hold it


def _case(shape, compact=False, key=None):
    """(batch, two PerUELearner twins' factory) of a shape of the CPU table."""
    U, B, H, E, T, slots = shape
    batch = fs.group_collected(('group-accum', key, tuple(slots), U, B, H, E, T, compact), U, B, H, 'tanh', E, T, slots, compact)
    return batch, lambda max_rows: fs.per_ue_learner(fs.policy_set(U, B, H, 'tanh', slots), max_rows)


def _pattern_gradients(torch, learner):
    """The handle's gradients filled with PATTERN: finish of an accumulator that holds it, over a count of one (g = acc x 1)."""
    acc, sums = learner.new_accumulators()
    acc.view(torch.int32).fill_(PATTERN)
    sums[4] = 1.0
    learner.finish(acc, sums)
    got = fs.flat(learner.read('grads'))
    assert np.all(got.view(np.int32) == PATTERN)
    return got


def _index(torch, P, width, N, seed):
    return torch.randint(0, N, (P, width), generator=torch.Generator(device='cuda').manual_seed(seed), device='cuda', dtype=torch.int32)


# ---------------------------------------------------------------------------------------------- 1: accumulate
@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_group_accumulate_is_p_sgd_accumulate_calls(torch_cuda, compact):
    """dcomp_learner_group_accumulate (the C call) against dcomp_sgd_accumulate per member on twins: 4 500 and 2 250 positions (3 and 2
    weight-gradient chunks), a third member without rows; a second call with the counts swapped carries the running sums in.  acc and
    sums are equal per slice after each call; the idle member's slices keep their byte pattern; no handle's gradients and no
    statistics buffer is written."""
    torch = torch_cuda
    from deepcomp_amd import _lib
    from deepcomp_amd.learner import PPOLearner
    U, B, H, E, T, slots = ac.CALL
    batch, _ = _case(ac.CALL, compact)
    mk = lambda: [PPOLearner(m, max_rows=max(ac.CALL_ROWS), **dict(HYPER, lr=1e-3, kl_coeff=0.2 + 0.1 * p))      # noqa: E731
                  for p, m in enumerate(fs.policy_set(U, B, H, 'tanh', slots).members)]
    grp, seq = mk(), mk()
    src = fs.source(batch, grp[0].actor, own_advantages=True)
    N = src['actions'].shape[0]
    index = _index(torch, 3, max(ac.CALL_ROWS), N, 9)
    kept_stats = [ln.grads_indexed(src, index[p, :50].contiguous()) for p, ln in enumerate(grp)]      # gradients and statistics of an earlier call
    kept_bits = [s.clone() for s in kept_stats]
    kept = [fs.flat(ln.read('grads')) for ln in grp]
    rc, h, msg = fs.c_group(grp)
    assert rc == 0, msg
    L = _lib.load()
    F = grp[0].flat_size
    acc = torch.zeros((3, F), dtype=torch.float32, device='cuda')
    sums = torch.zeros((3, _lib.ACCUM_SUMS), dtype=torch.float64, device='cuda')
    acc[2].view(torch.int32).fill_(PATTERN)
    sums[2].view(torch.int64).fill_(PATTERN)
    twin = [ln.new_accumulators() for ln in seq]
    hy = fs.c_hypers(grp)
    for rows in (ac.CALL_ROWS, [ac.CALL_ROWS[1], ac.CALL_ROWS[0], 0]):
        b = fs.c_group_batch(src, index, rows, compact)
        assert L.dcomp_learner_group_accumulate(h, ctypes.byref(b), hy, ctypes.c_void_p(acc.data_ptr()), ctypes.c_void_p(sums.data_ptr()),
                                                grp[0].actor._stream()) == 0, L.dcomp_last_error()
        for p in (0, 1):
            seq[p].accumulate_indexed(src, index[p, :rows[p]].contiguous(), *twin[p])
            assert torch.equal(acc[p], twin[p][0]) and torch.equal(sums[p], twin[p][1]), (rows, p)
    assert sums[:2, 4].tolist() == [6750.0, 6750.0] and bool(torch.isfinite(acc[:2]).all()) and float(acc[0].abs().max()) > 0
    assert not torch.equal(acc[0], acc[1])
    assert bool((acc[2].view(torch.int32) == PATTERN).all()) and bool((sums[2].view(torch.int64) == PATTERN).all())
    for p, ln in enumerate(grp):
        assert np.array_equal(fs.flat(ln.read('grads')), kept[p]), p
        assert torch.equal(kept_stats[p], kept_bits[p])
    assert L.dcomp_learner_group_destroy(h) == 0


# ---------------------------------------------------------------------------------------------- 2: finish
@pytest.mark.parametrize('H', [32, 64])
def test_group_finish_is_p_accum_finish_calls(torch_cuda, H):
    """finish_grouped against PPOLearner.finish per member: hidden 32 (3 751 entries: less than one norm block) and 64 (11 591: three
    norm partials).  One clip per policy: policy 0's bites, policy 1's does not, policy 2 has none but its norm is asked for, policy 3
    is masked out and keeps pattern-filled gradients, its statistics row and its norm entry.  acc and sums are read only; a second
    finish gives the same bits."""
    torch = torch_cuda
    batch, mk = _case(ac.FINISH[H])
    grp, seq = mk(128), mk(128)
    P = 4
    for s in (grp, seq):
        for p, ln in enumerate(s.learners):
            ln.hyper['kl_coeff'] = 0.2 + 0.1 * p
    src = fs.source(batch, grp.learners[0].actor, own_advantages=True)
    index = _index(torch, P, 100, src['actions'].shape[0], 5)
    rows = [100, 77, 50, 64]
    acc, sums = grp.new_accumulators()
    assert tuple(acc.shape) == (P, {32: 3751, 64: 11591}[H]) and tuple(sums.shape) == (P, 8) and grp.flat_size == acc.shape[1]
    grp.accumulate_grouped(grp.group_batch(src, index), rows, acc, sums)
    norms = []
    for p, ln in enumerate(seq.learners):                                              # the unclipped norms, from the per-member call
        n = torch.zeros(1, device='cuda')
        ln.finish(acc[p], sums[p], grad_norm=n)
        norms.append(float(n))
    clips = [0.5 * norms[0], 2.0 * norms[1], 0.0, 0.5 * norms[3]]
    pattern = [_pattern_gradients(torch, s.learners[3]) for s in (grp, seq)][0]
    acc0, sums0 = acc.clone(), sums.clone()
    runs = []
    for _ in range(2):
        stats = torch.full((P, 5), -777.0, device='cuda')
        norm = torch.full((P,), -777.0, device='cuda')
        assert grp.finish_grouped(acc, sums, clips, [1, 1, 1, 0], stats, norm) is stats
        assert torch.equal(acc, acc0) and torch.equal(sums, sums0)
        got = [fs.flat(ln.read('grads')) for ln in grp.learners]
        runs.append((stats.cpu().numpy(), norm.cpu().numpy(), got))
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][2], runs[1][2])) and all(np.array_equal(runs[0][i], runs[1][i]) for i in (0, 1))
    stats, norm, got = runs[0]
    for p in range(3):
        n = torch.zeros(1, device='cuda')
        want = seq.learners[p].finish(acc[p], sums[p], grad_clip=clips[p], grad_norm=n).cpu().numpy()
        assert np.array_equal(stats[p], want) and np.all(np.isfinite(want)), p
        assert norm[p] == float(n) == np.float32(norms[p]), p
        assert np.array_equal(got[p], fs.flat(seq.learners[p].read('grads'))), p
    unclipped = [acc0[p].cpu().numpy() * np.float32(1.0 / rows[p]) for p in range(3)]
    assert norms[0] > clips[0] and not np.array_equal(got[0], unclipped[0]) and np.abs(got[0]).max() < np.abs(unclipped[0]).max()
    assert norms[1] < clips[1] and np.array_equal(got[1], unclipped[1]) and np.array_equal(got[2], unclipped[2])
    assert np.array_equal(got[3], pattern) and np.all(stats[3] == -777.0) and norm[3] == -777.0
    # without a norm anywhere (no clip, none asked for) the norm launch is skipped: the gradients are the unclipped ones
    grp.finish_grouped(acc, sums, None, [1, 1, 1, 0])
    for p in range(3):
        assert np.array_equal(fs.flat(grp.learners[p].read('grads')), unclipped[p]), p
    with pytest.raises(ValueError, match='grad_clip'):
        grp.finish_grouped(acc, sums, [0.0, -1.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        grp.finish_grouped(acc[:3], sums)


# ---------------------------------------------------------------------------------------------- 3: more members than one slice
def test_more_members_than_one_launch_slice(torch_cuda):
    """DCOMP_GROUP_SLICE + 1 members (the shape family of tests/test_learner_group_gpu.py's slice test), every fifth one idle -- the
    first of the first slice among them; the one member of the second slice takes part.  Accumulate (two calls) + finish + apply
    through the group equal the per-member calls: accumulators, statistics, norms and state_dict()."""
    torch = torch_cuda
    P = ac.group_slice() + 1
    shape = (P, 2, 32, 4, 2, list(range(P)))
    batch, mk = _case(shape)
    grp, seq = mk(32), mk(32)
    src = fs.source(batch, grp.learners[0].actor, own_advantages=True)
    index = _index(torch, P, 32, src['actions'].shape[0], 3)
    rows = [0 if p % 5 == 0 else 1 + (7 * p) % 32 for p in range(P)]
    assert rows[0] == 0 and rows[P - 1] > 0 and max(rows) == 32 and len(set(rows)) > 20
    active = [1 if r else 0 for r in rows]
    clips = [0.0 if p % 3 == 0 else 0.05 * (1 + p % 4) for p in range(P)]
    acc, sums = grp.new_accumulators()
    gb = grp.group_batch(src, index)
    grp.accumulate_grouped(gb, rows, acc, sums)
    grp.accumulate_grouped(gb, [r // 2 for r in rows], acc, sums, offset=0)
    norm = torch.full((P,), -1.0, device='cuda')
    stats = grp.finish_grouped(acc, sums, clips, active, grad_norm=norm)
    grp.apply_grouped(active)
    stats, norm = stats.cpu().numpy(), norm.cpu().numpy()
    for p, ln in enumerate(seq.learners):
        if not rows[p]:
            assert not acc[p].any() and not sums[p].any() and not stats[p].any() and norm[p] == -1.0 and grp.learners[p].state_dict()['step'] == 0
            continue
        a, s = ln.new_accumulators()
        ln.accumulate_indexed(src, index[p, :rows[p]].contiguous(), a, s)
        if rows[p] // 2:
            ln.accumulate_indexed(src, index[p, :rows[p] // 2].contiguous(), a, s)
        n = torch.zeros(1, device='cuda')
        want = ln.finish(a, s, grad_clip=clips[p], grad_norm=n).cpu().numpy()
        ln.apply()
        assert torch.equal(acc[p], a) and torch.equal(sums[p], s), p
        assert np.array_equal(stats[p], want) and norm[p] == float(n), p
        fs.same_state(grp.learners[p].state_dict(), ln.state_dict(), stepped=True)


# ---------------------------------------------------------------------------------------------- 4: update(grouped, micro_rows, grad_clip)
def _spy_norms(torch, learner, log):
    """finish_grouped of a set with the norms asked for (with a clip they are computed anyway: the same launches, the same bits)."""
    orig = learner.finish_grouped

    def finish(acc, sums, grad_clip=None, active=None, stats=None, grad_norm=None, hyper=None):
        norm = torch.full((len(learner.learners),), -1.0, device='cuda')
        log.append((norm, list(active)))
        return orig(acc, sums, grad_clip, active, stats, norm, hyper)
    learner.finish_grouped = finish


@pytest.mark.parametrize('minibatch', [None, 3000], ids=['whole-batch', 'two-rounds'])
@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_grouped_update_with_micro_rows_and_grad_clip_equals_the_sequential_update(torch_cuda, compact, minibatch):
    """4 600 / 2 300 / 2 300 rows per policy on max_rows = 2 048 learners, micro_rows = 2 048: micro-batches of 2 048 + 2 048 + 504 and
    2 048 + 252; with minibatch_rows = 3 000 policy 0 takes two rounds and the others one.  Two iterations.  The clip is the middle of
    the smallest and the largest norm of the first minibatch round, which a probe run with a clip nothing reaches reports: before the
    first step the norms do not depend on the clip, so in that round it bites for one policy and not for another -- asserted from
    the norms the grouped run's own finish calls report."""
    torch = torch_cuda
    batch, mk = _case(ac.UPDATE, compact)
    probe, log0 = mk(CHUNK), []
    _spy_norms(torch, probe, log0)
    probe.update(batch, num_sgd_iter=1, minibatch_rows=minibatch, seed=4, grouped=True, micro_rows=CHUNK, grad_clip=1e30)
    first = log0[0][0].cpu().numpy()
    assert log0[0][1] == [1, 1, 1] and np.all(first > 0) and first.max() > first.min()
    clip = 0.5 * (float(first.min()) + float(first.max()))
    grp, seq, log = mk(CHUNK), mk(CHUNK), []
    _spy_norms(torch, grp, log)
    got = grp.update(batch, num_sgd_iter=2, minibatch_rows=minibatch, seed=4, grouped=True, micro_rows=CHUNK, grad_clip=clip)
    want = seq.update(batch, num_sgd_iter=2, minibatch_rows=minibatch, seed=4, micro_rows=CHUNK, grad_clip=clip)
    fs.same_run(got, want, grp, seq)
    rounds = 1 if minibatch is None else 2
    assert len(log) == 2 * rounds and [a for _, a in log] == ([[1, 1, 1]] if rounds == 1 else [[1, 1, 1], [1, 0, 0]]) * 2
    assert [ln.state_dict()['step'] for ln in grp.learners] == [2 * rounds, 2, 2]
    bites = [float(n[p]) > clip for n, a in log for p in range(3) if a[p]]
    assert np.array_equal(log[0][0].cpu().numpy(), first) and any(bites[:3]) and not all(bites[:3]), (clip, first)
    assert all(float(n[p]) == -1.0 for n, a in log for p in range(3) if not a[p])      # a policy that sits a round out: its entry untouched


# ---------------------------------------------------------------------------------------------- 5: the chunk-aligned guarantee
def test_grouped_micro_batches_equal_the_grouped_update_on_learners_that_hold_the_minibatch(torch_cuda):
    """Without grad_clip: update(grouped=True, micro_rows=2048) on max_rows = 2 048 learners against update(grouped=True) on learners
    whose max_rows holds the minibatch of 3 000, same batch, same seed.  Every micro-batch but a minibatch's last is a whole number
    of chunks, so by include/dcomp_learner_accum.h the gradients -- and with them weights, moments and steps -- are the same BITS.
    The statistics are not the same computation: the accumulated path adds each call's per-tile sums and then the calls, the other
    all tiles at once, both in double; tests/test_learner_accum_gpu.py (1) bounds the float32 means to one ulp of each other, and a
    mean of at most two such minibatches is held to its bar, 2^-22 max(1, |x|).  kl_coeff follows a threshold and is equal."""
    batch, mk = _case(ac.UPDATE)
    micro, whole = mk(CHUNK), mk(3000)
    got = micro.update(batch, num_sgd_iter=2, minibatch_rows=3000, seed=7, grouped=True, micro_rows=CHUNK)
    want = whole.update(batch, num_sgd_iter=2, minibatch_rows=3000, seed=7, grouped=True)
    for p in range(3):
        fs.same_state(micro.learners[p].state_dict(), whole.learners[p].state_dict(), stepped=True)
        assert got[p]['kl_coeff'] == want[p]['kl_coeff']
        for k in want[p]:
            print(f'policy {p} {k}: accumulated {got[p][k]!r} whole {want[p][k]!r}')
            assert abs(got[p][k] - want[p][k]) <= 2.0 ** -22 * max(1.0, abs(want[p][k])), (p, k)
    assert [ln.state_dict()['step'] for ln in micro.learners] == [4, 2, 2]
    with pytest.raises(ValueError, match='max_rows'):                                  # without micro_rows the minibatch must fit the handles
        micro.update(batch, num_sgd_iter=1, minibatch_rows=3000, grouped=True)


# ---------------------------------------------------------------------------------------------- 6: mixing
def test_grouped_sequential_member_and_accumulated_calls_mix(torch_cuda):
    """One round of each in turn on one set -- grouped accumulated update, sequential accumulated update, the group's own calls, a
    member's accumulated update, a plain grouped update -- equals the same sequence on a twin through member calls only."""
    torch = torch_cuda
    from deepcomp_amd.learner import standardize
    U, B, H, E, T, slots = ac.UPDATE
    batch, mk = _case(ac.UPDATE, True)
    one, two = mk(CHUNK), mk(CHUNK)
    rows = one.rows_of(T * E * U)
    kw = dict(num_sgd_iter=1, minibatch_rows=CHUNK, grad_clip=1.0)

    def members(seed, **more):
        return [ln.update(batch, seed=seed + p, rows=rows[p], check_rows=False, **dict(kw, **more)) for p, ln in enumerate(two.learners)]
    assert one.update(batch, seed=1, grouped=True, **kw) == members(1)
    assert one.update(batch, seed=2, grouped=False, micro_rows=CHUNK, **kw) == members(2, micro_rows=CHUNK)
    # the group's own calls: 300 positions of every policy's rows in order, each policy its own clip
    src = fs.source(batch, one.learners[0].actor, own_advantages=True)
    for p in range(3):
        src['advantages'].index_copy_(0, rows[p], standardize(src['advantages'].index_select(0, rows[p])))
    index = torch.stack([rows[p][:300].to(torch.int32) for p in range(3)]).contiguous()
    acc, sums = one.new_accumulators()
    one.accumulate_grouped(one.group_batch(src, index), [300, 200, 0], acc, sums)
    one.finish_grouped(acc, sums, [0.5, 0.0, 0.0], [1, 1, 0])
    one.apply_grouped([1, 1, 0])
    for p, (n, c) in enumerate(((300, 0.5), (200, None))):
        a, s = two.learners[p].new_accumulators()
        two.learners[p].accumulate_indexed(src, index[p, :n].contiguous(), a, s)
        two.learners[p].finish(a, s, grad_clip=c)
        two.learners[p].apply()
    assert one.learners[2].update(batch, seed=9, rows=rows[2], micro_rows=CHUNK, **kw) == two.learners[2].update(batch, seed=9, rows=rows[2], micro_rows=CHUNK, **kw)
    assert one.update(batch, num_sgd_iter=1, minibatch_rows=CHUNK, seed=3, grouped=True) == \
        [ln.update(batch, num_sgd_iter=1, minibatch_rows=CHUNK, seed=3 + p, rows=rows[p], check_rows=False) for p, ln in enumerate(two.learners)]
    for a, b in zip(one.state_dict(), two.state_dict()):
        fs.same_state(a, b, stepped=True)
    assert [s['step'] for s in one.state_dict()] == [3 + 3 + 1 + 3, 2 + 2 + 1 + 2, 2 + 2 + 2 + 2]


# ---------------------------------------------------------------------------------------------- 7: lockstep
def _ranks(torch, shape, R, max_rows=CHUNK, key='lock'):
    """(shards, DataParallelPerUELearner ranks): one batch of R x E envs collected once, rank r's E envs of it; every rank a set of its
    own built from the same seeds."""
    from deepcomp_amd.dp_learner import DataParallelPerUELearner
    U, B, H, E, T, slots = shape
    batch, mk = _case((U, B, H, E * R, T, slots), key=key)
    shards = [fs.shard(batch, r, R, E * R, U, T) for r in range(R)]
    return shards, [DataParallelPerUELearner(mk(max_rows), rank=r, world=R) for r in range(R)]


@pytest.mark.parametrize('R', [2, 3])
def test_lockstep_ranks_stay_identical(torch_cuda, R):
    from deepcomp_amd.dp_learner import run_lockstep
    from deepcomp_amd.learner import STATS
    shards, dps = _ranks(torch_cuda, ac.LOCK, R)
    for it in range(2):
        outs = run_lockstep(dps, shards, num_sgd_iter=2, minibatch_rows=R * 256, seed=10 + it, grad_clip=5.0)
        assert all(o == outs[0] for o in outs) and len(outs[0]) == 2 and all(np.isfinite(o[k]) for o in outs[0] for k in STATS)
        for p in range(2):
            assert len({d.set.learners[p].hyper['kl_coeff'] for d in dps}) == 1 and outs[0][p]['kl_coeff'] == dps[0].set.learners[p].hyper['kl_coeff']
            for d in dps[1:]:
                fs.same_state(d.set.learners[p].state_dict(), dps[0].set.learners[p].state_dict(), stepped=True)
        assert [s['step'] for s in dps[0].set.state_dict()] == [4 * (it + 1)] * 2
        shas = run_lockstep(dps, phases='check_sync')
        assert all(s == shas[0] for s in shas) and len(shas[0]) == 2 and shas[0][0] != shas[0][1] and len(shas[0][0]) == 64
    # check_sync does raise, and names the policy: one rank's policy 1 takes a step of its own
    dps[-1].set.learners[1].apply()
    with pytest.raises(RuntimeError, match='differ for policy 1$'):
        run_lockstep(dps, phases='check_sync')


def test_lockstep_of_one_rank_is_the_grouped_update(torch_cuda):
    from deepcomp_amd.dp_learner import run_lockstep
    shards, (dp,) = _ranks(torch_cuda, ac.LOCK, 1)
    _, mk = _case(ac.LOCK, key='lock')
    ref = mk(CHUNK)
    kw = dict(num_sgd_iter=2, minibatch_rows=256, micro_rows=CHUNK, seed=21, grad_clip=5.0)
    assert run_lockstep([dp], shards, **kw)[0] == ref.update(shards[0], grouped=True, **kw)
    for a, b in zip(dp.set.state_dict(), ref.state_dict()):
        fs.same_state(a, b, stepped=True)
    assert dp.update(shards[0], **kw) == ref.update(shards[0], grouped=True, **kw)       # (no group: update() alone is the same thing)
    for a, b in zip(dp.set.state_dict(), ref.state_dict()):
        fs.same_state(a, b, stepped=True)
    assert [s['step'] for s in ref.state_dict()] == [8, 8]


def test_lockstep_of_two_ranks_is_the_phases_written_out(torch_cuda):
    """R = 2 against member calls: per policy the advantages standardised with the float64 moments of both ranks' rows; policy p on rank
    r permutes with seed + p + P r; per minibatch round every rank accumulates its 128 positions per policy (accumulate_indexed), the
    accumulators are added in rank order, every rank finishes (grad_clip) and applies; kl_coeff by RLlib's rule."""
    torch = torch_cuda
    import math
    from deepcomp_amd import learner as lm
    from deepcomp_amd.dp_learner import run_lockstep
    U, B, H, E, T, slots = ac.LOCK
    R, P, seed, mb, CLIP = 2, 2, 31, 128, 0.01      # (tests/test_learner_accum_gpu.py: at this net and these rows 0.01 clips every step)
    shards, dps = _ranks(torch, ac.LOCK, R)
    outs = run_lockstep(dps, shards, num_sgd_iter=2, minibatch_rows=R * mb, seed=seed, grad_clip=CLIP)
    _, mk = _case(ac.LOCK, key='lock')
    refs = [mk(CHUNK) for _ in range(R)]
    srcs = [fs.source(s, refs[0].learners[0].actor, own_advantages=True) for s in shards]
    rows = refs[0].rows_of(srcs[0]['actions'].shape[0])
    n = int(rows[0].numel())
    assert n == 512 == int(rows[1].numel())
    for p in range(P):
        a = [s['advantages'].index_select(0, rows[p]).double() for s in srcs]         # a rank's moments are its own sums; the ranks' are added in rank order
        s1, s2, cnt = float(a[0].sum()) + float(a[1].sum()), float((a[0] * a[0]).sum()) + float((a[1] * a[1]).sum()), float(a[0].numel()) + float(a[1].numel())
        mean = s1 / cnt
        std = math.sqrt(max(0.0, s2 / cnt - mean * mean))
        for s in srcs:
            s['advantages'].index_copy_(0, rows[p], ((s['advantages'].index_select(0, rows[p]).double() - mean) / max(1e-4, std)).float())
    gens = {(r, p): torch.Generator(device='cuda').manual_seed(seed + p + P * r) for r in range(R) for p in range(P)}
    stats = torch.zeros((P, n // mb, 5), device='cuda')
    norms = []
    for _ in range(2):
        perms = {k: torch.randperm(n, generator=g, device='cuda') for k, g in gens.items()}
        for i, s0 in enumerate(range(0, n, mb)):
            for p in range(P):
                parts = []
                for r in range(R):
                    acc, sums = refs[r].learners[p].new_accumulators()
                    refs[r].learners[p].accumulate_indexed(srcs[r], rows[p].index_select(0, perms[r, p][s0:s0 + mb]).to(torch.int32), acc, sums)
                    parts.append((acc, sums))
                acc, sums = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]      # rank order
                assert float(sums[4]) == R * mb
                for r in range(R):
                    nrm = torch.zeros(1, device='cuda')
                    refs[r].learners[p].finish(acc, sums, grad_clip=CLIP, stats=stats[p, i], grad_norm=nrm)
                    refs[r].learners[p].apply()
                norms.append(float(nrm))
    print(f'norms of the written-out run: min {min(norms):.4e} max {max(norms):.4e} clip {CLIP}')
    assert max(norms) > CLIP                                                           # the clip was exercised
    for p in range(P):
        kl = float(stats[p].mean(0)[3])
        coeff = lm.adapt_kl_coeff(HYPER['kl_coeff'], kl, refs[0].learners[p].kl_target)
        assert outs[0][p]['kl'] == kl and outs[0][p]['kl_coeff'] == coeff and outs[1][p] == outs[0][p]
        for r in range(R):
            fs.same_state(dps[r].set.learners[p].state_dict(), dict(refs[r].learners[p].state_dict(), kl_coeff=coeff))
    assert [s['step'] for s in dps[0].set.state_dict()] == [8, 8]


@pytest.mark.parametrize('shape', [ac.LOCK, ac.LOCK4], ids=['P2', 'P4'])
def test_the_ranks_meet_exactly_twice_per_minibatch_round(torch_cuda, shape):
    """A counting driver over two ranks: behind the shard agreement and the moments (one SUM each, per update) every minibatch round has
    exactly two SUM points whatever P is -- acc [P, flat] and sums [P, 8]."""
    torch = torch_cuda
    from deepcomp_amd.learner import SUM
    P = len(set(shape[5]))
    shards, dps = _ranks(torch, shape, 2, key=('count', P))
    per_policy = shape[3] * shape[4] * shape[5].count(0)
    mb, iters = per_policy // 2, 3
    gens = [d.update_phases(b, num_sgd_iter=iters, minibatch_rows=2 * mb, seed=1, grad_clip=5.0) for d, b in zip(dps, shards)]
    seen, results = [], []
    while not results:
        items = []
        for g in gens:
            try:
                items.append(next(g))
            except StopIteration as stop:
                results.append(stop.value)
        if results:
            assert len(results) == 2 and not items
            break
        (t0, op0), (t1, op1) = items
        assert op0 == op1 == SUM and t0.shape == t1.shape
        seen.append((tuple(t0.shape), t0.dtype))
        total = t0 + t1
        t0.copy_(total)
        t1.copy_(total)
    F = dps[0].set.flat_size
    rounds = iters * (per_policy // mb)
    assert seen[:2] == [((P, 2), torch.float64), ((P, 3), torch.float64)]
    assert seen[2:] == [((P, F), torch.float32), ((P, 8), torch.float64)] * rounds and rounds == 6
    assert results[0] == results[1] and len(results[0]) == P


def test_lockstep_refuses_unequal_shards_before_any_launch(torch_cuda):
    from deepcomp_amd.dp_learner import run_lockstep
    U, B, H, E, T, slots = ac.LOCK
    shards, dps = _ranks(torch_cuda, ac.LOCK, 2)
    batch, _ = _case((U, B, H, 2 * E, T, slots), key='lock')
    keys = list(shards[0])
    lo = {k: batch[k].reshape(T, 2 * E, U, -1)[:, :40].reshape(T, 40 * U, -1).contiguous() for k in keys}
    hi = {k: batch[k].reshape(T, 2 * E, U, -1)[:, 40:].reshape(T, 24 * U, -1).contiguous() for k in keys}
    with pytest.raises(ValueError, match='different numbers of rows of policy 0'):
        run_lockstep(dps, [lo, hi], num_sgd_iter=1)
    with pytest.raises(ValueError, match='world size'):
        run_lockstep(dps, shards, num_sgd_iter=1, minibatch_rows=257)
    for d in dps:                                                                      # nothing ran: no step, no group was even built
        assert [s['step'] for s in d.set.state_dict()] == [0, 0] and d.set._group is None


# ---------------------------------------------------------------------------------------------- 8: two real ranks
def test_two_gloo_ranks_equal_lockstep(torch_cuda):
    """tools/dp_train.py --per-ue --world 2 --backend gloo --same-device (the ranks are fresh child processes): 32 envs x 4 UEs x 8
    steps per rank, one policy per UE, one SGD iteration, a clip.  Both ranks report the same sha256 over their policies' master
    weights, and it is the one --lockstep 2 reports with the same seeds: a sum of two f32 terms does not depend on the order."""
    tool = [sys.executable, os.path.join(REPO, 'tools', 'dp_train.py'), '--per-ue', '--envs', '32', '--ues', '4', '--bs', '5', '--steps', '8', '--hidden', '32',
            '--sgd-iters', '1', '--minibatch', '256', '--grad-clip', '0.5', '--seed', '5', '--timeout', '150']

    def run(extra):
        r = subprocess.run(tool + extra, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=170)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
        assert len(lines) == 1, r.stdout
        return json.loads(lines[0])
    ranks = run(['--world', '2', '--backend', 'gloo', '--same-device'])
    assert ranks['mode'] == 'ranks' and ranks['world'] == 2
    assert len(ranks['sha256']) == 2 and ranks['sha256'][0] == ranks['sha256'][1] and ranks['in_sync']
    lock = run(['--lockstep', '2'])
    assert lock['mode'] == 'lockstep' and lock['sha256'] == ranks['sha256']
    assert lock['stats'] == ranks['stats'] and len(ranks['stats']) == 4 and all(np.isfinite(s['total_loss']) for s in ranks['stats'])
