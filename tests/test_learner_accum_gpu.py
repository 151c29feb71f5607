"""GPU tests of the accumulated and data-parallel gradients (include/dcomp_learner_accum.h; PPOLearner.accumulate / accumulate_indexed /
finish / update(micro_rows, grad_clip); deepcomp_amd.dp_learner; tools/dp_train.py).

The identity claimed: when every accumulate call but the last has a multiple of the whole batch's chunk_rows, and the whole batch has
mult == 1 (at most 262 144 rows, chunk_rows = 2 048), finish() leaves the gradients dcomp_learner_grads computes on the whole batch,
BIT FOR BIT -- the f32 chunk partials are the same numbers and they are added in the same order, the running sum merely lives in the
caller's buffer between calls.  Beyond 262 144 rows the two differ by f32 re-association only and no identity is claimed.  The same
holds across ranks: R learners that each accumulate one chunk and have their sums added in rank order hold what one learner computes
on the R chunks in a row.

(1) micro-batches equal the whole; a split that is not chunk-aligned is held to ppo_loss_reference at the whole batch's bars;
(2) ranks equal the whole; (3) nothing else is written; (4) clipping; (5) update(micro_rows) against update(); (6) run_lockstep;
(7) two real ranks through tools/dp_train.py.  Shapes: multi U 4, B 5, hidden 32, and central U 10, B 5, hidden 64 (fcnet_cases'
EPILOGUE_SHAPES)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fcnet_cases as fc
from tests import fcnet_support as fs

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTI, CENTRAL, ROWS, CHUNK, LOCK = fc.ACCUM_MULTI, fc.ACCUM_CENTRAL, fc.ACCUM_ROWS, fc.CHUNK, fc.ACCUM_LOCK
ALIGNED = [(2048, 2048, 2348), (4096, 2348)]
UNALIGNED = (1000, 5444)


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert fc.CHUNK_UNIT == CHUNK and fc.row_split(ROWS) == dict(mult=1, chunk_rows=CHUNK, nchunks=4)
    return torch


def _twin(shape, c, max_rows, **kw):
    kind, E, U, B, H, T = shape
    return fs.ppo_learner(kind, U, B, c['w'], c['vw'], 'tanh', max_rows=max_rows, **kw)


def _split(sizes):
    assert sum(sizes) == ROWS
    lo = 0
    for n in sizes:
        yield lo, lo + n
        lo += n


def _accumulate(learner, c, sizes, surface):
    """One minibatch of ROWS positions in micro-batches of `sizes` through a surface; returns (acc, sums)."""
    acc, sums = learner.new_accumulators()
    for lo, hi in _split(sizes):
        if surface == 'rows':
            learner.accumulate(**{k: t[lo:hi] for k, t in c['gathered'].items()}, acc=acc, sums=sums)
        else:
            learner.accumulate_indexed(c['src'], c['index'][lo:hi], acc, sums)
    return acc, sums


# ---------------------------------------------------------------------------------------------- (1) micro-batches equal the whole
@pytest.mark.parametrize('case', ['multi-rows', 'multi-indexed', 'multi-compact', 'central-rows', 'central-indexed'])
def test_micro_batches_equal_the_whole_bit_for_bit(torch_cuda, case):
    """Condition (see the header): every call but the last is a multiple of the whole batch's chunk_rows = 2 048 and the whole has
    mult == 1.  The gradients then are those of grads() on the 6 444 rows, array_equal.

    The statistics: the four loss sums are doubles.  grads() adds the 202 per-tile sums of the batch in 256 fixed ranges and then the
    ranges in order; the accumulated path adds each call's tiles the same way and then the calls.  Both are re-associations of the same
    202 doubles (the per-tile sums themselves are identical: a tile's rows are the same in both), so each sum is off from the exact
    one by at most (202 - 1) x 2^-53 x sum |tile sums| <= 2^-45.3 x sum over rows |term|, the two differ by at most twice that, and after
    the 1 / N the means differ by less than 2^-44 x mean |term| -- 2^-40 is the bar.  The conversion to float32 can then fall to
    either side: one float32 ulp of the whole-batch value.  total_loss is formed from the four float32 means and is held to the same
    form with the per-row term of the total."""
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    shape = MULTI if case.startswith('multi') else CENTRAL
    surface = case.split('-')[1]
    c = fs.now(fs.whole(torch, shape, compact=surface == 'compact'))
    rows_c = fs.now(fs.whole(torch, shape))                      # (the per-row terms: from the rows of the same index)
    _, terms = fs.row_terms(rows_c, shape)
    micro = _twin(shape, c, 4096)
    assert micro.flat_size == fs.flat(c['grads']).size
    for sizes in ALIGNED:
        assert all(n % CHUNK == 0 for n in sizes[:-1])
        acc, sums = _accumulate(micro, c, sizes, 'rows' if surface == 'rows' else 'indexed')
        stats = micro.finish(acc, sums).cpu().numpy()
        got = micro.read('grads')
        for n in lm.ARRAYS:
            assert np.array_equal(got[n], c['grads'][n]), (sizes, n, np.abs(got[n] - c['grads'][n]).max())
        assert float(sums[4]) == ROWS and not sums[5:].any()
        for i, n in enumerate(lm.STATS):
            bar = float(np.spacing(np.abs(c['stats'][i]))) + 2.0 ** -40 * terms[n]
            print(f'accumulated {case} {sizes} {n}: {stats[i]!r} whole {c["stats"][i]!r} |diff| {abs(float(stats[i]) - float(c["stats"][i])):.3e} bar {bar:.3e}')
            assert abs(float(stats[i]) - float(c['stats'][i])) <= bar, (sizes, n)
    assert any(np.abs(c['grads'][n]).max() > 0 for n in ('w1', 'vw1'))


@pytest.mark.parametrize('shape', [MULTI, CENTRAL], ids=['multi', 'central'])
def test_a_split_that_is_not_chunk_aligned_meets_the_whole_batch_bars(torch_cuda, shape):
    """1 000 + 5 444 rows: the first call ends inside a chunk, so the sums over rows are re-associated and no identity is claimed; the
    gradients are held to the float64 model at test_learner_gpu's bar for a whole batch (2 x the CPU bf16 chain's own error, per
    array).  The statistics are not re-associated by the split beyond test (1)'s bound and are held to the whole batch's."""
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    c = fs.now(fs.whole(torch, shape))
    ref64, _ = fs.row_terms(c, shape)
    host = {k: t.cpu().numpy() for k, t in c['gathered'].items()}
    chain = lm.ppo_loss_reference(c['w_now'], c['vw_now'], host, fc.HYPER, 'tanh', 'bf16')
    learner = _twin(shape, c, ROWS)
    assert UNALIGNED[0] % CHUNK
    acc, sums = _accumulate(learner, c, UNALIGNED, 'rows')
    stats = learner.finish(acc, sums).cpu().numpy()
    got = learner.read('grads')
    worst = []
    for name, ek, ec in fs.errors(lm, stats, got, ref64, chain):
        print(f'unaligned split {shape[0]} {name}: CPU chain max abs err {ec:.3e}  kernel {ek:.3e}')
        if name in lm.ARRAYS and not ek <= 2 * ec:           # the gradients: what the split re-associates
            worst.append((name, ek, ec))
    assert not worst, worst
    # the whole batch's gradients are inside the same bars, and the split did change bits: neither comparison is vacuous
    assert all(ek <= 2 * ec for name, ek, ec in fs.errors(lm, c['stats'], c['grads'], ref64, chain) if name in lm.ARRAYS)
    assert any(not np.array_equal(got[n], c['grads'][n]) for n in lm.ARRAYS)
    # the statistics do not depend on where a call ends: test (1)'s bar against the whole batch
    _, terms = fs.row_terms(c, shape)
    for i, n in enumerate(lm.STATS):
        assert abs(float(stats[i]) - float(c['stats'][i])) <= float(np.spacing(np.abs(c['stats'][i]))) + 2.0 ** -40 * terms[n], n


# ---------------------------------------------------------------------------------------------- (2) ranks equal the whole
def _probe(torch, learner, obs):
    """What the actor's packed weights compute on obs, and the learner's masters and moments."""
    a = learner.actor
    rows = obs.shape[0]
    logits, logp = torch.full((rows, a.num_logits), float('nan'), device='cuda'), torch.full((rows, a.heads), float('nan'), device='cuda')
    vf = torch.full((rows,), float('nan'), device='cuda')
    act = a.actions(obs, sample=True, seed=5, step=2, logits=logits, logp=logp, vf=vf)
    return (act, logits, logp, vf), learner.state_dict()


def _same(torch, lm, p1, p2):
    for x, y in zip(p1[0], p2[0]):
        assert torch.equal(x, y)
    assert bool(torch.isfinite(p1[0][1]).all())
    fs.same_state(p1[1], p2[1])


@pytest.mark.parametrize('R', [2, 3])
def test_ranks_equal_the_whole_bit_for_bit(torch_cuda, R):
    """R learners with equal weights accumulate 2 048 rows each; acc and sums are added in rank order with torch and written back;
    finish + apply on every rank.  All ranks hold the same master weights, moments and packed actor weights (probed through the actor
    and through the next gradients, which read the backward fragments), and they are those of one learner after grads + apply on
    the R x 2 048 rows in a row."""
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    c = fs.whole(torch, MULTI)
    n = R * CHUNK
    rows = {k: t[:n] for k, t in c['gathered'].items()}
    one = _twin(MULTI, c, n, lr=1e-3)
    one.grads(**rows)
    one.apply()
    ranks = [_twin(MULTI, c, CHUNK, lr=1e-3) for _ in range(R)]
    accs = []
    for r, ln in enumerate(ranks):
        acc, sums = ln.new_accumulators()
        ln.accumulate(**{k: t[r * CHUNK:(r + 1) * CHUNK] for k, t in rows.items()}, acc=acc, sums=sums)
        accs.append((acc, sums))
    acc_sum, sums_sum = accs[0][0].clone(), accs[0][1].clone()
    for acc, sums in accs[1:]:                               # rank order
        acc_sum += acc
        sums_sum += sums
    assert float(sums_sum[4]) == n
    for ln, (acc, sums) in zip(ranks, accs):
        acc.copy_(acc_sum)
        sums.copy_(sums_sum)
        ln.finish(acc, sums)
        ln.apply()
    obs = rows['obs'][:300]
    want = _probe(torch, one, obs)
    assert want[1]['step'] == 1 and np.abs(want[1]['weights']['w2'] - lm.join_weights(*fs.perturbed(c['w'], c['vw']))['w2']).max() > 1e-4
    for ln in ranks:
        _same(torch, lm, _probe(torch, ln, obs), want)
    # the backward fragments: the next gradients, on rows none of the ranks has seen
    nxt = {k: t[n:n + 300] for k, t in c['gathered'].items()} if n + 300 <= ROWS else {k: t[:300] for k, t in c['gathered'].items()}
    g_want = (one.grads(**nxt).cpu().numpy(), one.read('grads'))
    for ln in ranks:
        s = ln.grads(**nxt).cpu().numpy()
        g = ln.read('grads')
        assert np.array_equal(s, g_want[0])
        for name in lm.ARRAYS:
            assert np.array_equal(g[name], g_want[1][name]), name


# ---------------------------------------------------------------------------------------------- (3) nothing else is written
def test_nothing_else_is_written_and_repeats_are_identical(torch_cuda):
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    c = fs.whole(torch, MULTI)
    learner = _twin(MULTI, c, ROWS)
    F = learner.flat_size
    first = {k: t[:700] for k, t in c['gathered'].items()}
    kept_stats = learner.grads(**first)
    kept_stats_bits, kept = kept_stats.clone(), learner.read('grads')
    runs = []
    for _ in range(2):
        # guard words on both sides of acc and sums
        abuf = torch.full((F + 128,), float('nan'), device='cuda')
        sbuf = torch.full((8 + 16,), float('nan'), dtype=torch.float64, device='cuda')
        acc, sums = abuf[64:64 + F], sbuf[8:16]
        acc.zero_()
        sums.zero_()
        for lo, hi in _split(ALIGNED[0]):
            learner.accumulate(**{k: t[lo:hi] for k, t in c['gathered'].items()}, acc=acc, sums=sums)
        # accumulate has left the handle's gradients and the caller's statistics alone
        after = learner.read('grads')
        for n in lm.ARRAYS:
            assert np.array_equal(after[n], kept[n]), n
        assert torch.equal(kept_stats, kept_stats_bits)
        assert bool(torch.isnan(abuf[:64]).all()) and bool(torch.isnan(abuf[64 + F:]).all())
        assert bool(torch.isnan(sbuf[:8]).all()) and bool(torch.isnan(sbuf[16:]).all())
        assert bool(torch.isfinite(acc).all()) and float(sums[4]) == ROWS and not sums[5:].any()
        acc0, sums0 = acc.clone(), sums.clone()
        norm = torch.full((3,), float('nan'), device='cuda')
        stats = learner.finish(acc, sums, grad_clip=1e-3, grad_norm=norm[1:2])
        got = learner.read('grads')
        # finish has left acc and sums alone, and everything around them
        assert torch.equal(acc, acc0) and torch.equal(sums, sums0)
        assert bool(torch.isnan(abuf[:64]).all()) and bool(torch.isnan(abuf[64 + F:]).all())
        assert bool(torch.isnan(sbuf[:8]).all()) and bool(torch.isnan(sbuf[16:]).all())
        assert bool(torch.isnan(norm[0])) and bool(torch.isnan(norm[2])) and float(norm[1]) > 1e-3
        again = learner.finish(acc, sums, grad_clip=1e-3)     # (it can be called again)
        assert torch.equal(again, stats)
        for n in lm.ARRAYS:
            assert np.array_equal(learner.read('grads')[n], got[n]), n
        runs.append((acc0.cpu().numpy(), sums0.cpu().numpy(), stats.cpu().numpy(), fs.flat(got), norm.cpu().numpy()[1]))
        learner.grads(**first, stats=kept_stats)             # the handle's gradients as before the next run
    for x, y in zip(*runs):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------- (4) clipping
def test_global_norm_clipping(torch_cuda):
    """clip_reference is the model.  The float64 norm of the read-back unclipped gradient against grad_norm: one float32 ulp.  Every
    clipped entry against float32(g x coef_ref): two float32 ulps -- one for the coefficient's rounding falling either side (the
    kernel's double norm is a different order of the same sum), one for the product.  Below the clip: unchanged bit for bit."""
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    c = fs.whole(torch, MULTI)
    learner = _twin(MULTI, c, 4096)
    acc, sums = _accumulate(learner, c, ALIGNED[1], 'rows')
    learner.finish(acc, sums)
    g = fs.flat(learner.read('grads'))
    assert np.array_equal(g, fs.flat(c['grads']))
    norm64 = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    for clip, clipped in ((0.5 * norm64, True), (2.0 * norm64, False)):
        assert (norm64 > clip) == clipped                    # from the read-back unclipped gradient
        norm = torch.full((1,), float('nan'), device='cuda')
        learner.finish(acc, sums, grad_clip=clip, grad_norm=norm)
        got = fs.flat(learner.read('grads'))
        want, want_norm = lm.clip_reference(g, clip)
        assert learner.clip_reference is lm.clip_reference
        print(f'clip {clip:.6e}: grad_norm {float(norm):.9e} float64 norm {norm64:.9e} |diff| {abs(float(norm) - norm64):.3e} ulp {float(np.spacing(np.float32(norm64))):.3e}')
        assert abs(float(norm) - norm64) <= float(np.spacing(np.float32(norm64)))
        if clipped:
            ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
            print(f'clipped entries: max distance from float32(g x coef_ref) {ulps.max():.2f} ulp')
            assert ulps.max() <= 2.0
            assert np.abs(got).max() < np.abs(g).max() and abs(float(np.sqrt((got.astype(np.float64) ** 2).sum())) - clip) < 1e-5 * clip
        else:
            assert np.array_equal(got, g)
    # grad_clip 0 / None: no clipping, the norm all the same
    for none in (0.0, None):
        norm = torch.full((1,), float('nan'), device='cuda')
        learner.finish(acc, sums, grad_clip=none, grad_norm=norm)
        assert np.array_equal(fs.flat(learner.read('grads')), g)
        assert abs(float(norm) - norm64) <= float(np.spacing(np.float32(norm64)))
    with pytest.raises(ValueError):
        learner.finish(acc, sums, grad_clip=-1.0)
    with pytest.raises(ValueError):
        learner.finish(acc[:-1], sums)


# ---------------------------------------------------------------------------------------------- (5) update(micro_rows)
@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_update_with_micro_rows_equals_update(torch_cuda, compact):
    """6 464 rows in minibatches of 4 096 (one full, one of 2 368), two iterations: update(micro_rows=2048) by a learner whose handle
    holds 2 048 rows leaves the state update() leaves a twin whose handle holds the minibatch, bit for bit; and update() with the
    defaults is still the gathered loop written out from grads + apply (tests/test_learner_indexed_gpu.py)."""
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    kind, E, U, B, H, T = MULTI
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, compact)
    mk = lambda max_rows: fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=max_rows, perturb=False, lr=1e-3)      # noqa: E731
    whole, micro, loop = mk(4096), mk(CHUNK), mk(4096)
    out_w = whole.update(batch, num_sgd_iter=2, minibatch_rows=4096, seed=3)
    out_m = micro.update(batch, num_sgd_iter=2, minibatch_rows=4096, seed=3, micro_rows=CHUNK)
    s_w, s_m = whole.state_dict(), micro.state_dict()
    assert s_w['step'] == 4 and np.abs(s_w['weights']['w2'] - w['w2']).max() > 1e-4
    fs.same_state(s_w, s_m)
    for n in lm.STATS:                                       # means of two minibatches' float32 statistics, each within an ulp (test (1))
        assert abs(out_w[n] - out_m[n]) <= 2.0 ** -22 * max(1.0, abs(out_w[n])), n
    fs.gathered_update(torch, loop, batch if not compact else fs.rows_batch(batch, U, B), 2, 4096, 3)
    fs.same_state(s_w, dict(loop.state_dict(), kl_coeff=s_w['kl_coeff']))
    # the refusals of update's new arguments
    for bad in (1000, CHUNK + 1, 0):
        with pytest.raises(ValueError, match='multiple'):
            micro.update(batch, num_sgd_iter=1, minibatch_rows=4096, micro_rows=bad)
    with pytest.raises(ValueError, match='max_rows'):
        micro.update(batch, num_sgd_iter=1, minibatch_rows=4096, micro_rows=2 * CHUNK)
    with pytest.raises(ValueError, match='max_rows'):
        micro.update(batch, num_sgd_iter=1, minibatch_rows=4096)            # without micro_rows the minibatch must fit the handle
    with pytest.raises(ValueError, match='grad_clip'):
        whole.update(batch, num_sgd_iter=1, minibatch_rows=4096, grad_clip=-0.5)
    assert micro.state_dict()['step'] == 4


def test_update_with_grad_clip_clips(torch_cuda):
    """update(grad_clip) against the loop written out: accumulate, finish(grad_clip), apply -- and the clip does change the step."""
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    kind, E, U, B, H, T = MULTI
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, False)
    mk = lambda: fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=4096, perturb=False, lr=1e-3)      # noqa: E731
    clipped, loop, free = mk(), mk(), mk()
    clipped.update(batch, num_sgd_iter=1, minibatch_rows=4096, seed=3, grad_clip=0.01)
    free.update(batch, num_sgd_iter=1, minibatch_rows=4096, seed=3)
    src = fs.source(batch, loop.actor)
    adv = src['advantages']
    src['advantages'] = (adv - adv.mean()) / adv.std(unbiased=False).clamp_min(1e-4)
    N = src['obs'].shape[0]
    gen = torch.Generator(device='cuda')
    gen.manual_seed(3)
    perm = torch.randperm(N, generator=gen, device='cuda')
    acc, sums = loop.new_accumulators()
    norms = []
    for s in range(0, N, 4096):
        acc.zero_()
        sums.zero_()
        loop.accumulate(**{k: t.index_select(0, perm[s:s + 4096]) for k, t in src.items()}, acc=acc, sums=sums)
        norm = torch.zeros(1, device='cuda')
        loop.finish(acc, sums, grad_clip=0.01, grad_norm=norm)
        norms.append(float(norm))
        loop.apply()
    assert min(norms) > 0.01                                 # every step was clipped
    fs.same_state(clipped.state_dict(), dict(loop.state_dict(), kl_coeff=clipped.hyper['kl_coeff']))
    assert not np.array_equal(clipped.read('m')['w2'], free.read('m')['w2'])


# ---------------------------------------------------------------------------------------------- (6) lockstep
def _dp_ranks(torch, R, w, vw, max_rows):
    from deepcomp_amd.dp_learner import DataParallelLearner
    kind, E, U, B, H, T = LOCK
    return [DataParallelLearner(fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=max_rows, perturb=False, lr=1e-3), rank=r, world=R) for r in range(R)]


@pytest.mark.parametrize('R', [2, 3])
def test_lockstep_ranks_stay_identical(torch_cuda, R):
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    from deepcomp_amd.dp_learner import run_lockstep
    kind, E, U, B, H, T = LOCK
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, False)
    shards = [fs.shard(batch, r, R, E, U, T) for r in range(R)]
    n = E * U * T // R
    dps = _dp_ranks(torch, R, w, vw, max_rows=n // 2)
    obs = shards[0]['obs'].reshape(-1, 4 * B + 1)[:200]
    for it in range(2):
        outs = run_lockstep(dps, shards, num_sgd_iter=2, minibatch_rows=R * (n // 2), seed=10 + it, grad_clip=5.0)
        assert all(o == outs[0] for o in outs) and all(np.isfinite(outs[0][k]) for k in lm.STATS)
        assert len({d.learner.hyper['kl_coeff'] for d in dps}) == 1 and outs[0]['kl_coeff'] == dps[0].learner.hyper['kl_coeff']
        probes = [_probe(torch, d.learner, obs) for d in dps]
        assert probes[0][1]['step'] == 4 * (it + 1)
        for p in probes[1:]:
            _same(torch, lm, p, probes[0])
        shas = run_lockstep(dps, phases='check_sync')
        assert len(set(shas)) == 1 and len(shas[0]) == 64
    assert np.abs(probes[0][1]['weights']['w2'] - w['w2']).max() > 1e-4
    # check_sync does raise: one rank takes a step of its own
    dps[-1].learner.apply()
    with pytest.raises(RuntimeError, match='differ'):
        run_lockstep(dps, phases='check_sync')


def test_lockstep_of_one_rank_is_the_phases_written_out(torch_cuda):
    """R = 1 against the primitives: the stated standardisation (float64 moments, max(0, .), the 1e-4 floor, one rounding), a
    permutation seeded seed + 0, per minibatch zeroed accumulators, accumulate, finish, apply; kl_coeff by RLlib's rule."""
    torch = torch_cuda
    import math
    from deepcomp_amd import learner as lm
    from deepcomp_amd.dp_learner import DataParallelLearner, run_lockstep
    kind, E, U, B, H, T = LOCK
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, False)
    dp = _dp_ranks(torch, 1, w, vw, max_rows=CHUNK)[0]
    out = run_lockstep([dp], [batch], num_sgd_iter=2, minibatch_rows=CHUNK, micro_rows=CHUNK, seed=21)[0]
    assert out == DataParallelLearner(fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=CHUNK, perturb=False, lr=1e-3)).update(
        batch, num_sgd_iter=2, minibatch_rows=CHUNK, micro_rows=CHUNK, seed=21)          # (no group: update() alone is the same thing)
    ref = fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=CHUNK, perturb=False, lr=1e-3)
    src = fs.source(batch, ref.actor)
    a = src['advantages'].double()
    n = a.numel()
    mean = float(a.sum()) / n
    var = max(0.0, float((a * a).sum()) / n - mean * mean)
    src['advantages'] = ((a - mean) / max(1e-4, math.sqrt(var))).float()
    gen = torch.Generator(device='cuda')
    gen.manual_seed(21)
    acc, sums = ref.new_accumulators()
    starts = list(range(0, n, CHUNK))
    stats = torch.zeros((len(starts), 5), device='cuda')
    for _ in range(2):
        perm = torch.randperm(n, generator=gen, device='cuda')
        for i, s in enumerate(starts):
            acc.zero_()
            sums.zero_()
            ref.accumulate(**{k: t.index_select(0, perm[s:s + CHUNK]) for k, t in src.items()}, acc=acc, sums=sums)
            ref.finish(acc, sums, stats=stats[i])
            ref.apply()
    kl = float(stats.mean(0)[3])
    want_coeff = lm.adapt_kl_coeff(fc.HYPER['kl_coeff'], kl, ref.kl_target)
    assert out['kl'] == kl and out['kl_coeff'] == want_coeff
    fs.same_state(dp.learner.state_dict(), dict(ref.state_dict(), kl_coeff=want_coeff))
    assert dp.learner.state_dict()['step'] == 4


def test_lockstep_refuses_unequal_shards_before_any_launch(torch_cuda):
    torch = torch_cuda
    from deepcomp_amd.dp_learner import run_lockstep
    kind, E, U, B, H, T = LOCK
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, False)
    dps = _dp_ranks(torch, 2, w, vw, max_rows=CHUNK)
    before = [d.learner.state_dict() for d in dps]
    lo = {k: batch[k].reshape(T, E, U, -1)[:, :40].reshape(T, 40 * U, -1).contiguous() for k in fs.shard(batch, 0, 2, E, U, T)}
    hi = {k: batch[k].reshape(T, E, U, -1)[:, 40:].reshape(T, 56 * U, -1).contiguous() for k in lo}
    with pytest.raises(ValueError, match='different numbers of rows'):
        run_lockstep(dps, [lo, hi], num_sgd_iter=1)
    with pytest.raises(ValueError, match='world size'):
        run_lockstep(dps, [fs.shard(batch, r, 2, E, U, T) for r in range(2)], num_sgd_iter=1, minibatch_rows=1025)
    from deepcomp_amd import learner as lm
    for d, s in zip(dps, before):                            # nothing ran: no step, the weights as they were
        fs.same_state(d.learner.state_dict(), s)
        assert d.learner.state_dict()['step'] == 0


# ---------------------------------------------------------------------------------------------- (7) two real ranks
def test_two_gloo_ranks_equal_lockstep(torch_cuda):
    """tools/dp_train.py --world 2 --backend gloo --same-device: 64 envs x 4 UEs x 8 steps per rank, one SGD iteration, one minibatch.
    Both ranks report the same sha256 of their master weights, and it is the one --lockstep 2 reports with the same seeds: a sum of
    two f32 terms does not depend on the order, so gloo's all-reduce and the rank-order sum must agree exactly."""
    tool = [sys.executable, os.path.join(REPO, 'tools', 'dp_train.py'), '--envs', '64', '--ues', '4', '--bs', '5', '--steps', '8', '--hidden', '32',
            '--sgd-iters', '1', '--seed', '5', '--timeout', '150']

    def run(extra):
        r = subprocess.run(tool + extra, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=170)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
        assert len(lines) == 1, r.stdout
        return json.loads(lines[0])
    ranks = run(['--world', '2', '--backend', 'gloo', '--same-device'])
    assert ranks['mode'] == 'ranks' and ranks['world'] == 2 and ranks['rows_per_rank'] == 2048
    assert len(ranks['sha256']) == 2 and ranks['sha256'][0] == ranks['sha256'][1] and ranks['in_sync']
    lock = run(['--lockstep', '2'])
    assert lock['mode'] == 'lockstep' and lock['sha256'] == ranks['sha256']
    assert lock['stats'] == ranks['stats'] and np.isfinite(ranks['stats']['total_loss'])
    assert set(ranks['seconds']) >= {'accumulate', 'reduce', 'finish', 'apply'}
