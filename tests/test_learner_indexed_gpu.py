"""GPU tests of the learner's indexed minibatches (include/dcomp_learner_indexed.h; PPOLearner.grads_indexed / evaluate_indexed / update).

The specification is "the existing call on the gathered rows": the indexed call and learner.grads / learner.evaluate on the minibatch
gathered with torch.index_select (the rows of a compact source built with FragmentCodec.unpack) stage the same values at the same
positions, so every comparison here is EXACT -- the five statistics, all twelve gradient arrays, every per-row output, bit for bit.
The learner under test runs weights perturbed against the ones the batch was collected with, so ratios differ from 1 and the KL from 0.

(1) rows, multi: a shuffled index, one of two tiles and a partial one, no index, repeated entries; (2) the compact record with one
connection word; (3) two connection words and two staging chunks of layer 1, rows and compact; (4) several weight-gradient chunks;
(5) central with unlisted heads, and the compact record refused there; (6) upstream gradients through an index; (7) index entries
outside the sample batch are not read; (8) nothing is written past the minibatch; (9)-(11) update: a compact batch (through the row
index) and the rows unpacked from it agree, a gathered loop written out here ends in the same state, also with num_active below the
env's slots; (12) the refusals that read the handle."""
import ctypes

import numpy as np
import pytest

from tests import fcnet_cases as fc
from tests import fcnet_support as fs
from tests.fcnet_support import OUTS, torch_cuda  # noqa: F401  (torch_cuda: the fixture)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- (1), (2) rows and compact, multi
@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_multi_indexed_equals_gathered(torch_cuda, compact):
    """U 5, B 4, hidden 64, tanh, 1 600 source rows of a collect() batch with T = 5: the index crosses time steps and envs."""
    torch = torch_cuda
    from deepcomp_amd.learner import ARRAYS
    kind, E, U, B, H, T = 'multi', 64, 5, 4, 64, 5
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, compact)
    learner = fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=E * U * T)
    src = fs.source(batch, learner.actor)
    n_src = E * U * T
    assert ('obs_compact' in src) == compact and src['actions'].shape[0] == n_src == 1600
    shuffled = fs.shuffled(torch, n_src, 512, 1)
    assert int(shuffled.max()) - int(shuffled.min()) > 4 * E * U                  # (more than four time steps apart)
    stats, grads, _ = fs.check_against_gathered(torch, learner, src, shuffled)
    fs.check_against_gathered(torch, learner, src, fs.shuffled(torch, n_src, 70, 2))    # two tiles and a partial one
    repeated = torch.cat([shuffled[:100], shuffled[:60], shuffled[50:90]]).contiguous()
    fs.check_against_gathered(torch, learner, src, repeated)
    # no index: every source row in order -- the gathered call is then learner.grads on the source itself
    full_stats, full, _ = fs.check_against_gathered(torch, learner, src, None)
    direct = learner.grads(**fs.as_rows(src, learner.actor))
    assert torch.equal(full_stats, direct)
    got = learner.read('grads')
    assert all(np.array_equal(got[n], full[n]) for n in ARRAYS)
    # and the index does select: the first 512 source rows give other numbers than the shuffled 512
    head = torch.arange(512, device='cuda', dtype=torch.int32)
    assert not torch.equal(learner.grads_indexed(src, head), stats)


# ---------------------------------------------------------------------------------------------- (3) two connection words, two chunks
@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_two_connection_words_and_two_staging_chunks(torch_cuda, compact):
    """U 3, B 40, hidden 32, relu, E 16, T 2: a record with two connection words per UE (the generic env kernel writes it), and
    4B + 1 = 161 inputs > the 144 staged at a time, so the value sweep fetches its rows again instead of reusing LDS."""
    torch = torch_cuda
    kind, E, U, B, H, T = 'multi', 16, 3, 40, 32, 2
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'relu', T, compact)
    learner = fs.ppo_learner(kind, U, B, w, vw, 'relu', max_rows=E * U * T)
    assert learner.actor.num_in == 161 > 144
    src = fs.source(batch, learner.actor)
    if compact:
        assert src['obs_compact'].shape[1] == U * (B + 3) + 2 * B
    fs.check_against_gathered(torch, learner, src, fs.shuffled(torch, E * U * T, 70, 3))
    fs.check_against_gathered(torch, learner, src, None)


# ---------------------------------------------------------------------------------------------- (4) several weight-gradient chunks
@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_several_weight_gradient_chunks(torch_cuda, compact):
    """6 400 of 8 000 source rows at hidden 96 (packed as 128): three weight-gradient chunks and a partial one."""
    torch = torch_cuda
    kind, E, U, B, H, T = 'multi', 160, 5, 4, 96, 10
    assert 3 * fc.CHUNK < 6400 < 4 * fc.CHUNK and E * U * T == 8000
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, compact)
    learner = fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=6400)
    fs.check_against_gathered(torch, learner, fs.source(batch, learner.actor), fs.shuffled(torch, 8000, 6400, 4))


# ---------------------------------------------------------------------------------------------- (5) central
def test_central_indexed_equals_gathered_and_refuses_the_compact_record(torch_cuda):
    torch = torch_cuda
    from deepcomp_amd import _lib
    kind, E, U, B, H, T = 'central', 100, 4, 3, 64, 3
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, False)
    learner = fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=E * T)
    src = fs.source(batch, learner.actor)
    idx = fs.shuffled(torch, E * T, 200, 5)
    stats3, _, _ = fs.check_against_gathered(torch, learner, src, idx, num_active=3)
    stats4, _, _ = fs.check_against_gathered(torch, learner, src, idx)
    assert not torch.equal(stats3, stats4)                                         # (the fourth head does count)
    words = torch.zeros((E * T, 64), dtype=torch.int32, device='cuda')
    compact = dict(src, obs_compact=words)
    del compact['obs']
    with pytest.raises(NotImplementedError):
        learner.grads_indexed(compact, idx)
    with pytest.raises(NotImplementedError):
        learner.evaluate_indexed(compact, idx)
    # the library's own refusal of the same call
    L = _lib.load()
    ptrs = [src[k].data_ptr() for k in ('actions', 'old_logp', 'old_logits', 'advantages', 'value_targets', 'old_vf')]
    b = _lib.DcompSgdBatch(ctypes.sizeof(_lib.DcompSgdBatch), _lib.ACTOR_COMPACT, 200, E * T, idx.data_ptr(), U, 0, words.data_ptr(), *ptrs, *([None] * 7))
    hy = learner._hyper_struct()
    st = torch.zeros(5, device='cuda')
    assert L.dcomp_sgd_grads(learner._h, ctypes.byref(b), ctypes.byref(hy), ctypes.c_void_p(st.data_ptr()), None) == _lib.EUNSUPPORTED
    assert b'multi-agent' in L.dcomp_last_error()
    b.logp = st.data_ptr()
    assert L.dcomp_sgd_evaluate(learner._h, ctypes.byref(b), None) == _lib.EUNSUPPORTED


# ---------------------------------------------------------------------------------------------- (6) upstream gradients
def test_upstream_gradients_through_an_index(torch_cuda):
    """dlogits / dvalue in the SOURCE, on the integer data of the exact-gradient test: the indexed call equals the gathered call,
    and the gathered call equals the float64 reference of the gathered rows exactly."""
    torch = torch_cuda
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.learner import PPOLearner, ARRAYS
    kind, E, U, B, H = 'multi', 40, 7, 3, 32
    w, v, x, dl, dv, _ = fc.learner_int_case(kind, E, U, B, H, seed=1)
    learner = PPOLearner(FcnetActor(kind, U, B, w, activation='relu', value_weights=v), max_rows=150)
    src = {'obs': fs.cuda(torch, x), 'dlogits': fs.cuda(torch, dl), 'dvalue': fs.cuda(torch, dv)}
    idx = fs.shuffled(torch, E * U, 150, 6)
    stats, got, _ = fs.check_against_gathered(torch, learner, src, idx)
    assert np.array_equal(stats.cpu().numpy(), np.zeros(5, dtype=np.float32))
    pick = idx.cpu().numpy()
    x64, dl64 = x[pick].astype(np.float64), dl[pick].astype(np.float64)
    h1 = np.maximum(x64 @ w['w1'] + w['b1'], 0)
    h2 = np.maximum(h1 @ w['w2'] + w['b2'], 0)
    assert np.array_equal(got['w3'], (h2.T @ dl64).astype(np.float32)) and np.array_equal(got['b3'], dl64.sum(0).astype(np.float32))
    assert all(np.isfinite(got[n]).all() for n in ARRAYS)


# ---------------------------------------------------------------------------------------------- (7), (8) bad entries, guard band
@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_index_entries_outside_the_batch_are_not_read(torch_cuda, compact):
    """An index of 70 with -1 at position 3 and source_rows at position 40: those positions' outputs are 0, every other position's
    outputs are those of the same call with valid entries there, statistics and gradients are finite.  A guard test: the kernel
    compares the entry with [0, source_rows) before it forms an address."""
    torch = torch_cuda
    from deepcomp_amd.learner import ARRAYS
    kind, E, U, B, H, T = 'multi', 64, 5, 4, 64, 5
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, compact)
    learner = fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=70)
    src = fs.source(batch, learner.actor)
    n_src = E * U * T
    valid = fs.shuffled(torch, n_src, 70, 7)
    bad = valid.clone()
    bad[3], bad[40] = -1, n_src
    want, got = fs.outputs(torch, 70, 1), fs.outputs(torch, 70, 1)
    learner.grads_indexed(src, valid, **want)
    stats = learner.grads_indexed(src, bad, **got)
    grads = learner.read('grads')
    assert bool(torch.isfinite(stats).all()) and all(np.isfinite(grads[n]).all() for n in ARRAYS)
    others = torch.ones(70, dtype=torch.bool, device='cuda')
    others[3] = others[40] = False
    for k in OUTS:
        assert bool((got[k][~others] == 0).all()), k
        assert torch.equal(fs.tbits(torch, got[k][others]), fs.tbits(torch, want[k][others])), k
        assert bool(torch.isfinite(want[k]).all()), k
    e = learner.evaluate_indexed(src, bad)
    e_valid = learner.evaluate_indexed(src, valid)
    for x, y in zip(e, e_valid):
        assert bool((x[~others] == 0).all()) and torch.equal(fs.tbits(torch, x[others]), fs.tbits(torch, y[others]))


def test_nothing_is_written_past_the_minibatch(torch_cuda):
    """Per-row outputs with a guard of 64 sentinel elements behind the 70 positions (two tiles and a partial one)."""
    torch = torch_cuda
    kind, E, U, B, H, T = 'multi', 64, 5, 4, 64, 5
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, True)
    learner = fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=70 + 64)
    src = fs.source(batch, learner.actor)
    idx = fs.shuffled(torch, E * U * T, 70, 8)
    bufs = fs.outputs(torch, 70, 1, pad=64)
    learner.grads_indexed(src, idx, **{k: b[:70] for k, b in bufs.items()})
    for k, b in bufs.items():
        assert bool(torch.isnan(b[70:]).all()), k
        assert bool(torch.isfinite(b[:70]).all()), k
    bufs = fs.outputs(torch, 70, 1, pad=64)
    learner.evaluate_indexed(src, idx)                                             # (allocates its own outputs)
    b = learner._sgd_batch(learner._sgd_source(src, idx), src, idx, None, ('actions',), {k: (bufs[k][:70], 1) for k in ('logp', 'entropy', 'vf')})
    from deepcomp_amd import _lib
    _lib.check(learner._L.dcomp_sgd_evaluate(learner._h, ctypes.byref(b), learner.actor._stream()))
    for k in ('logp', 'entropy', 'vf'):
        assert bool(torch.isnan(bufs[k][70:]).all()) and bool(torch.isfinite(bufs[k][:70]).all()), k


# ---------------------------------------------------------------------------------------------- (9)-(11) update
def test_update_agrees_on_rows_and_compact_and_with_the_gathered_loop(torch_cuda):
    """(9) one compact batch and the rows batch unpacked from it, two learners on twin actors: bit-identical state.  (10) a third
    twin through the gathered loop written out above: the same state again."""
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    kind, E, U, B, H, T = 'multi', 64, 5, 4, 64, 5
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, True)
    rows = fs.rows_batch(batch, U, B)
    assert 'obs' not in batch and rows['obs'].shape == (T, E, U, 4 * B + 1)
    learners = [fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=512, perturb=False, lr=1e-3) for _ in range(3)]
    out_c = learners[0].update(batch, num_sgd_iter=2, minibatch_rows=512, seed=3)
    out_r = learners[1].update(rows, num_sgd_iter=2, minibatch_rows=512, seed=3)
    assert out_c == out_r and all(np.isfinite(out_c[n]) for n in lm.STATS)
    s_c, s_r = learners[0].state_dict(), learners[1].state_dict()
    assert s_c['step'] == 8                                                        # 1 600 rows: three full minibatches and a partial one, twice
    fs.same_state(s_c, s_r)
    assert np.abs(s_c['weights']['w2'] - w['w2']).max() > 1e-4
    fs.gathered_update(torch, learners[2], rows, 2, 512, 3)
    s_g = dict(learners[2].state_dict(), kl_coeff=s_r['kl_coeff'])                 # (the loop leaves kl_coeff alone)
    fs.same_state(s_r, s_g)


@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_update_with_unlisted_slots_equals_the_gathered_loop_over_the_kept_rows(torch_cuda, compact):
    torch = torch_cuda
    kind, E, U, B, H, T = 'multi', 64, 5, 4, 64, 5
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, True)
    rows = fs.rows_batch(batch, U, B)
    a, b = (fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=512, perturb=False, lr=1e-3) for _ in range(2))
    a.update(batch if compact else rows, num_sgd_iter=2, minibatch_rows=512, seed=9, num_active=3)
    fs.gathered_update(torch, b, rows, 2, 512, 9, num_active=3)
    s_a = a.state_dict()
    assert s_a['step'] == 4                                                        # 960 kept rows: one full minibatch and a partial one, twice
    fs.same_state(s_a, dict(b.state_dict(), kl_coeff=s_a['kl_coeff']))
    full = fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=512, perturb=False, lr=1e-3)
    full.update(rows, num_sgd_iter=2, minibatch_rows=512, seed=9)
    assert not np.array_equal(full.state_dict()['weights']['w1'], s_a['weights']['w1'])      # (the unlisted rows are left out)


# ---------------------------------------------------------------------------------------------- (12) refusals that read the handle
def test_refusals_that_need_a_handle(torch_cuda):
    torch = torch_cuda
    from deepcomp_amd import _lib
    kind, E, U, B, H, T = 'multi', 64, 5, 4, 64, 5
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, True)
    learner = fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=64)
    src = fs.source(batch, learner.actor)
    rows_src = fs.as_rows(src, learner.actor)
    n_src = E * U * T
    idx = fs.shuffled(torch, n_src, 70, 1)
    with pytest.raises(ValueError):
        learner.grads_indexed(src, idx)                                            # 70 rows > max_rows 64
    with pytest.raises(ValueError):
        learner.grads_indexed(src, idx[:64].long())                                # the index is int32
    with pytest.raises(ValueError):
        learner.grads_indexed(src, idx[:64].cpu())
    with pytest.raises(ValueError):
        learner.grads_indexed(dict(src, obs=rows_src['obs']), idx[:64])            # rows and record at once
    with pytest.raises(ValueError):
        learner.grads_indexed(dict(src, advantages=src['advantages'][:-1].contiguous()), idx[:64])
    with pytest.raises(ValueError):
        learner.grads_indexed(src, idx[:64], num_active=3)                         # multi: through the index instead
    L = _lib.load()
    st = torch.zeros(5, device='cuda')
    hy = learner._hyper_struct()

    def call(fmt, rows, source_rows, num_active, obs):
        ptrs = [src[k].data_ptr() for k in ('actions', 'old_logp', 'old_logits', 'advantages', 'value_targets', 'old_vf')]
        b = _lib.DcompSgdBatch(ctypes.sizeof(_lib.DcompSgdBatch), fmt, rows, source_rows, idx.data_ptr(), num_active, 0, obs.data_ptr(), *ptrs, *([None] * 7))
        return L.dcomp_sgd_grads(learner._h, ctypes.byref(b), ctypes.byref(hy), ctypes.c_void_p(st.data_ptr()), None)
    assert call(_lib.ACTOR_ROWS, 70, n_src, U, rows_src['obs']) == _lib.EINVAL and b'max_rows' in L.dcomp_last_error()
    assert call(_lib.ACTOR_COMPACT, 64, n_src - 1, U, src['obs_compact']) == _lib.EINVAL and b'multiple of num_ue' in L.dcomp_last_error()
    assert call(_lib.ACTOR_ROWS, 64, n_src, U + 1, rows_src['obs']) == _lib.EINVAL and b'num_active' in L.dcomp_last_error()
    for fmt, obs in ((_lib.ACTOR_ROWS, rows_src['obs']), (_lib.ACTOR_COMPACT, src['obs_compact'])):
        assert call(fmt, 64, n_src, 3, obs) == _lib.EINVAL and b'through the index' in L.dcomp_last_error()
        assert call(fmt, 64, n_src, U, obs) == _lib.OK
    torch.cuda.synchronize()
