"""GPU tests of the grouped PPO learner (include/dcomp_learner_group.h; PerUELearner.update(grouped=True)).

The reference is the existing sequential path -- PerUELearner.update, P PPOLearner.update calls, and dcomp_sgd_grads -- which other
tests hold to the float64 model.  A policy's arithmetic is unchanged and its row split depends on its own row count alone, so every
comparison here is EXACT: np.array_equal on state_dict() (weights, m, v, step, kl_coeff) and == on the statistics dicts.

Shapes: tests/group_cases.py's GROUP_CASES (tests/test_learner_group_cpu.py shows that they reach every grouped instantiation and every
weight-gradient form).  A sample batch is collected once per case and left unchanged."""
import ctypes

import numpy as np
import pytest

from tests import fcnet_support as fs
from tests import group_cases as cases
from tests.fcnet_cases import HYPER
from tests.fcnet_support import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -6


# ---------------------------------------------------------------------------------------------- 1: the uneven split
@pytest.mark.parametrize('name', cases.UNEVEN)
def test_uneven_split_equals_the_sequential_update(torch_cuda, name):
    """Policy 0 has 700 rows and policy 1 has 1 050: 11 against 17 minibatch rounds (policy 0 sits six out), last minibatches of 60
    and 26 rows, and from the second iteration on the policies' Adam steps differ."""
    batch, grp, seq = fs.twins(name)
    got = grp.update(batch, num_sgd_iter=2, minibatch_rows=64, seed=4, grouped=True)
    want = seq.update(batch, num_sgd_iter=2, minibatch_rows=64, seed=4)
    fs.same_run(got, want, grp, seq)
    assert [ln.state_dict()['step'] for ln in grp.learners] == [22, 34]
    w = [ln.read('weights')['w1'] for ln in grp.learners]
    assert not np.array_equal(w[0], w[1])


# ---------------------------------------------------------------------------------------------- 2: the other cells
@pytest.mark.parametrize('name', [n for n in cases.GROUP_CASES if n not in cases.UNEVEN])
def test_every_other_cell_equals_the_sequential_update(torch_cuda, name):
    batch, grp, seq = fs.twins(name)
    got = grp.update(batch, num_sgd_iter=2, minibatch_rows=64, seed=2, grouped=True)
    want = seq.update(batch, num_sgd_iter=2, minibatch_rows=64, seed=2)
    fs.same_run(got, want, grp, seq)


# ---------------------------------------------------------------------------------------------- 3: weight-gradient chunks per policy
def test_several_weight_gradient_chunks_that_differ_per_policy(torch_cuda):
    """U 3, slots [0, 0, 1], E 450, T 5, minibatch_rows = max_rows = 4 500: policy 0 gets one minibatch of 4 500 rows (3 chunks, the
    last one partial), policy 1 one of 2 250 rows (2 chunks)."""
    U, B, H, act, E, T, slots = 3, 3, 32, 'tanh', 450, 5, [0, 0, 1]
    batch = fs.group_collected('chunks', U, B, H, act, E, T, slots, True)
    grp, seq = fs.per_ue_learner(fs.policy_set(U, B, H, act, slots), 4500), fs.per_ue_learner(fs.policy_set(U, B, H, act, slots), 4500)
    got = grp.update(batch, num_sgd_iter=2, minibatch_rows=4500, seed=1, grouped=True)
    want = seq.update(batch, num_sgd_iter=2, minibatch_rows=4500, seed=1)
    fs.same_run(got, want, grp, seq)
    assert [ln.state_dict()['step'] for ln in grp.learners] == [2, 2]


# ---------------------------------------------------------------------------------------------- 4: more policies than one slice
@pytest.mark.parametrize('skip', [False, True], ids=['every-policy', 'one-without-slots'])
def test_more_policies_than_one_launch_slice(torch_cuda, skip):
    """DCOMP_GROUP_SLICE + 2 policies: two launch rounds per call.  skip: the first policy of the second slice has no slot (its
    neighbour has two): it returns None and its weights, moments and step stay as created."""
    from deepcomp_amd.learner import ARRAYS
    P = cases.group_slice() + 2
    U, B, H, act, E, T = P, 2, 32, 'tanh', 4, 2
    slots = list(range(P))
    if skip:
        slots[P - 2] = P - 1
    batch = fs.group_collected(('slice', skip), U, B, H, act, E, T, slots, False)
    grp, seq = fs.per_ue_learner(fs.policy_set(U, B, H, act, slots), 32), fs.per_ue_learner(fs.policy_set(U, B, H, act, slots), 32)
    if skip:                                                                           # (the members come from max(slots) + 1: all P)
        assert len(grp.learners) == P
        before = grp.learners[P - 2].state_dict()
    got = grp.update(batch, num_sgd_iter=2, minibatch_rows=32, seed=3, grouped=True)
    want = seq.update(batch, num_sgd_iter=2, minibatch_rows=32, seed=3)
    fs.same_run(got, want, grp, seq)
    assert sum(g is None for g in got) == (1 if skip else 0)
    if skip:
        assert got[P - 2] is None
        after = grp.learners[P - 2].state_dict()
        assert after['step'] == 0 == before['step'] and after['kl_coeff'] == before['kl_coeff']
        for k in ('weights', 'm', 'v'):
            for n in ARRAYS:
                assert np.array_equal(after[k][n], before[k][n]), (k, n)
        assert grp.learners[P - 1].state_dict()['step'] == 2 and grp.learners[0].state_dict()['step'] == 2


# ---------------------------------------------------------------------------------------------- 5: the C call directly
@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_group_grads_is_p_sgd_grads_calls(torch_cuda, compact):
    """One dcomp_learner_group_grads against dcomp_sgd_grads per policy on twins: all twelve gradient arrays and the [P][5] statistics.
    Policy 0's index has repeated and out-of-range entries (-1, source_rows); policy 2 sits the call out and keeps its gradients and
    its statistics row; a guard band behind stats_dev stays; a second identical call gives identical bits."""
    torch = torch_cuda
    from deepcomp_amd import _lib
    from deepcomp_amd.learner import ARRAYS, PPOLearner
    U, B, H, act, E, T, slots, _ = cases.GROUP_CASES['a-compact' if compact else 'a-rows']
    batch = fs.group_collected('a-compact' if compact else 'a-rows', U, B, H, act, E, T, slots, compact)
    mk = lambda: [PPOLearner(m, max_rows=128, **dict(HYPER, lr=1e-3, kl_coeff=0.2 + 0.1 * p)) for p, m in enumerate(fs.policy_set(U, B, H, act, [0, 1, 2, 0, 1]).members)]      # noqa: E731
    grp, seq = mk(), mk()
    src = fs.source(batch, grp[0].actor, own_advantages=True)
    N = src['actions'].shape[0]
    g = torch.Generator(device='cuda').manual_seed(9)
    index = torch.randint(0, N, (3, 130), generator=g, device='cuda', dtype=torch.int32)
    index[0, 3], index[0, 40], index[0, 41], index[0, 99] = -1, N, int(index[0, 7]), int(index[0, 7])
    rows = [100, 77, 0]
    # policy 2 has gradients of an earlier call of its own, in both runs
    for lns in (grp, seq):
        lns[2].grads_indexed(src, index[2, :50].contiguous())
    kept = grp[2].read('grads')
    rc, h, msg = fs.c_group(grp)
    assert rc == 0, msg
    L = _lib.load()
    GUARD = 33
    stats = torch.full((3 * _lib.PPO_NUM_STATS + GUARD,), -12345.0, dtype=torch.float32, device='cuda')
    b = fs.c_group_batch(src, index, rows, compact)
    hy = fs.c_hypers(grp)
    stream = grp[0].actor._stream()
    for again in range(2):
        assert L.dcomp_learner_group_grads(h, ctypes.byref(b), hy, ctypes.c_void_p(stats.data_ptr()), stream) == 0, L.dcomp_last_error()
        got = stats.cpu().numpy()
        assert np.all(got[10:] == -12345.0)                                            # policy 2's row and the guard band
        for p in (0, 1):
            want = seq[p].grads_indexed(src, index[p, :rows[p]].contiguous()).cpu().numpy()
            assert np.array_equal(got[5 * p:5 * p + 5], want) and np.all(np.isfinite(want)), p
            gg, gs = grp[p].read('grads'), seq[p].read('grads')
            for n in ARRAYS:
                assert np.array_equal(gg[n], gs[n]), (p, n)
            assert np.any(gg['w1'] != 0)
        now = grp[2].read('grads')
        for n in ARRAYS:
            assert np.array_equal(now[n], kept[n]), n
    # apply with one member inactive: steps and weights as the per-learner calls leave them
    lr = (ctypes.c_float * 3)(1e-3, 2e-3, 3e-3)
    active = (ctypes.c_int32 * 3)(1, 1, 0)
    assert L.dcomp_learner_group_apply(h, lr, active, stream) == 0, L.dcomp_last_error()
    seq[0].apply(1e-3)
    seq[1].apply(2e-3)
    for p in range(3):
        sg, ss = grp[p].state_dict(), seq[p].state_dict()
        assert sg['step'] == ss['step'] == (1 if p < 2 else 0)
        for k in ('weights', 'm', 'v'):
            for n in ARRAYS:
                assert np.array_equal(sg[k][n], ss[k][n]), (p, k, n)
    assert L.dcomp_learner_group_destroy(h) == 0


def test_chunk_counts_that_fall_as_the_rows_grow(torch_cuda):
    """Policies on both sides of CHUNK_UNIT x MAX_CHUNKS = 262 144 rows: 262 176 rows are 65 weight-gradient chunks, 262 144 rows are
    128 -- the LARGER policy has fewer.  The grouped launch must still run every chunk of both: gradients and statistics equal those
    of dcomp_sgd_grads per policy.  (The C call with an index of repeated source rows: no batch of that size is needed.)"""
    torch = torch_cuda
    from deepcomp_amd import _lib
    from deepcomp_amd.learner import ARRAYS, PPOLearner
    from tests import fcnet_cases as fc
    rows = [262176, 262144]
    assert [fc.row_split(r)['nchunks'] for r in rows] == [65, 128]
    U, B, H, act, E, T, slots, _ = cases.GROUP_CASES['a-rows']
    batch = fs.group_collected('a-rows', U, B, H, act, E, T, slots, False)
    mk = lambda: [PPOLearner(m, max_rows=rows[0], **dict(HYPER, lr=1e-3)) for m in fs.policy_set(U, B, H, act, [0, 1, 0, 1, 0]).members]      # noqa: E731
    grp, seq = mk(), mk()
    src = fs.source(batch, grp[0].actor, own_advantages=True)
    g = torch.Generator(device='cuda').manual_seed(11)
    index = torch.randint(0, src['actions'].shape[0], (2, rows[0]), generator=g, device='cuda', dtype=torch.int32)
    rc, h, msg = fs.c_group(grp)
    assert rc == 0, msg
    L = _lib.load()
    stats = torch.zeros(2 * _lib.PPO_NUM_STATS, dtype=torch.float32, device='cuda')
    b = fs.c_group_batch(src, index, rows, False)
    assert L.dcomp_learner_group_grads(h, ctypes.byref(b), fs.c_hypers(grp), ctypes.c_void_p(stats.data_ptr()), grp[0].actor._stream()) == 0, L.dcomp_last_error()
    got = stats.cpu().numpy()
    for p in (0, 1):
        want = seq[p].grads_indexed(src, index[p, :rows[p]].contiguous()).cpu().numpy()
        assert np.array_equal(got[5 * p:5 * p + 5], want) and np.all(np.isfinite(want)), p
        gg, gs = grp[p].read('grads'), seq[p].read('grads')
        for n in ARRAYS:
            assert np.array_equal(gg[n], gs[n]), (p, n)
        assert np.any(gg['w1'] != 0)
    assert L.dcomp_learner_group_destroy(h) == 0


# ---------------------------------------------------------------------------------------------- 6: mixing
def test_grouped_sequential_and_member_calls_mix(torch_cuda):
    """grouped update -> one member's own PPOLearner.update -> grouped update equals the same sequence run all-sequentially; and
    state_dict -> a new set and learner -> load_state_dict -> grouped update equals the uninterrupted run."""
    from deepcomp_amd.policy_set import policy_rows
    batch, grp, seq = fs.twins('a-compact')
    U, _, _, _, E, T, slots, _ = cases.GROUP_CASES['a-compact']
    rows1 = policy_rows(T * E * U, U, slots, 2, 'cuda')[1]
    saved = None
    for ln, grouped in ((grp, True), (seq, False)):
        ln.update(batch, num_sgd_iter=1, minibatch_rows=64, seed=1, grouped=grouped)
        ln.learners[1].update(batch, num_sgd_iter=1, minibatch_rows=64, seed=8, rows=rows1)
        if grouped:
            saved = ln.state_dict()
        ln.update(batch, num_sgd_iter=1, minibatch_rows=64, seed=2, grouped=grouped)
    for s1, s2 in zip(grp.state_dict(), seq.state_dict()):
        fs.same_state(s1, s2, stepped=True)
    assert [s['step'] for s in grp.state_dict()] == [22, 34 + 17]
    _, _, resumed = fs.twins('a-compact')
    resumed.load_state_dict(saved)
    resumed.update(batch, num_sgd_iter=1, minibatch_rows=64, seed=2, grouped=True)
    for s1, s2 in zip(grp.state_dict(), resumed.state_dict()):
        fs.same_state(s1, s2, stepped=True)


# ---------------------------------------------------------------------------------------------- 7: refusals that need handles
def test_refusals_that_need_handles(torch_cuda):
    torch = torch_cuda
    from deepcomp_amd import _lib
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.learner import PPOLearner
    L = _lib.load()

    def learner(U=5, B=3, H=32, act='tanh', kind='multi', seed=1, max_rows=64):
        a = FcnetActor(kind, U, B, FcnetActor.random_weights(kind, U, B, H, seed=seed, bias_std=0.1), activation=act,
                       value_weights=FcnetActor.random_value_weights(kind, U, B, H, seed=seed, bias_std=0.1))
        return PPOLearner(a, max_rows=max_rows, **HYPER)
    base = learner()
    for other, what in ((learner(H=64), 'hidden'), (learner(act='relu'), 'activation'), (learner(U=4), 'num_ue'), (learner(B=4), 'num_bs')):
        rc, h, msg = fs.c_group([base, other])
        assert rc == EINVAL and h.value is None and 'dcomp_learner_group_create' in msg and what in msg, msg
    rc, h, msg = fs.c_group([base, base])
    assert rc == EINVAL and 'learner 1 is learner 0 again' in msg
    rc, h, msg = fs.c_group([base, PPOLearner(base.actor, max_rows=64, **HYPER)])
    assert rc == EINVAL and 'the same actor' in msg
    rc, h, msg = fs.c_group([learner(kind='central'), learner(kind='central', seed=2)])
    assert rc == EUNSUPPORTED and 'dcomp_learner_group_create' in msg and 'DCOMP_CENTRAL' in msg
    rc, h, msg = fs.c_group([base, learner(kind='central')])
    assert rc == EINVAL and 'obs_kind' in msg

    U, B, H, act, E, T, slots, _ = cases.GROUP_CASES['a-rows']
    second = learner(seed=2, max_rows=32)
    rc, h, msg = fs.c_group([base, second])
    assert rc == 0, msg
    rows_src = fs.source(fs.group_collected('a-rows', U, B, H, act, E, T, slots, False), base.actor, own_advantages=True)
    compact_src = fs.source(fs.group_collected('a-compact', U, B, H, act, E, T, slots, True), base.actor, own_advantages=True)
    N = rows_src['actions'].shape[0]
    index = torch.zeros((2, 80), dtype=torch.int32, device='cuda')
    narrow = torch.zeros((2, 16), dtype=torch.int32, device='cuda')
    stats = torch.zeros(10, dtype=torch.float32, device='cuda')
    hy = fs.c_hypers([base, second])

    def grads(b):
        rc = L.dcomp_learner_group_grads(h, ctypes.byref(b), hy, ctypes.c_void_p(stats.data_ptr()), None)
        return rc, L.dcomp_last_error().decode()
    for b, what in ((fs.c_group_batch(rows_src, index, [65, 10], False), 'rows[0] 65'), (fs.c_group_batch(rows_src, index, [10, 33], False), 'rows[1] 33'),
                    (fs.c_group_batch(rows_src, index, [-1, 10], False), 'rows[0] -1'), (fs.c_group_batch(rows_src, narrow, [17, 10], False), 'index_stride'),
                    (fs.c_group_batch(rows_src, index, [0, 0], False), 'at least one'),
                    (fs.c_group_batch(compact_src, index, [10, 10], True, source_rows=N - 1), 'multiple of num_ue'),
                    (fs.c_group_batch(rows_src, index, [10, 10], False, source_rows=0), 'source_rows')):
        rc, msg = grads(b)
        assert rc == EINVAL and 'dcomp_learner_group_grads' in msg and what in msg, (what, msg)
    torch.cuda.synchronize()
    assert bool((stats == 0).all())                                                    # nothing was launched
    assert base.state_dict()['step'] == 0
    bad_lr = (ctypes.c_float * 2)(1e-3, float('nan'))
    assert L.dcomp_learner_group_apply(h, bad_lr, None, None) == EINVAL and b'lr[1]' in L.dcomp_last_error()
    assert L.dcomp_learner_group_apply(h, bad_lr, (ctypes.c_int32 * 2)(0, 0), None) == EINVAL and b'no member is active' in L.dcomp_last_error()
    assert L.dcomp_learner_group_destroy(h) == 0
