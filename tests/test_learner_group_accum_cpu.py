"""CPU-side checks of the grouped accumulated gradients (include/dcomp_learner_group_accum.h, PerUELearner.update(grouped=True,
micro_rows=, grad_clip=), deepcomp_amd.dp_learner.DataParallelPerUELearner): the header compiles as C, the two entry points exist and
are declared, every argument the library can judge before its first HIP call is refused in the order the header documents, the
grouped micro-batch plan hands every policy the positions its own PPOLearner.update would take, and the shapes of
tests/test_learner_group_accum_gpu.py reach what that file claims of them.  No GPU compute is called here.

The refusals that depend on the group (rows against max_rows, the number of members) are made on FAKE handles: memory images that
hold only what the checks under test read before they refuse -- of a group its member list (the three pointers of a std::vector),
of a member its max_rows (the second 64-bit word of the handle).  Everything else in them is zero and is never reached."""
import ctypes
import os
import re

import pytest

from tests import c_surface as cs
from tests.c_surface import EABI, EINVAL, REPO, lib  # noqa: F401  (lib: the fixture)
from tests.c_surface import group_batch as _batch
from tests.c_surface import ppo_hypers as _hypers
from tests.group_cases import CALL, CALL_ROWS, CHUNK, FINISH, GROUP_CASES, LOCK, LOCK4, PLANS, UPDATE, group_slice

HEADER = cs.header('dcomp_learner_group_accum.h')
NAMES = ['dcomp_learner_group_accumulate', 'dcomp_learner_group_accum_finish']


def test_symbols_are_exported_and_declared_and_the_header_is_c(lib, tmp_path):
    from deepcomp_amd import _lib
    hdr = open(HEADER).read()
    assert _lib.GROUP_ACCUM_EXPORTS == NAMES
    for name in NAMES:
        assert re.search(r'\bint %s\s*\(' % name, hdr), name
        getattr(lib, name)
        assert not any(name in lst for lst in (_lib.EXPORTS, _lib.LEARNER_EXPORTS, _lib.SGD_EXPORTS, _lib.GROUP_EXPORTS, _lib.ACCUM_EXPORTS))
    assert sorted(re.findall(r'\bint (dcomp_\w+)\s*\(', hdr)) == sorted(NAMES)
    assert '#include "dcomp_learner_group.h"' in hdr and '#include "dcomp_learner_accum.h"' in hdr
    every = ''.join(f'#include "{h}"\n' for h in ('dcomp.h', 'dcomp_learner.h', 'dcomp_learner_indexed.h', 'dcomp_policy_set.h', 'dcomp_learner_group.h',
                                                   'dcomp_learner_accum.h', 'dcomp_learner_group_accum.h'))
    main = 'int main(void) { return DCOMP_ACCUM_SUMS == 8 && DCOMP_GROUP_SLICE >= 64 && DCOMP_EABI == -7 ? 0 : 1; }\n'
    cs.compiles_as_c99(tmp_path, 'group_accum', [text + main for text in (
        '#include "dcomp_learner_group_accum.h"\n', every, '#include "dcomp_learner_group_accum.h"\n' + every)])
    # both of the build's header lists name it: the source list and dcomp_learner.o's dependency rule
    assert open(os.path.join(REPO, 'deepcomp_amd', 'build.py')).read().count("'dcomp_learner_group_accum.h'") == 2


# ---------------------------------------------------------------------------------------------- fake handles
class _FakeGroup:
    """The image of a group of len(max_rows) members, as far as the checks under test read it (the module docstring)."""

    def __init__(self, max_rows):
        P = len(max_rows)
        self.zero = (ctypes.c_int64 * 8192)()                                          # where a member's actor pointer leads: zeros
        self.members = [(ctypes.c_int64 * 1024)() for _ in range(P)]
        for m, r in zip(self.members, max_rows):
            m[0], m[1] = ctypes.addressof(self.zero), r
        self.list = (ctypes.c_void_p * P)(*[ctypes.addressof(m) for m in self.members])
        self.image = (ctypes.c_int64 * 8)()
        self.image[0] = ctypes.addressof(self.list)
        self.image[1] = self.image[2] = ctypes.addressof(self.list) + 8 * P
        self.handle = ctypes.c_void_p(ctypes.addressof(self.image))


def test_accumulate_refuses_in_the_documented_order(lib):
    from deepcomp_amd import _lib
    err = lib.dcomp_last_error
    name = b'dcomp_learner_group_accumulate:'
    fake = ctypes.c_void_p(4096)
    own = ctypes.sizeof(_lib.DcompGroupBatch)
    acc = lambda g, b, h, a, s: lib.dcomp_learner_group_accumulate(g, ctypes.byref(b) if b is not None else None, h, a, s, None)      # noqa: E731
    # 1: NULL arguments, before anything is read (a group handle that leads nowhere, a batch whose struct_size is wrong)
    for args in ((None, _batch(size=0), _hypers(1), fake, fake), (fake, None, _hypers(1), fake, fake), (fake, _batch(size=0), None, fake, fake),
                 (fake, _batch(size=0), _hypers(1), None, fake), (fake, _batch(size=0), _hypers(1), fake, None)):
        assert acc(*args) == EINVAL and name in err() and b'NULL' in err(), err()
    assert acc(fake, _batch(size=0), _hypers(1), None, fake) == EINVAL and b'acc_dev' in err()
    # 2: the struct size, before the group is read
    for size in (0, own - 8, own + 8):
        assert acc(fake, _batch(size=size), _hypers(1), fake, fake) == EABI and name in err() and b'dcomp_group_batch' in err()
    # 3: rows / index NULL
    assert acc(fake, _batch(rows=None), _hypers(1), fake, fake) == EINVAL and b'batch.rows' in err()
    assert acc(fake, _batch(rows=[1], index=None), _hypers(1), fake, fake) == EINVAL and b'batch.index' in err()
    # 4: per member in order -- rows[p] against max_rows, against the stride, then the member's own checks
    g = _FakeGroup([32, 48, 16])
    hy = _hypers(3)
    for rows, what in (([33, 49, 0], b'rows[0] 33'), ([32, 49, 99], b'rows[1] 49'), ([-1, 0, 0], b'rows[0] -1'), ([0, 0, 17], b'rows[2] 17')):
        assert acc(g.handle, _batch(rows=rows), hy, fake, fake) == EINVAL and name in err() and what in err() and b'max_rows' in err(), err()
    assert acc(g.handle, _batch(rows=[0, 48, 0], stride=47), hy, fake, fake) == EINVAL and b'rows[1] 48 > index_stride 47' in err()
    assert acc(g.handle, _batch(rows=[33, 48, 0], stride=47), hy, fake, fake) == EINVAL and b'rows[0] 33' in err()      # max_rows of 0 before the stride of 1
    assert acc(g.handle, _batch(rows=[0, 4, 0]), _hypers(3, size=8, bad=1), fake, fake) == EABI and b'dcomp_ppo_hyper' in err() and name in err()
    assert acc(g.handle, _batch(rows=[0, 4, 0], given=False), hy, fake, fake) == EINVAL and b'obs' in err()
    assert acc(g.handle, _batch(rows=[0, 4, 0], source_rows=0), hy, fake, fake) == EINVAL and b'source_rows' in err()
    # 5: all rows 0
    assert acc(g.handle, _batch(rows=[0, 0, 0]), hy, fake, fake) == EINVAL and name in err() and b'at least one' in err()
    assert acc(g.handle, _batch(rows=[0, 0, 17]), hy, fake, fake) == EINVAL and b'rows[2] 17' in err()                   # ... after the per-member checks


def test_finish_refuses_in_the_documented_order(lib):
    err = lib.dcomp_last_error
    name = b'dcomp_learner_group_accum_finish:'
    fake = ctypes.c_void_p(4096)
    fin = lambda g, a, s, h, clip=None, active=None: lib.dcomp_learner_group_accum_finish(      # noqa: E731
        g, a, s, h, (ctypes.c_float * len(clip))(*clip) if clip is not None else None,
        (ctypes.c_int32 * len(active))(*active) if active is not None else None, None, None, None)
    for args, what in (((None, fake, fake, _hypers(1)), b'group'), ((fake, None, fake, _hypers(1)), b'acc_dev'), ((fake, fake, None, _hypers(1)), b'sums_dev'),
                       ((fake, fake, fake, None), b'hyper')):
        assert fin(*args) == EINVAL and name in err() and what in err() and b'NULL' in err(), err()
    g = _FakeGroup([32, 32, 32])
    assert fin(g.handle, fake, fake, _hypers(3, size=4, bad=2)) == EABI and b'dcomp_ppo_hyper' in err() and name in err()
    for bad in (-1.0, -1e-30, float('nan'), float('-inf')):
        assert fin(g.handle, fake, fake, _hypers(3), clip=[0.0, bad, 1.0]) == EINVAL and name in err() and b'grad_clip[1]' in err(), bad
        assert fin(g.handle, fake, fake, _hypers(3), clip=[0.0, bad, 1.0], active=[0, 0, 0]) == EINVAL and b'no member is active' in err()
    assert fin(g.handle, fake, fake, _hypers(3, size=4, bad=0), clip=[-1.0, 0.0, 0.0]) == EABI                           # per member: the size before the clip
    assert fin(g.handle, fake, fake, _hypers(3), active=[0, 0, 0]) == EINVAL and name in err() and b'no member is active' in err()


# ---------------------------------------------------------------------------------------------- the plan
def _member_positions(n, minibatch_rows, max_rows, micro_rows, grad_clip):
    """What PPOLearner.update(rows=..., minibatch_rows=, micro_rows=, grad_clip=) does with a permutation of n positions: per minibatch
    the list of (start, stop) slices it hands to the library -- update()'s loop over minibatch_stats' starts, accumulate_minibatch's
    loop over the micro-batches (submit_picks takes the whole minibatch when the update is not accumulated)."""
    from deepcomp_amd.learner import minibatch_plan
    mb, micro, accumulated = minibatch_plan(n, minibatch_rows, max_rows, micro_rows, grad_clip)
    out = []
    for s in range(0, n, mb):
        stop = min(s + mb, n)
        out.append([(lo, min(lo + micro, stop)) for lo in range(s, stop, micro)] if accumulated else [(s, stop)])
    return out, accumulated


@pytest.mark.parametrize('name', sorted(PLANS))
def test_the_grouped_plan_hands_every_policy_its_own_positions(lib, name):
    from deepcomp_amd.policy_set import group_plan
    n_of, minibatch_rows, max_rows, micro_rows, grad_clip = PLANS[name]
    P = len(n_of)
    accumulated, taken, rounds = group_plan(n_of, minibatch_rows, [max_rows] * P, micro_rows, grad_clip)
    assert accumulated == (micro_rows is not None or grad_clip is not None)
    for p in range(P):
        if not n_of[p]:
            assert taken[p] == 0 and all(rr[p] == 0 and all(r[p] == 0 for _, r in micro) for rr, micro in rounds)
            continue
        want, acc_p = _member_positions(n_of[p], minibatch_rows, max_rows, micro_rows, grad_clip)
        assert acc_p == accumulated and taken[p] == len(want)
        got = []
        for k, (rr, micro) in enumerate(rounds):
            mine = [(off, off + r[p]) for off, r in micro if r[p]]
            assert (rr[p] > 0) == (k < taken[p]) and sum(b - a for a, b in mine) == rr[p]
            if mine:
                got.append(mine)
            # a policy's launches of a round are its first ones: once it sits a launch out it has no rows left in this round
            flags = [r[p] > 0 for _, r in micro]
            assert flags == sorted(flags, reverse=True)
            assert all(r[p] <= max_rows for _, r in micro)
        assert got == want, (p, got, want)
    for rr, micro in rounds:                                                           # no launch without a policy in it
        assert any(rr) and all(any(r) for _, r in micro)
    assert len(rounds) == max(taken)


def test_the_plans_are_the_ones_the_issue_describes(lib):
    from deepcomp_amd.policy_set import group_plan
    _, taken, rounds = group_plan(*PLANS['whole-batch'][:2], [2048] * 3, 2048, 0.5)
    assert taken == [1, 1, 1] and [r for _, r in rounds[0][1]] == [[2048, 2048, 2048], [2048, 252, 252], [504, 0, 0]]
    _, taken, rounds = group_plan(*PLANS['two-rounds'][:2], [2048] * 3, 2048, 0.5)
    assert taken == [2, 1, 1] and [rr for rr, _ in rounds] == [[3000, 2300, 2300], [1600, 0, 0]]
    assert [(off, r) for off, r in rounds[0][1]] == [(0, [2048, 2048, 2048]), (2048, [952, 252, 252])] and rounds[1][1] == [(3000, [1600, 0, 0])]
    # refusals are minibatch_plan's own
    with pytest.raises(ValueError, match='max_rows'):
        group_plan([4600, 2300], 3000, [2048, 2048])
    with pytest.raises(ValueError, match='multiple'):
        group_plan([4600, 2300], 3000, [2048, 2048], micro_rows=1000)
    with pytest.raises(ValueError, match='grad_clip'):
        group_plan([100, 100], None, [2048, 2048], grad_clip=-1.0)


# ---------------------------------------------------------------------------------------------- what the shapes reach
def _flat(U, B, H):
    from deepcomp_amd.actor import layer_shapes
    nin, heads, nout, shapes = layer_shapes('multi', U, B, H)
    policy = sum(a * (b[0] if b else 1) for a, *b in shapes.values())
    return policy + (nin * H + H) + (H * H + H) + (H + 1)                              # + the value trunk: vw1 vb1 vw2 vb2 wv bv


def test_the_shapes_reach_what_the_gpu_tests_claim(lib):
    from tests import fcnet_cases as fc
    assert fc.CHUNK_UNIT == CHUNK
    # finish: fewer entries than one 4 096-entry norm block and no multiple of 256; three norm partials and 46 blocks of 256
    for U in (1, 4, 9):
        assert _flat(U, 5, 32) == 3751 and _flat(U, 5, 64) == 11591
    assert 3751 < 4096 and 3751 % 256 and -(-3751 // 4096) == 1
    assert -(-11591 // 4096) == 3 and -(-11591 // 256) == 46 and 11591 % 256
    assert all(_flat(*FINISH[h][:3]) == n for h, n in ((32, 3751), (64, 11591)))
    # accumulate: 3 and 2 weight-gradient chunks, the last of the larger one partial; the index fits the batch's source rows
    assert [fc.row_split(r)['nchunks'] for r in CALL_ROWS[:2]] == [3, 2] and 4500 % CHUNK
    U, B, H, E, T, slots = CALL
    assert (U, B, H, E) == GROUP_CASES['a-rows'][:2] + (GROUP_CASES['a-rows'][2], GROUP_CASES['a-rows'][4]) and T > GROUP_CASES['a-rows'][5]
    assert T * E * U >= max(CALL_ROWS) and max(slots) == 2
    # update: 4 600 / 2 300 / 2 300 rows in micro-batches of 2 048 + 2 048 + 504 and 2 048 + 252
    U, B, H, E, T, slots = UPDATE
    assert [T * E * slots.count(p) for p in range(3)] == [4600, 2300, 2300] == PLANS['whole-batch'][0]
    assert 4600 == 2 * CHUNK + 504 and 2300 == CHUNK + 252
    # lockstep: equal shards per policy for two and three ranks
    U, B, H, E, T, slots = LOCK
    assert [T * E * slots.count(p) for p in range(2)] == [512, 512] and len(set(LOCK4[5])) == 4
    assert group_slice() + 1 == 65
