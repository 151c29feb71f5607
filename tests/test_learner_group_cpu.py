"""CPU-side checks of the grouped PPO learner (include/dcomp_learner_group.h, PerUELearner.update(grouped=True)): the four entry
points exist and are declared, the two ctypes mirrors match the header, every argument the library can judge without dereferencing a
handle is refused on the host before the first HIP call, and the table of grouped cases tests/test_learner_group_gpu.py runs reaches
every grouped instantiation and every weight-gradient form.  No GPU compute is called here."""
import ctypes
import re
import subprocess

from tests import c_surface as cs
from tests.c_surface import EABI, EINVAL, OK, REPO, lib  # noqa: F401  (lib: the fixture)
from tests.group_cases import GROUP_CASES, group_slice

HEADER = cs.header('dcomp_learner_group.h')


def test_symbols_are_exported_and_declared(lib):
    from deepcomp_amd import _lib
    hdr = open(HEADER).read()
    assert _lib.GROUP_EXPORTS == ['dcomp_learner_group_create', 'dcomp_learner_group_destroy', 'dcomp_learner_group_grads', 'dcomp_learner_group_apply']
    for name in _lib.GROUP_EXPORTS:
        assert re.search(r'\bint %s\s*\(' % name, hdr), name
        getattr(lib, name)
        assert all(name not in lst for lst in (_lib.EXPORTS, _lib.LEARNER_EXPORTS, _lib.SGD_EXPORTS, _lib.SET_EXPORTS))
    assert sorted(re.findall(r'\bint (dcomp_\w+)\s*\(', hdr)) == sorted(_lib.GROUP_EXPORTS)
    assert group_slice() >= 64
    assert -(-128 // group_slice()) <= 2                                               # config 5's 128 policies: at most two launch rounds
    for other in ('dcomp.h', 'dcomp_types.h', 'dcomp_learner.h', 'dcomp_learner_indexed.h', 'dcomp_policy_set.h'):
        assert not re.search(r'dcomp_learner_group', open(cs.header(other)).read()), other


def test_ctypes_mirrors_match_the_header(tmp_path):
    """Member names from the header text, sizes and offsets from a C program compiled against it (C99, pedantic)."""
    from deepcomp_amd import _lib
    mirrors = {'dcomp_learner_group_cfg': _lib.DcompLearnerGroupCfg, 'dcomp_group_batch': _lib.DcompGroupBatch}
    prints = []
    for name, S in mirrors.items():
        names = cs.struct_members(HEADER, name)
        assert names == [f[0] for f in S._fields_], names
        prints.append('    printf("%%zu", sizeof(%s));\n' % name + ''.join('    printf(" %%zu", offsetof(%s, %s));\n' % (name, m) for m in names) + '    printf("\\n");\n')
    lines = cs.c_program_output(tmp_path, '#include <stdio.h>\n#include <stddef.h>\n#include "dcomp_learner_group.h"\nint main(void) {\n' + ''.join(prints) +
                                '    return DCOMP_EABI == -7 && DCOMP_GROUP_SLICE >= 64 ? 0 : 1;\n}\n')
    for line, S in zip(lines, mirrors.values()):
        assert line == [ctypes.sizeof(S)] + [getattr(S, f[0]).offset for f in S._fields_], S


def _cfg(num_learners=2, learners='fake', size=None):
    from deepcomp_amd import _lib
    if learners == 'fake':
        learners = [4096]                                                              # (never dereferenced by the checks under test)
    arr = (ctypes.c_void_p * len(learners))(*learners) if learners is not None else None
    cfg = _lib.DcompLearnerGroupCfg(ctypes.sizeof(_lib.DcompLearnerGroupCfg) if size is None else size, num_learners, arr)
    cfg._keep = arr
    return cfg


def test_create_refuses_what_needs_no_handle_on_the_host(lib):
    from deepcomp_amd import _lib
    err = lib.dcomp_last_error
    out = ctypes.c_void_p(1234)
    create = lambda c, o=out: lib.dcomp_learner_group_create(ctypes.byref(c) if c is not None else None, ctypes.byref(o) if o is not None else None)      # noqa: E731
    assert create(None) == EINVAL and b'dcomp_learner_group_create' in err() and b'cfg' in err()
    assert out.value is None                                                           # *out is cleared on every failure
    assert lib.dcomp_learner_group_create(ctypes.byref(_cfg()), None) == EINVAL and b'out' in err()
    for size in (0, ctypes.sizeof(_lib.DcompLearnerGroupCfg) - 8, ctypes.sizeof(_lib.DcompLearnerGroupCfg) + 8):
        assert create(_cfg(size=size)) == EABI and b'dcomp_learner_group_cfg' in err()
    assert create(_cfg(learners=None)) == EINVAL and b'learners' in err()
    for P in (0, -1, _lib.MAX_UE + 1):
        assert create(_cfg(num_learners=P)) == EINVAL and b'num_learners' in err(), P
    assert create(_cfg(num_learners=2, learners=[4096, None])) == EINVAL and b'learner 1 is NULL' in err()
    assert create(_cfg(num_learners=1, learners=[None])) == EINVAL and b'learner 0 is NULL' in err()
    assert create(_cfg(num_learners=2, learners=[4096, 4096])) == EINVAL and b'learner 1 is learner 0 again' in err()
    assert out.value is None
    assert lib.dcomp_learner_group_destroy(None) == OK


def test_grads_and_apply_refuse_nulls_and_a_wrong_struct_size(lib):
    """With a fake group handle that is never dereferenced: these checks come before the group is read."""
    from deepcomp_amd import _lib
    err = lib.dcomp_last_error
    fake = ctypes.c_void_p(4096)
    batch = lambda size=None: _lib.DcompGroupBatch(ctypes.sizeof(_lib.DcompGroupBatch) if size is None else size)      # noqa: E731
    hyper = cs.ppo_hyper()
    grads = lambda g, b, h, s: lib.dcomp_learner_group_grads(g, ctypes.byref(b) if b is not None else None, ctypes.byref(h) if h is not None else None, s, None)      # noqa: E731
    for args in ((None, batch(), hyper, fake), (fake, None, hyper, fake), (fake, batch(), None, fake), (fake, batch(), hyper, None)):
        assert grads(*args) == EINVAL and b'dcomp_learner_group_grads:' in err() and b'NULL' in err()
    for size in (0, ctypes.sizeof(_lib.DcompGroupBatch) - 8, ctypes.sizeof(_lib.DcompGroupBatch) + 8):
        assert grads(fake, batch(size), hyper, fake) == EABI and b'dcomp_learner_group_grads:' in err() and b'dcomp_group_batch' in err()
    assert grads(fake, batch(), hyper, fake) == EINVAL and b'batch.rows' in err()      # rows and index NULL
    lr = (ctypes.c_float * 1)(1e-3)
    assert lib.dcomp_learner_group_apply(None, lr, None, None) == EINVAL and b'dcomp_learner_group_apply:' in err() and b'NULL' in err()
    assert lib.dcomp_learner_group_apply(fake, None, None, None) == EINVAL and b'dcomp_learner_group_apply:' in err() and b'NULL' in err()


def test_the_grouped_cases_reach_every_instantiation_and_weight_gradient_form(lib):
    """learner_group_kernel<MT, RELU> for MT in 1, 2, 4, 8 x tanh / relu; wgrad_block<1, 1>, <2, 1>, <1, 4>, <2, 4>; wgrad_bias<1>, <4>:
    which cell a shape reaches is the library's answer (tests/fcnet_cases.py: dcomp_fcnet_describe)."""
    from tests import fcnet_cases as fc
    kernels, blocks, biases = {}, {}, {}
    for name, (U, B, H, act, E, T, slots, compact) in GROUP_CASES.items():
        d = fc.learner_dispatch('multi', U, B, H)
        kernels.setdefault((d['mt'], act), []).append(name)
        for blk in d['blocks']:
            blocks.setdefault(blk, []).append(name)
        for nb in d['bias']:
            biases.setdefault(nb, []).append(name)
        assert len(slots) == U and fc.describe('multi', U, B, H).actor.hidden == H
    assert sorted(kernels) == sorted((mt, act) for mt in (1, 2, 4, 8) for act in ('relu', 'tanh')), kernels
    assert sorted(blocks) == [(1, 1), (1, 4), (2, 1), (2, 4)], blocks
    assert sorted(biases) == [1, 4], biases
    # the forms the issue names, where it names them
    assert (1, 1) in fc.learner_dispatch('multi', 5, 3, 32)['blocks'] and fc.learner_dispatch('multi', 5, 3, 64)['blocks'][2] == (2, 1)
    assert (1, 4) in fc.learner_dispatch('multi', 4, 5, 128)['blocks'] and 4 in fc.learner_dispatch('multi', 4, 5, 128)['bias']
    assert (2, 4) in fc.learner_dispatch('multi', 4, 10, 128)['blocks']
    # the uneven split of the first GPU test: 11 against 17 minibatch rounds, last minibatches of 60 and 26 rows
    U, B, H, act, E, T, slots, _ = GROUP_CASES['a-rows']
    n = [T * E * slots.count(p) for p in (0, 1)]
    assert n == [700, 1050] and [-(-x // 64) for x in n] == [11, 17] and [x % 64 for x in n] == [60, 26]
    # several weight-gradient chunks that differ per policy (the third GPU test): 4 500 rows are 3 chunks, 2 250 are 2
    assert [fc.row_split(r)['nchunks'] for r in (4500, 2250)] == [3, 2] and 4500 % fc.row_split(4500)['chunk_rows'] != 0


def test_the_chunk_axis_of_a_grouped_launch_is_the_largest_chunk_count_not_the_largest_policys(tmp_path):
    """row_split(rows).nchunks is not monotonic: past CHUNK_UNIT x MAX_CHUNKS = 262 144 padded rows the chunks get longer and fewer.
    group_chunks (csrc/dcomp_fcnet_plan.h), which sizes wgrad_group_kernel's chunk axis, must cover every policy's own count -- a
    stand-alone host program over the plan header alone."""
    from tests import fcnet_cases as fc
    n = {r: fc.row_split(r)['nchunks'] for r in (300000, 200000, 262176, 262144, 4500, 2250)}
    assert n == {300000: 74, 200000: 98, 262176: 65, 262144: 128, 4500: 3, 2250: 2}, n      # the larger policy has FEWER chunks, twice
    src = tmp_path / 'group_chunks.cpp'
    src.write_text('#include <cstdio>\n#include "deepcomp_amd/csrc/dcomp_fcnet_plan.h"\n'
                   'int main() {\n'
                   '    const int64_t a[2] = {300000, 200000}, b[2] = {262176, 262144}, c[3] = {0, 4500, 2250}, d[2] = {0, 0}, e[2] = {200000, 300000};\n'
                   '    std::printf("%d %d %d %d %d\\n", dlearn::group_chunks(a, 2), dlearn::group_chunks(b, 2), dlearn::group_chunks(c, 3),\n'
                   '                dlearn::group_chunks(d, 2), dlearn::group_chunks(e, 2));\n'
                   '    return 0;\n}\n')
    exe = tmp_path / 'group_chunks'
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', REPO, '-o', str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [max(n[300000], n[200000]), max(n[262176], n[262144]), 3, 0, 98] == [98, 128, 3, 0, 98], got

