"""CPU-side checks of the learner's indexed minibatches (include/dcomp_learner_indexed.h, deepcomp_amd/learner.py): the two entry points
exist and are declared, the ctypes mirror matches the header, the header compiles as C alone and next to the other two, and every
argument the library can judge without its handle is refused on the host before the first HIP call -- with a fake handle that is
never dereferenced.  The refusals that read the handle (rows > max_rows, the compact record with a central handle, source rows that
are not whole envs, num_active of a multi-agent handle) are in tests/test_learner_indexed_gpu.py.  No GPU compute is called here."""
import ctypes
import re

import pytest

from tests import c_surface as cs
from tests.c_surface import EABI, EINVAL, EUNSUPPORTED, lib  # noqa: F401  (lib: the fixture)
from tests.c_surface import LOSS_INPUTS as _LOSS_INPUTS
from tests.c_surface import ppo_hyper as _hyper
from tests.c_surface import sgd_batch as _batch

HEADER = cs.header('dcomp_learner_indexed.h')


def test_symbols_are_exported_and_declared(lib):
    from deepcomp_amd import _lib
    hdr = open(HEADER).read()
    assert _lib.SGD_EXPORTS == ['dcomp_sgd_grads', 'dcomp_sgd_evaluate']
    for name in _lib.SGD_EXPORTS:
        assert re.search(r'\bint %s\s*\(' % name, hdr), name
        getattr(lib, name)
        assert name not in _lib.EXPORTS and name not in _lib.LEARNER_EXPORTS
    assert sorted(re.findall(r'\bint (dcomp_\w+)\s*\(', hdr)) == sorted(_lib.SGD_EXPORTS)
    # the surfaces the existing tests pin are as they were
    assert len(_lib.LEARNER_EXPORTS) == 7 and len(_lib.EXPORTS) == 42
    assert not re.search(r'dcomp_sgd_', open(cs.header('dcomp_learner.h')).read())


def test_ctypes_mirror_matches_the_header(tmp_path):
    """Member names from the header text, sizes from a C program compiled against it (C99, pedantic); dcomp_ppo_batch keeps its size."""
    from deepcomp_amd import _lib
    members = cs.struct_members(HEADER, 'dcomp_sgd_batch')
    assert members == [f[0] for f in _lib.DcompSgdBatch._fields_], members
    sizes, = cs.c_program_output(                                                      # (compiled alone first)
        tmp_path, '#include <stdio.h>\n#include <stddef.h>\n#include "dcomp_learner_indexed.h"\n'
                   'int main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu\\n", sizeof(dcomp_sgd_batch), sizeof(dcomp_ppo_batch), offsetof(dcomp_sgd_batch, index),\n'
                   '           offsetof(dcomp_sgd_batch, obs), offsetof(dcomp_sgd_batch, ratio));\n'
                   '    return 0;\n'
                   '}\n')
    main = 'int main(void) { return DCOMP_EABI == -7 && DCOMP_ACTOR_COMPACT == 1 ? 0 : 1; }\n'
    cs.compiles_as_c99(tmp_path, 'both', [text + main for text in (                    # with the other two public headers, either order
        '#include "dcomp.h"\n#include "dcomp_learner.h"\n#include "dcomp_learner_indexed.h"\n',
        '#include "dcomp_learner_indexed.h"\n#include "dcomp_learner.h"\n#include "dcomp.h"\n')])
    S = _lib.DcompSgdBatch
    assert sizes == [ctypes.sizeof(S), ctypes.sizeof(_lib.DcompPpoBatch), S.index.offset, S.obs.offset, S.ratio.offset]
    assert ctypes.sizeof(_lib.DcompPpoBatch) == 24 + 14 * 8                           # (as before this header existed)


def test_grads_refuses_bad_arguments_on_the_host(lib):
    from deepcomp_amd import _lib
    fake = ctypes.c_void_p(4096)
    err = lib.dcomp_last_error
    g = lambda l, b, h, s: lib.dcomp_sgd_grads(l, ctypes.byref(b) if b is not None else None, ctypes.byref(h) if h is not None else None, s, None)      # noqa: E731
    assert g(None, _batch(), _hyper(), fake) == EINVAL and b'handle' in err()
    assert g(fake, None, _hyper(), fake) == EINVAL
    assert g(fake, _batch(), None, fake) == EINVAL and b'hyper' in err()
    assert g(fake, _batch(), _hyper(), None) == EINVAL and b'stats_dev' in err()
    for size in (0, ctypes.sizeof(_lib.DcompPpoBatch), ctypes.sizeof(_lib.DcompSgdBatch) + 8):
        assert g(fake, _batch(size=size), _hyper(), fake) == EABI and b'dcomp_sgd_batch' in err()
    assert g(fake, _batch(), _hyper(size=8), fake) == EABI and b'dcomp_ppo_hyper' in err()
    assert g(fake, _batch(), _hyper(clip=-0.1), fake) == EINVAL and b'clip_param' in err()
    assert g(fake, _batch(), _hyper(vf_clip=float('nan')), fake) == EINVAL
    assert g(fake, _batch(fmt=2), _hyper(), fake) == EINVAL and b'obs_format' in err()
    assert g(fake, _batch(fmt=-1), _hyper(), fake) == EINVAL
    for fmt in (0, 1):                                                    # rows and the compact record: the same checks up to the handle
        assert g(fake, _batch(given=_LOSS_INPUTS[1:], fmt=fmt), _hyper(), fake) == EINVAL and b'obs' in err()
        for missing in _LOSS_INPUTS[1:]:
            rc = g(fake, _batch(given=[n for n in _LOSS_INPUTS if n != missing], fmt=fmt), _hyper(), fake)
            assert rc == EINVAL and b'NULL' in err(), missing
        assert g(fake, _batch(given=('obs', 'dlogits'), fmt=fmt), _hyper(), fake) == EINVAL and b'together' in err()
        assert g(fake, _batch(given=('obs', 'dvalue'), fmt=fmt), _hyper(), fake) == EINVAL
        assert g(fake, _batch(rows=0, fmt=fmt), _hyper(), fake) == EINVAL and b'rows' in err()
        assert g(fake, _batch(given=('obs', 'dlogits', 'dvalue'), rows=-1, fmt=fmt), _hyper(), fake) == EINVAL
        assert g(fake, _batch(source_rows=0, fmt=fmt), _hyper(), fake) == EINVAL and b'source_rows' in err()
        assert g(fake, _batch(source_rows=-5, fmt=fmt), _hyper(), fake) == EINVAL
        assert g(fake, _batch(source_rows=2 ** 31, fmt=fmt), _hyper(), fake) == EINVAL and b'2^31' in err()
        assert g(fake, _batch(rows=65, source_rows=64, index=None, fmt=fmt), _hyper(), fake) == EINVAL and b'index' in err()


def test_evaluate_refuses_bad_arguments_on_the_host(lib):
    fake = ctypes.c_void_p(4096)
    err = lib.dcomp_last_error
    ev = lambda l, b: lib.dcomp_sgd_evaluate(l, ctypes.byref(b) if b is not None else None, None)      # noqa: E731
    ok = ('obs', 'actions', 'logp')
    assert ev(None, _batch(given=ok)) == EINVAL
    assert ev(fake, None) == EINVAL
    assert ev(fake, _batch(given=ok, size=16)) == EABI and b'dcomp_sgd_batch' in err()
    assert ev(fake, _batch(given=ok, fmt=3)) == EINVAL and b'obs_format' in err()
    assert ev(fake, _batch(given=('actions', 'logp'))) == EINVAL and b'obs' in err()
    assert ev(fake, _batch(given=('obs', 'logp'))) == EINVAL and b'actions' in err()
    assert ev(fake, _batch(given=('obs', 'actions'))) == EINVAL and b'nothing to write' in err()
    assert ev(fake, _batch(given=('obs', 'actions', 'vf', 'dlogits', 'dvalue'))) == EINVAL and b'upstream' in err()
    assert ev(fake, _batch(given=('obs', 'actions', 'vf'), rows=0)) == EINVAL
    assert ev(fake, _batch(given=('obs', 'actions', 'vf'), source_rows=0, fmt=1)) == EINVAL and b'source_rows' in err()
    assert ev(fake, _batch(given=('obs', 'actions', 'vf'), rows=9, source_rows=8, index=None)) == EINVAL


def test_the_pinned_surface_still_refuses_the_compact_record(lib):
    """dcomp_learner_grads / _evaluate take a contiguous minibatch of rows: the compact record stays DCOMP_EUNSUPPORTED there."""
    from deepcomp_amd import _lib
    fake = ctypes.c_void_p(4096)
    b = _lib.DcompPpoBatch(ctypes.sizeof(_lib.DcompPpoBatch), 1, 8, 1, 0, *([4096] * 7 + [None] * 7))
    assert lib.dcomp_learner_grads(fake, ctypes.byref(b), ctypes.byref(_hyper()), fake, None) == EUNSUPPORTED and b'compact' in lib.dcomp_last_error()
    b = _lib.DcompPpoBatch(ctypes.sizeof(_lib.DcompPpoBatch), 1, 8, 1, 0, *([4096] * 2 + [None] * 5 + [4096] + [None] * 6))
    assert lib.dcomp_learner_evaluate(fake, ctypes.byref(b), None) == EUNSUPPORTED


def test_batch_structs_are_filled_by_member_name_from_one_field_table():
    """learner.FIELDS names members the structs have (ctypes would take a misspelt keyword as a new attribute, so fill() refuses
    one), and the per-row members follow `obs` in every struct, as the headers declare them."""
    import ctypes
    import pytest
    from deepcomp_amd import _lib
    from deepcomp_amd import learner as lm
    members = lambda s: [n for n, _ in s._fields_]                              # noqa: E731
    assert set(lm.FIELDS) <= set(members(_lib.DcompPpoBatch)) and set(lm.FIELDS) <= set(members(_lib.DcompSgdBatch))
    assert set(lm.INPUTS) <= set(members(_lib.DcompGroupBatch))
    assert not (set(lm.FIELDS) - set(lm.INPUTS)) & set(members(_lib.DcompGroupBatch))      # the grouped call has no outputs, no upstream
    for struct in (_lib.DcompPpoBatch, _lib.DcompSgdBatch):                     # every pointer member but obs / index is in the table
        assert {n for n, t in struct._fields_ if t is ctypes.c_void_p} - {'obs', 'index'} == set(lm.FIELDS)
    assert lm.INPUTS == ('actions', 'old_logp', 'old_logits', 'advantages', 'value_targets', 'old_vf') and set(lm.BATCH_KEYS) == set(lm.INPUTS)
    b = lm.fill(_lib.DcompSgdBatch, obs_format=_lib.ACTOR_COMPACT, rows=3, source_rows=7, index=None, num_active=2, obs=64, ratio=128)
    assert (b.struct_size, b.obs_format, b.rows, b.source_rows, b.index, b.num_active, b.reserved, b.obs, b.ratio, b.logp) == \
        (ctypes.sizeof(_lib.DcompSgdBatch), _lib.ACTOR_COMPACT, 3, 7, None, 2, 0, 64, 128, None)
    g = lm.fill(_lib.DcompGroupBatch, obs_format=_lib.ACTOR_ROWS, source_rows=9, obs=64, index_stride=5, old_vf=128)
    assert (g.struct_size, g.source_rows, g.index_stride, g.old_vf, g.index) == (ctypes.sizeof(_lib.DcompGroupBatch), 9, 5, 128, None)
    for struct, bad in ((_lib.DcompPpoBatch, 'source_rows'), (_lib.DcompSgdBatch, 'old_logit'), (_lib.DcompGroupBatch, 'logp')):
        with pytest.raises(TypeError, match=bad):
            lm.fill(struct, **{bad: 1})
