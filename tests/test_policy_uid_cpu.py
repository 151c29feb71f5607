"""CPU-side checks of the policy set keyed by UE id (include/dcomp_policy_set_uid.h, deepcomp_amd.policy_set.PerIdActor /
policy_rows_by_id): the entry point exists and is declared, the header compiles as C alone and next to the others, the older surfaces
are as they were, what the library can judge without dereferencing the set handle is refused on the host before the first HIP call,
and the row split by id is, on hand-written traces, what the cut-out trajectories of tests/gae_uid_cases.py say.  The three checks the
entry adds behind actor_launch's read the set's first member, so they are held with a real set in tests/test_policy_uid_gpu.py, like
every refusal of dcomp_policy_set.h that reads a member.  No GPU compute is called here."""
import ctypes
import re

import numpy as np
import pytest

from tests import c_surface as cs
from tests import gae_uid_cases as gc
from tests import policy_uid_cases as pc
from tests.c_surface import EABI, EINVAL, lib  # noqa: F401  (lib: the fixture)

HEADER = cs.header('dcomp_policy_set_uid.h')


def test_symbol_is_exported_and_declared(lib):
    from deepcomp_amd import _lib
    hdr = open(HEADER).read()
    assert _lib.SET_UID_EXPORTS == ['dcomp_policy_set_actions_uid']
    assert re.findall(r'\bint (dcomp_\w+)\s*\(', hdr) == _lib.SET_UID_EXPORTS
    fn = lib.dcomp_policy_set_actions_uid
    assert len(fn.argtypes) == 7                                                       # set, run, obs, uid, action, vf, stream
    decl = re.search(r'int dcomp_policy_set_actions_uid\s*\((.*?)\);', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S), flags=re.S).group(1)
    assert [re.split(r'[\s*]+', a.strip())[-1] for a in decl.split(',')] == ['s', 'run', 'obs', 'uid', 'action', 'vf', 'stream']
    # the surfaces the existing tests pin are as they were, and the set's own header only points here
    assert len(_lib.EXPORTS) == 42 and len(_lib.SET_EXPORTS) == 4 and 'dcomp_policy_set_actions_uid' not in _lib.EXPORTS + _lib.SET_EXPORTS
    assert 'dcomp_policy_set_uid.h' in open(cs.header('dcomp_policy_set.h')).read()
    for other in ('dcomp.h', 'dcomp_types.h', 'dcomp_learner.h', 'dcomp_gae_uid.h'):
        assert 'dcomp_policy_set_actions_uid' not in open(cs.header(other)).read(), other


def test_header_parses_alone_and_next_to_the_others(tmp_path):
    """C99, pedantic, warnings are errors; struct sizes as in the headers it builds on: it adds no struct of its own."""
    from deepcomp_amd import _lib
    sizes, = cs.c_program_output(
        tmp_path, '#include <stdio.h>\n#include <stddef.h>\n#include "dcomp_policy_set_uid.h"\n#include "dcomp.h"\n'
                   'int main(void) {\n'
                   '    int (*fn)(dcomp_policy_set *, const dcomp_actor_run *, const void *, const uint16_t *, uint8_t *, float *, void *) = 0;\n'
                   '    printf("%zu %zu\\n", sizeof(dcomp_actor_run), sizeof(dcomp_policy_set_cfg));\n'
                   '    return fn == 0 && DCOMP_EABI == -7 ? 0 : 1;\n'
                   '}\n')
    assert sizes == [ctypes.sizeof(_lib.DcompActorRun), ctypes.sizeof(_lib.DcompPolicySetCfg)]
    main = 'int main(void) { return DCOMP_EABI == -7 && DCOMP_ACTOR_COMPACT == 1 ? 0 : 1; }\n'
    cs.compiles_as_c99(tmp_path, 'uid', [text + main for text in (
        '#include "dcomp.h"\n#include "dcomp_policy_set_uid.h"\n', '#include "dcomp_policy_set_uid.h"\n#include "dcomp.h"\n',
        '#include "dcomp_policy_set.h"\n#include "dcomp_gae_uid.h"\n#include "dcomp_policy_set_uid.h"\n#include "dcomp.h"\n')])


def test_a_null_handle_or_run_and_a_wrong_struct_size_are_refused_on_the_host(lib):
    """With a fake set handle that is never dereferenced: these checks come before the set is read, so no HIP call can have been made."""
    from deepcomp_amd import _lib
    err = lib.dcomp_last_error
    fake = ctypes.c_void_p(4096)
    run = lambda size=None: _lib.DcompActorRun(ctypes.sizeof(_lib.DcompActorRun) if size is None else size, 0, 4, 2, 0, 0, 0, 0, None, None)      # noqa: E731
    call = lambda s, r: lib.dcomp_policy_set_actions_uid(s, ctypes.byref(r) if r is not None else None, fake, fake, fake, fake, None)      # noqa: E731
    name = b'dcomp_policy_set_actions_uid:'
    assert call(None, run()) == EINVAL and name in err() and b'NULL' in err()
    assert call(fake, None) == EINVAL and name in err() and b'NULL' in err()
    for size in (0, ctypes.sizeof(_lib.DcompActorRun) - 8, ctypes.sizeof(_lib.DcompActorRun) + 8):
        assert call(fake, run(size)) == EABI and name in err() and b'dcomp_actor_run' in err()


@pytest.mark.parametrize('name', sorted(pc.TRACES))
def test_row_split_reference_on_hand_written_traces(name):
    from deepcomp_amd.policy_set import policy_rows_by_id_reference
    from deepcomp_amd.sampler import gae_uid_reference
    make, P = pc.TRACES[name]
    uid, uid_next, end = make()
    T, E, U = uid.shape
    reward, vf, last_vf = gc.fill_values(uid, uid_next, seed=3, last=not end[-1], poison=False)
    live = gae_uid_reference(reward, vf, uid, uid_next, last_vf, end)[2]
    rows = policy_rows_by_id_reference({'uid': uid.view(np.int16), 'live': live}, P)
    want = pc.check_split(rows, uid, uid_next, end, P)
    if name == 'a':
        # id 9 never appears, 8' arrives in the last step and never acts; every other id has rows
        assert P == 9 and rows[8].size == 0 and rows[7].size == 0 and all(r.size for r in rows[:7])
        # two departures in step 3 of env 0 (6' and 5): neither row counts, and the dead tail never does
        at = lambda t, e, s: (t * E + e) * U + s      # noqa: E731
        every = set(np.concatenate(rows).tolist())
        assert at(3, 0, 4) not in every and at(3, 0, 5) not in every and at(2, 0, 6) not in every and at(3, 0, 3) in every
        assert not any(at(t, e, 6) in every for t in (0, 3, 4, 5) for e in range(E))
        # 5 leaves env 0 in step 3 and 5' arrives in step 5: the same policy, and the arrival has no counted row before it has acted
        assert rows[4].tolist() == [at(0, 0, 4), at(0, 1, 4), at(1, 0, 4), at(1, 1, 4), at(2, 0, 4), at(2, 1, 4), at(3, 1, 3), at(4, 1, 1), at(5, 1, 1)]
    assert sum(w.size for w in want) == int(live.sum())


@pytest.mark.parametrize('name', sorted(pc.TRACES))
def test_row_split_on_cpu_tensors_is_the_reference(name):
    import torch
    from deepcomp_amd.policy_set import policy_rows_by_id, policy_rows_by_id_reference
    from deepcomp_amd.sampler import gae_uid_reference
    make, P = pc.TRACES[name]
    uid, uid_next, end = make()
    T, E, U = uid.shape
    zeros = np.zeros((T, E, U), np.float32)
    live = gae_uid_reference(zeros, zeros, uid, uid_next, None, end)[2]
    batch = {'uid': torch.from_numpy(uid.view(np.int16).copy()), 'live': torch.from_numpy(live.reshape(T, E * U).copy())}
    for policies in (P, 4, 1):                                                         # fewer policies than ids: rows of the others are in no split
        got = policy_rows_by_id(batch, policies)
        want = policy_rows_by_id_reference(batch, policies)
        assert len(got) == len(want) == policies
        for g, w in zip(got, want):
            assert g.dtype == torch.int64 and g.is_contiguous() or g.numel() == 0
            assert np.array_equal(g.numpy(), w)
    with pytest.raises(ValueError):
        policy_rows_by_id({'uid': batch['uid'][:-1], 'live': batch['live']}, P)


def test_uid_fields_on_tensors_are_the_numpy_fields():
    import torch
    from deepcomp_amd.tape import uid_fields
    words = np.array([0, 1, 5, 0x8005, 0xFFFF, 0x8000, 0x7FFF], dtype=np.uint16)
    ids, born = uid_fields(words)
    tid, tborn = uid_fields(torch.from_numpy(words.view(np.int16).copy()))
    assert tid.dtype == torch.int64 and tborn.dtype == torch.bool
    assert tid.tolist() == ids.tolist() == [0, 1, 5, 5, 0x7FFF, 0, 0x7FFF] and tborn.tolist() == born.tolist()
