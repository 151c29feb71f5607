"""CPU-side checks of the per-UE policy set (include/dcomp_policy_set.h, deepcomp_amd/policy_set.py): the four entry points exist
and are declared, the ctypes mirror matches the header, the header compiles as C alone and next to dcomp.h in either order, the older
export lists keep their lengths, every argument the library can judge without dereferencing a member handle is refused on the host
before the first HIP call, and PerUELearner's row split is what the issue says.  The refusals that read the members are in
tests/test_policy_set_gpu.py.  No GPU compute is called here."""
import ctypes
import re

import pytest

from tests import c_surface as cs
from tests.c_surface import EABI, EINVAL, OK, lib  # noqa: F401  (lib: the fixture)

HEADER = cs.header('dcomp_policy_set.h')


def test_symbols_are_exported_and_declared(lib):
    from deepcomp_amd import _lib
    hdr = open(HEADER).read()
    assert _lib.SET_EXPORTS == ['dcomp_policy_set_create', 'dcomp_policy_set_destroy', 'dcomp_policy_set_actions', 'dcomp_policy_set_actions_v']
    for name in _lib.SET_EXPORTS:
        assert re.search(r'\bint %s\s*\(' % name, hdr), name
        getattr(lib, name)
        assert name not in _lib.EXPORTS and name not in _lib.LEARNER_EXPORTS and name not in _lib.SGD_EXPORTS
    assert sorted(re.findall(r'\bint (dcomp_\w+)\s*\(', hdr)) == sorted(_lib.SET_EXPORTS)
    # the surfaces the existing tests pin are as they were
    assert len(_lib.EXPORTS) == 42 and len(_lib.LEARNER_EXPORTS) == 7 and len(_lib.SGD_EXPORTS) == 2
    for other in ('dcomp.h', 'dcomp_types.h', 'dcomp_learner.h', 'dcomp_learner_indexed.h'):
        assert not re.search(r'dcomp_policy_set', open(cs.header(other)).read()), other


def test_ctypes_mirror_matches_the_header(tmp_path):
    """Member names from the header text, size and offsets from a C program compiled against it (C99, pedantic)."""
    from deepcomp_amd import _lib
    members = cs.struct_members(HEADER, 'dcomp_policy_set_cfg')
    assert members == [f[0] for f in _lib.DcompPolicySetCfg._fields_], members
    sizes, = cs.c_program_output(                                                      # (compiled alone first)
        tmp_path, '#include <stdio.h>\n#include <stddef.h>\n#include "dcomp_policy_set.h"\n'
                   'int main(void) {\n'
                   '    printf("%zu %zu %zu %zu\\n", sizeof(dcomp_policy_set_cfg), offsetof(dcomp_policy_set_cfg, num_policies),\n'
                   '           offsetof(dcomp_policy_set_cfg, members), offsetof(dcomp_policy_set_cfg, slot_policy));\n'
                   '    return DCOMP_EABI == -7 ? 0 : 1;\n'
                   '}\n')
    main = ('int main(void) { dcomp_policy_set_cfg c; c.struct_size = (int32_t)sizeof c; '
            'return DCOMP_EABI == -7 && DCOMP_ACTOR_COMPACT == 1 && c.struct_size > 0 ? 0 : 1; }\n')
    cs.compiles_as_c99(tmp_path, 'both', [text + main for text in (                    # with dcomp.h, either order
        '#include "dcomp.h"\n#include "dcomp_policy_set.h"\n', '#include "dcomp_policy_set.h"\n#include "dcomp.h"\n')])
    S = _lib.DcompPolicySetCfg
    assert sizes == [ctypes.sizeof(S), S.num_policies.offset, S.members.offset, S.slot_policy.offset]


def _cfg(num_policies=2, members='fake', size=None, slots=None):
    from deepcomp_amd import _lib
    keep = []
    if members == 'fake':
        members = [4096] * max(num_policies, 1)                                        # (never dereferenced by the checks under test)
    arr = None
    if members is not None:
        arr = (ctypes.c_void_p * len(members))(*members)
        keep.append(arr)
    cfg = _lib.DcompPolicySetCfg(ctypes.sizeof(_lib.DcompPolicySetCfg) if size is None else size, num_policies, arr, slots)
    cfg._keep = keep
    return cfg


def test_create_refuses_what_needs_no_member_on_the_host(lib):
    from deepcomp_amd import _lib
    err = lib.dcomp_last_error
    out = ctypes.c_void_p(1234)
    create = lambda c, o=out: lib.dcomp_policy_set_create(ctypes.byref(c) if c is not None else None, ctypes.byref(o) if o is not None else None)      # noqa: E731
    assert create(None) == EINVAL and b'cfg' in err()
    assert out.value is None                                                           # *out is cleared on every failure
    assert lib.dcomp_policy_set_create(ctypes.byref(_cfg()), None) == EINVAL and b'out' in err()
    for size in (0, ctypes.sizeof(_lib.DcompPolicySetCfg) - 8, ctypes.sizeof(_lib.DcompPolicySetCfg) + 8):
        assert create(_cfg(size=size)) == EABI and b'dcomp_policy_set_cfg' in err()
    assert create(_cfg(members=None)) == EINVAL and b'members' in err()
    for P in (0, -1, _lib.MAX_UE + 1):
        assert create(_cfg(num_policies=P)) == EINVAL and b'num_policies' in err(), P
    assert create(_cfg(num_policies=3, members=[4096, None, 4096])) == EINVAL and b'member 1 is NULL' in err()
    assert create(_cfg(num_policies=1, members=[None])) == EINVAL and b'member 0 is NULL' in err()
    assert out.value is None
    assert lib.dcomp_policy_set_destroy(None) == OK


def test_actions_refuse_a_null_handle_or_run_and_a_wrong_struct_size(lib):
    """With a fake set handle that is never dereferenced: these checks come before the set is read."""
    from deepcomp_amd import _lib
    err = lib.dcomp_last_error
    fake = ctypes.c_void_p(4096)
    run = lambda size=None: _lib.DcompActorRun(ctypes.sizeof(_lib.DcompActorRun) if size is None else size, 0, 4, 2, 0, 0, 0, 0, None, None)      # noqa: E731
    calls = {b'dcomp_policy_set_actions:': lambda s, r: lib.dcomp_policy_set_actions(s, ctypes.byref(r) if r is not None else None, fake, fake, None),
             b'dcomp_policy_set_actions_v:': lambda s, r: lib.dcomp_policy_set_actions_v(s, ctypes.byref(r) if r is not None else None, fake, fake, fake, None)}
    for name, call in calls.items():
        assert call(None, run()) == EINVAL and name in err() and b'NULL' in err()
        assert call(fake, None) == EINVAL and name in err() and b'NULL' in err()
        for size in (0, ctypes.sizeof(_lib.DcompActorRun) - 8, ctypes.sizeof(_lib.DcompActorRun) + 8):
            assert call(fake, run(size)) == EABI and name in err() and b'dcomp_actor_run' in err()


def test_row_split_of_the_per_ue_learner():
    """U = 5, slot_policy = [0, 1, 1, 0, 1], 3 x 7 envs: the rows of policy p are exactly the flat rows whose row % U maps to p."""
    from deepcomp_amd.policy_set import default_slot_policy, policy_rows
    U, sp, T, E = 5, [0, 1, 1, 0, 1], 3, 7
    N = T * E * U
    rows = policy_rows(N, U, sp, 2)
    assert len(rows) == 2
    for p in range(2):
        assert rows[p].tolist() == [s for s in range(N) if sp[s % U] == p]
    a, b = set(rows[0].tolist()), set(rows[1].tolist())
    assert not (a & b) and a | b == set(range(N))
    assert len(a) == 2 * T * E and len(b) == 3 * T * E
    assert default_slot_policy(5, 2) == [0, 1, 0, 1, 0] and default_slot_policy(3, 3) == [0, 1, 2]
    third = policy_rows(N, U, sp, 3)                                                   # a policy no slot maps to has no rows
    assert third[2].numel() == 0 and third[0].tolist() == rows[0].tolist()
    with pytest.raises(ValueError):
        policy_rows(N, U, sp[:-1], 2)
