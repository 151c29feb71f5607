"""CPU-side checks of the per-UE advantage estimator (include/dcomp_gae_uid.h, deepcomp_amd/sampler.py: gae_uid_reference): the
backward-carry specification equals "cut every UE's rows out as a trajectory of its own and run gae_reference on it" bit for bit, on a
static layout it is gae_reference, the symbol exists and is declared, the header is C99, the ctypes mirror has the C size and bad
arguments are refused on the host before the first HIP call.  No GPU compute is called here."""
import ctypes
import re

import numpy as np
import pytest

from tests import c_surface as cs
from tests import gae_uid_cases as gc
from tests.c_surface import EABI, EINVAL, lib  # noqa: F401  (lib: the fixture)

HEADER = cs.header('dcomp_gae_uid.h')

# T, E, U, U0, listed rows per env, counted rows per env (None: not stated)
TRACES = [(9, 5, 8, 5, 48, 44), (7, 3, 68, 66, 463, 460), (6, 4, 8, 5, None, None)]


@pytest.mark.parametrize('T,E,U,U0,listed,counted', TRACES, ids=['u8-t9', 'u68-t7', 'u8-on-the-boundary'])
def test_reference_equals_the_trajectories_cut_out(T, E, U, U0, listed, counted):
    from deepcomp_amd.sampler import gae_uid_reference
    uid, uid_next, end = gc.make_trace(T, E, U, U0, gc.SCHEDULE, gc.HORIZON, seed=T + U)
    on_boundary = bool(end[T - 1])
    assert on_boundary == (T % gc.HORIZON == 0)
    reward, vf, last_vf = gc.fill_values(uid, uid_next, seed=1, last=not on_boundary)
    got = gae_uid_reference(reward, vf, uid, uid_next, last_vf, end, gc.GAMMA, gc.LAM)
    want = gc.by_trajectory(reward, vf, uid, uid_next, last_vf, end, gc.GAMMA, gc.LAM)
    assert got[0].dtype == got[1].dtype == np.float32 and got[2].dtype == np.uint8 and got[0].shape == got[2].shape == (T, E, U)
    for g, w, name in zip(got, want, ('advantages', 'value_targets', 'live')):
        assert np.array_equal(gc.bits(g), gc.bits(w)), name
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()            # the NaNs of rows that do not count reached nothing
    assert (got[0][got[2] == 0] == 0).all() and (got[1][got[2] == 0] == 0).all()
    if listed is not None:
        assert int((uid != 0).sum()) == listed * E
        assert int(got[2].sum()) == counted * E
    # the values matter: another bootstrap, another result at the last step's counted rows (and only with a bootstrap)
    if not on_boundary:
        other = gae_uid_reference(reward, vf, uid, uid_next, np.where(np.isnan(last_vf), last_vf, last_vf + 1), end, gc.GAMMA, gc.LAM)
        assert (other[0][T - 1][got[2][T - 1] == 1] != got[0][T - 1][got[2][T - 1] == 1]).all()


def test_a_departure_ends_the_trajectory_before_it():
    """One env, three UEs, T = 3; UE 2 departs in step 1.  gamma = lambda = 0.5, dyadic values: exact.
       UE 2: row (0, 1) counts, row (1, 1) does not -> its trajectory is the single row t = 0 with next value 0: A = 2 - 1 = 1.
       UE 3: rows (0, 2), (1, 2) -> found at slot 1 after step 1, then row (2, 1), bootstrap last_vf[1] = 4.
         t = 2: d = (1 + 0.5 * 4) - 2 = 1, A = 1;  t = 1: reward at slot 1: d = (2 + 0.5 * 2) - 1 = 2, A = 2 + 0.25 = 2.25;
         t = 0: d = (4 + 0.5 * 1) - 0.5 = 4, A = 4 + 0.25 * 2.25 = 4.5625"""
    from deepcomp_amd.sampler import gae_uid_reference
    nan = np.nan
    uid = np.array([[[1, 2, 3]], [[1, 2, 3]], [[1, 3, 0]]], np.uint16)
    uid_next = np.array([[[1, 2, 3]], [[1, 3, 0]], [[1, 3, 0]]], np.uint16)
    reward = np.array([[[0, 2, 4]], [[0, 2, nan]], [[0, 1, nan]]], np.float32)
    vf = np.array([[[0, 1, 0.5]], [[0, nan, 1]], [[0, 2, nan]]], np.float32)
    adv, tgt, live = gae_uid_reference(reward, vf, uid, uid_next, np.array([[0, 4, nan]], np.float32), None, 0.5, 0.5)
    assert live[:, 0].tolist() == [[1, 1, 1], [1, 0, 1], [1, 1, 0]]
    assert adv[0, 0, 1] == 1.0 and adv[1, 0, 1] == 0.0 and tgt[1, 0, 1] == 0.0
    assert [adv[0, 0, 2], adv[1, 0, 2], adv[2, 0, 1]] == [4.5625, 2.25, 1.0]
    assert [tgt[0, 0, 2], tgt[1, 0, 2], tgt[2, 0, 1]] == [5.0625, 3.25, 3.0]


@pytest.mark.parametrize('last', [True, False])
def test_static_layout_is_gae_reference(last):
    from deepcomp_amd.sampler import gae_reference, gae_uid_reference
    T, E, U = 11, 3, 7
    uid, uid_next, end = gc.static_trace(T, E, U, ends=(4, 10) if not last else (4,))
    reward, vf, last_vf = gc.fill_values(uid, uid_next, seed=2, last=last, poison=False)
    adv, tgt, live = gae_uid_reference(reward, vf, uid, uid_next, last_vf, end, gc.GAMMA, gc.LAM)
    want_a, want_t = gae_reference(reward, vf, last_vf, end, gc.GAMMA, gc.LAM)
    assert np.array_equal(gc.bits(adv.reshape(T, -1)), gc.bits(want_a)) and np.array_equal(gc.bits(tgt.reshape(T, -1)), gc.bits(want_t))
    assert live.all()


def test_symbol_is_exported_and_declared(lib):
    from deepcomp_amd import _lib
    assert _lib.GAE_UID_EXPORTS == ['dcomp_gae_uid']
    assert re.search(r'\bdcomp_gae_uid\s*\(', open(HEADER).read())
    getattr(lib, 'dcomp_gae_uid')
    assert 'dcomp_gae_uid' not in _lib.EXPORTS and 'dcomp_gae_uid' not in open(cs.header('dcomp.h')).read()      # a header and a list of its own


def test_header_compiles_as_c99(tmp_path):
    cs.compiles_as_c99(tmp_path, 'gae_uid', ['#include "dcomp_gae_uid.h"\n', '#include "dcomp.h"\n#include "dcomp_gae_uid.h"\n',
                                             '#include "dcomp_gae_uid.h"\n#include "dcomp.h"\n#include "dcomp_learner.h"\n'])


def test_ctypes_mirror_matches_the_header(tmp_path):
    from deepcomp_amd import _lib
    assert cs.struct_members(HEADER, 'dcomp_gae_uid_args') == [f[0] for f in _lib.DcompGaeUidArgs._fields_]
    sizes, = cs.c_program_output(
        tmp_path, '#include <stdio.h>\n#include <stddef.h>\n#include "dcomp_gae_uid.h"\n'
                   'int f(void) {\n'
                   '    dcomp_gae_uid_args g = {0};\n'
                   '    g.struct_size = (int32_t)sizeof g; g.num_steps = 1; g.num_envs = 1; g.num_slots = 1; g.max_shift = -1; g.gamma = 0.99f; g.lambda = 1.0f;\n'
                   '    return dcomp_gae_uid(&g, 0);\n'
                   '}\n'
                   'int main(void) {\n'
                   '    printf("%zu %zu %zu\\n", sizeof(dcomp_gae_uid_args), offsetof(dcomp_gae_uid_args, reward), offsetof(dcomp_gae_uid_args, live));\n'
                   '    return 0;\n'
                   '}\n', link=['-Wl,--unresolved-symbols=ignore-all'])
    m = _lib.DcompGaeUidArgs
    assert sizes == [ctypes.sizeof(m), m.reward.offset, m.live.offset]


PTRS = ('reward', 'vf', 'uid', 'uid_next', 'last_vf', 'end', 'advantages', 'value_targets', 'live')


def _args(size=None, T=3, E=5, U=8, max_shift=-1, null=()):
    from deepcomp_amd import _lib
    return _lib.DcompGaeUidArgs(ctypes.sizeof(_lib.DcompGaeUidArgs) if size is None else size, T, E, U, max_shift, 0.99, 0.95,
                                *[None if n in null else 4096 for n in PTRS])                    # (never dereferenced)


def test_refuses_bad_arguments_on_the_host(lib):
    from deepcomp_amd import _lib
    assert lib.dcomp_gae_uid(None, None) == EINVAL and b'args' in lib.dcomp_last_error()
    for size in (0, ctypes.sizeof(_lib.DcompGaeUidArgs) - 8, ctypes.sizeof(_lib.DcompGaeUidArgs) + 8):
        assert lib.dcomp_gae_uid(ctypes.byref(_args(size=size)), None) == EABI
        assert b'dcomp_gae_uid_args' in lib.dcomp_last_error()
    cases = [(dict(null=(n,)), 'NULL') for n in PTRS if n not in ('last_vf', 'end')] + \
            [(dict(T=0), 'num_steps'), (dict(T=-1), 'num_steps'), (dict(E=0), 'num_envs'), (dict(E=-4), 'num_envs'),
             (dict(U=0), 'num_slots'), (dict(U=1025), 'num_slots'), (dict(U=-1), 'num_slots'),
             (dict(T=2 ** 20, E=2 ** 20, U=1), '2^40'), (dict(T=2 ** 10, E=2 ** 20, U=1024), '2^40'), (dict(T=1, E=2 ** 31 - 1, U=1024), '2^40')]
    for kw, word in cases:
        rc = lib.dcomp_gae_uid(ctypes.byref(_args(**kw)), None)
        assert rc == EINVAL, (kw, rc, lib.dcomp_last_error())
        assert word.encode() in lib.dcomp_last_error(), (kw, lib.dcomp_last_error())
