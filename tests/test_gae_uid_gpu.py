"""GPU tests of the per-UE advantage estimator (include/dcomp_gae_uid.h, csrc/dcomp_gae_uid.hip, sampler.gae_uid): on every shape at
which one of its mechanisms can go wrong the kernel's three outputs are gae_uid_reference's, bit for bit.  In every case the outputs are
carved out of guarded buffers filled with 0xA5 (tests/guard.py: the guards stay intact, every word is written), rewards and values at
dead and unmatched positions are NaN, and the kernel runs with max_shift given and with -1 (search the whole prefix)."""
import functools

import numpy as np
import pytest

from tests import gae_uid_cases as gc
from tests import guard

pytestmark = pytest.mark.gpu


def _edges(t, e, k, n):
    """Case 4 (68 slots): departures at positions 0, 63, 64 and the last, so that a UE and its carry cross the wavefront boundary
    (slot 64 -> 63) at either end of the search window, next to envs whose first wavefront shifts as a whole or not at all."""
    table = {0: (0, 63, 64), 1: (64, n - 1, 0), 2: (63, 0, n - 1)}
    time = t % gc.HORIZON
    return table[e][0 if time == 2 else 1 + k]


# name: (T, E, U, U0, force, tile) -- tile: the trace is made for E / tile envs and repeated
CASES = {
    'u8-several-envs-per-wave': (9, 5, 8, 5, None, 1),
    'u7-odd-rows-tail-group': (9, 37, 7, 5, None, 1),
    'u64-exactly-one-wave': (9, 4, 64, 62, None, 1),
    'u68-across-the-wave-boundary': (9, 3, 68, 66, _edges, 1),
    'u1024-widest-workgroup': (4, 2, 1024, 1020, None, 1),
    'e1000-many-workgroups': (3, 1000, 8, 5, None, 1),
    't1-only-the-bootstrap': (1, 5, 8, 5, None, 1),
    'end-on-the-last-step': (6, 5, 8, 5, None, 1),
    # more envs than the grid holds at once (2 048 workgroups: 65 536 envs of 8 slots, 2 048 envs of more than 64): the env loops go round
    'e70000-narrow-kernel-strides': (3, 70000, 8, 5, None, 70),
    'e2100-wide-kernel-strides': (3, 2100, 68, 66, None, 700),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The trace, its values and the reference's outputs, computed once per case and left unchanged."""
    T, E, U, U0, force, tile = CASES[name]
    uid, uid_next, end = gc.make_trace(T, E // tile, U, U0, gc.SCHEDULE, gc.HORIZON, seed=len(name), force=force)
    uid, uid_next = np.tile(uid, (1, tile, 1)), np.tile(uid_next, (1, tile, 1))
    reward, vf, last_vf = gc.fill_values(uid, uid_next, seed=3, last=not end[T - 1])
    from deepcomp_amd.sampler import gae_uid_reference
    want = gae_uid_reference(reward, vf, uid, uid_next, last_vf, end, gc.GAMMA, gc.LAM)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and 0 < want[2].sum() <= (uid != 0).sum()
    for a in (uid, uid_next, end, reward, vf, last_vf) + want:
        if a is not None:
            a.setflags(write=False)
    return uid, uid_next, end, reward, vf, last_vf, want


def _run(torch, uid, uid_next, end, reward, vf, last_vf, max_shift):
    """The kernel on guarded, dirty outputs at odd phases; returns the three outputs as host arrays."""
    from deepcomp_amd.sampler import gae_uid
    dev = torch.device('cuda')
    T, E, U = uid.shape
    up = lambda a: None if a is None else torch.from_numpy(np.array(a.view(np.int16) if a.dtype == np.uint16 else a)).to(dev)      # noqa: E731
    adv = guard.carve(T * E * U, torch.float32, dev, phase_bytes=4)
    tgt = guard.carve(T * E * U, torch.float32, dev, phase_bytes=12)
    live = guard.carve(T * E * U, torch.uint8, dev, phase_bytes=3)
    got = gae_uid(up(reward), up(vf), up(uid), up(uid_next), up(last_vf), up(end), gc.GAMMA, gc.LAM, max_shift=max_shift,
                  out=(adv.view(T, E, U), tgt.view(T, E, U), live.view(T, E, U)))
    torch.cuda.synchronize()
    for buf, name in ((adv, 'advantages'), (tgt, 'value_targets'), (live, 'live')):
        guard.assert_guards(buf, name)
        guard.assert_all_written(buf, name)
    return [g.cpu().numpy() for g in got]


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.mark.parametrize('max_shift', [2, None], ids=['max_shift-2', 'whole-prefix'])
@pytest.mark.parametrize('name', list(CASES))
def test_kernel_is_the_reference(torch_cuda, name, max_shift):
    uid, uid_next, end, reward, vf, last_vf, want = _case(name)
    if name.startswith('u68'):                                 # the forced departures are where the docstring says
        assert [int(np.nonzero(uid[2, e] != uid_next[2, e])[0][0]) for e in range(3)] == [0, 64, 63]
        assert uid_next[3, 0, 63] == uid[3, 0, 64] and uid_next[3, 0, 64] == uid[3, 0, 66]       # pop(63), pop(64): slot 64 moves up by one, 66 by two
    got = _run(torch_cuda, uid, uid_next, end, reward, vf, last_vf, max_shift)
    for g, w, what in zip(got, want, ('advantages', 'value_targets', 'live')):
        assert np.array_equal(gc.bits(g), gc.bits(w)), f'{what} differ from gae_uid_reference'


@pytest.mark.parametrize('max_shift', [0, None], ids=['max_shift-0', 'whole-prefix'])
@pytest.mark.parametrize('U,last', [(8, True), (68, False)], ids=['u8', 'u68-end-on-the-last-step'])
def test_static_trace_is_the_plain_kernel(torch_cuda, U, last, max_shift):
    """Every row holds 1 ... U before and after every step: advantages and value targets are sampler.gae's (the device's) and
    gae_reference's, bit for bit, and every row counts."""
    torch = torch_cuda
    from deepcomp_amd.sampler import gae, gae_reference
    T, E = 7, 5
    uid, uid_next, end = gc.static_trace(T, E, U, ends=(2,) if last else (2, T - 1))
    reward, vf, last_vf = gc.fill_values(uid, uid_next, seed=4, last=last, poison=False)
    adv, tgt, live = _run(torch, uid, uid_next, end, reward, vf, last_vf, max_shift)
    want_a, want_t = gae_reference(reward, vf, last_vf, end, gc.GAMMA, gc.LAM)
    dev_a, dev_t = gae(torch.from_numpy(reward).cuda(), torch.from_numpy(vf).cuda(), None if last_vf is None else torch.from_numpy(last_vf).cuda(),
                       torch.from_numpy(end).cuda(), gc.GAMMA, gc.LAM)
    for got, ref, dev in ((adv, want_a, dev_a), (tgt, want_t, dev_t)):
        assert np.array_equal(gc.bits(got.reshape(T, -1)), gc.bits(ref)) and np.array_equal(gc.bits(got), gc.bits(dev.cpu().numpy()))
    assert live.all()


def test_gae_uid_refuses_wrong_tensors(torch_cuda):
    torch = torch_cuda
    from deepcomp_amd.sampler import gae_uid
    T, E, U = 2, 3, 4
    f = torch.zeros((T, E, U), device='cuda')
    w = torch.ones((T, E, U), dtype=torch.int16, device='cuda')
    gae_uid(f, f.clone(), w, w.clone())
    for bad in (dict(uid=w.to(torch.int32)), dict(uid_next=w[:1]), dict(reward=f[:1]), dict(vf=f.double()), dict(last_vf=f[0, 0]),
                dict(end=torch.zeros(T, device='cuda')), dict(out=(f.clone(), f.clone(), f.clone())), dict(uid=w.cpu())):
        kw = dict(dict(reward=f, vf=f.clone(), uid=w, uid_next=w.clone()), **bad)
        with pytest.raises(ValueError):
            gae_uid(**kw)
