"""CPU-side checks of the accumulated and data-parallel gradients (include/dcomp_learner_accum.h, deepcomp_amd/learner.py,
deepcomp_amd/dp_learner.py): the four entry points exist and are declared, the header compiles as C, every argument the library can
judge without its handle is refused on the host before the first HIP call (with a fake handle that is never dereferenced) under the
function's own name, micro_rows is validated against the library's chunk unit, and the two phases of a data-parallel update that need
no learner -- the global advantage standardisation and the shard agreement -- run under two and three gloo ranks on CPU tensors.
What needs a handle or the device is in tests/test_learner_accum_gpu.py.  No GPU compute is called here."""
import ctypes
import math
import os
import re

import pytest
import torch

from tests import c_surface as cs
from tests.c_surface import EABI, EINVAL, EUNSUPPORTED, lib  # noqa: F401  (lib: the fixture)
from tests.c_surface import LOSS_INPUTS as _LOSS_INPUTS
from tests.c_surface import ppo_batch as _ppo
from tests.c_surface import ppo_hyper as _hyper
from tests.c_surface import sgd_batch as _sgd
from tests.env_support import free_port as _free_port

HEADER = cs.header('dcomp_learner_accum.h')
NAMES = ['dcomp_learner_flat_size', 'dcomp_learner_accumulate', 'dcomp_sgd_accumulate', 'dcomp_learner_accum_finish']


def test_symbols_are_exported_and_declared(lib, tmp_path):
    from deepcomp_amd import _lib
    hdr = open(HEADER).read()
    assert _lib.ACCUM_EXPORTS == NAMES
    for name in NAMES:
        assert re.search(r'\bint %s\s*\(' % name, hdr), name
        getattr(lib, name)
        assert not any(name in lst for lst in (_lib.EXPORTS, _lib.LEARNER_EXPORTS, _lib.SGD_EXPORTS, _lib.GROUP_EXPORTS))
    assert sorted(re.findall(r'\bint (dcomp_\w+)\s*\(', hdr)) == sorted(NAMES)
    assert re.search(r'#define DCOMP_ACCUM_SUMS\s+8\b', hdr) and _lib.ACCUM_SUMS == 8
    # the surfaces the existing tests pin are as they were
    assert len(_lib.LEARNER_EXPORTS) == 7 and len(_lib.EXPORTS) == 42 and len(_lib.SGD_EXPORTS) == 2 and len(_lib.GROUP_EXPORTS) == 4
    for other in ('dcomp_learner.h', 'dcomp_learner_indexed.h', 'dcomp_learner_group.h'):
        assert not re.search(r'_accum|_flat_size', open(cs.header(other)).read())
    # the header as C99, alone and behind the others
    main = 'int main(void) { return DCOMP_ACCUM_SUMS == 8 && DCOMP_EABI == -7 ? 0 : 1; }\n'
    cs.compiles_as_c99(tmp_path, 'accum', [text + main for text in (
        '#include "dcomp_learner_accum.h"\n', '#include "dcomp.h"\n#include "dcomp_learner_group.h"\n#include "dcomp_learner_accum.h"\n')])


@pytest.mark.parametrize('surface', ['ppo', 'sgd'])
def test_accumulate_refuses_bad_arguments_on_the_host(lib, surface):
    from deepcomp_amd import _lib
    fake = ctypes.c_void_p(4096)
    err = lib.dcomp_last_error
    fn, batch = (lib.dcomp_learner_accumulate, _ppo) if surface == 'ppo' else (lib.dcomp_sgd_accumulate, _sgd)
    name = fn.__name__.encode()
    struct = b'dcomp_ppo_batch' if surface == 'ppo' else b'dcomp_sgd_batch'
    own = ctypes.sizeof(_lib.DcompPpoBatch if surface == 'ppo' else _lib.DcompSgdBatch)
    g = lambda l, b, h, acc, sums: fn(l, ctypes.byref(b) if b is not None else None, ctypes.byref(h) if h is not None else None, acc, sums, None)      # noqa: E731
    assert g(None, batch(), _hyper(), fake, fake) == EINVAL and b'handle' in err() and name in err()
    assert g(fake, None, _hyper(), fake, fake) == EINVAL and name in err()
    assert g(fake, batch(), _hyper(), None, fake) == EINVAL and b'acc_dev' in err() and name in err()
    assert g(fake, batch(), _hyper(), fake, None) == EINVAL and b'sums_dev' in err() and name in err()
    assert g(fake, batch(), None, fake, fake) == EINVAL and b'hyper' in err() and name in err()
    for size in (0, own - 8, own + 8):
        assert g(fake, batch(size=size), _hyper(), fake, fake) == EABI and struct in err() and name in err()
    assert g(fake, batch(), _hyper(size=8), fake, fake) == EABI and b'dcomp_ppo_hyper' in err() and name in err()
    # upstream gradients are plain sums already: refused, both or one of them
    for up in (('dlogits', 'dvalue'), ('dlogits',), ('dvalue',)):
        assert g(fake, batch(given=('obs',) + up), _hyper(), fake, fake) == EINVAL and b'upstream' in err() and name in err()
        assert g(fake, batch(given=_LOSS_INPUTS + up), _hyper(), fake, fake) == EINVAL and b'upstream' in err()
    # every check of the grads calls, through the same learner_check
    assert g(fake, batch(), _hyper(clip=-0.1), fake, fake) == EINVAL and b'clip_param' in err() and name in err()
    assert g(fake, batch(), _hyper(vf_clip=float('nan')), fake, fake) == EINVAL
    assert g(fake, batch(fmt=2), _hyper(), fake, fake) == EINVAL and b'obs_format' in err()
    assert g(fake, batch(given=_LOSS_INPUTS[1:]), _hyper(), fake, fake) == EINVAL and b'obs' in err()
    for missing in _LOSS_INPUTS[1:]:
        assert g(fake, batch(given=[n for n in _LOSS_INPUTS if n != missing]), _hyper(), fake, fake) == EINVAL and b'NULL' in err(), missing
    assert g(fake, batch(rows=0), _hyper(), fake, fake) == EINVAL and b'rows' in err() and name in err()
    if surface == 'ppo':
        assert g(fake, batch(fmt=1), _hyper(), fake, fake) == EUNSUPPORTED and b'compact' in err()
    else:
        assert g(fake, batch(source_rows=0), _hyper(), fake, fake) == EINVAL and b'source_rows' in err()
        assert g(fake, batch(source_rows=2 ** 31, fmt=1), _hyper(), fake, fake) == EINVAL and b'2^31' in err()
        assert g(fake, batch(rows=65, source_rows=64, index=None), _hyper(), fake, fake) == EINVAL and b'index' in err()


def test_finish_and_flat_size_refuse_bad_arguments_on_the_host(lib):
    fake = ctypes.c_void_p(4096)
    err = lib.dcomp_last_error
    name = b'dcomp_learner_accum_finish'
    f = lambda l, acc, sums, h, clip: lib.dcomp_learner_accum_finish(l, acc, sums, ctypes.byref(h) if h is not None else None, clip, None, None, None)      # noqa: E731
    assert f(None, fake, fake, _hyper(), 0.0) == EINVAL and b'handle' in err() and name in err()
    assert f(fake, None, fake, _hyper(), 0.0) == EINVAL and b'acc_dev' in err() and name in err()
    assert f(fake, fake, None, _hyper(), 0.0) == EINVAL and b'sums_dev' in err() and name in err()
    assert f(fake, fake, fake, None, 0.0) == EINVAL and b'hyper' in err() and name in err()
    assert f(fake, fake, fake, _hyper(size=4), 0.0) == EABI and b'dcomp_ppo_hyper' in err() and name in err()
    for clip in (-1.0, -1e-30, float('nan'), float('-inf')):
        assert f(fake, fake, fake, _hyper(), clip) == EINVAL and b'grad_clip' in err() and name in err(), clip
    n = ctypes.c_int64(7)
    assert lib.dcomp_learner_flat_size(None, ctypes.byref(n)) == EINVAL and b'dcomp_learner_flat_size' in err()
    assert lib.dcomp_learner_flat_size(fake, None) == EINVAL and n.value == 7


def test_micro_rows_validation(lib):
    from deepcomp_amd import learner as lm
    from tests import fcnet_cases as fc
    unit = lm.chunk_unit()
    assert unit == fc.CHUNK_UNIT == 2048
    assert lm.check_micro_rows(unit, 4 * unit) == unit and lm.check_micro_rows(4 * unit, 4 * unit) == 4 * unit
    for bad in (0, -unit, 1, unit - 1, unit + 1, 3 * unit // 2, 2.5 * unit, True):
        with pytest.raises(ValueError, match='multiple'):
            lm.check_micro_rows(bad, 1 << 20)
    with pytest.raises(ValueError, match='max_rows'):
        lm.check_micro_rows(2 * unit, 2 * unit - 1)


def test_clip_reference_is_clip_grad_norm():
    """clip_reference against torch.nn.utils.clip_grad_norm_ on the same float32 gradient, above and below the clip."""
    from deepcomp_amd import learner as lm
    import numpy as np
    g = torch.randn(1000, generator=torch.Generator().manual_seed(3)).numpy() * 0.1
    norm = math.sqrt(float((g.astype(np.float64) ** 2).sum()))
    for clip in (0.5 * norm, 2.0 * norm):
        p = torch.nn.Parameter(torch.zeros(1000))
        p.grad = torch.from_numpy(g.copy())
        total = torch.nn.utils.clip_grad_norm_([p], clip)
        got, got_norm = lm.clip_reference(g, clip)
        assert abs(float(got_norm) - float(total)) <= 2e-7 * norm
        assert np.abs(got - p.grad.numpy()).max() <= 2.0 ** -22 * np.abs(g).max()
        assert np.array_equal(got, g) == (clip > norm)
    same, n0 = lm.clip_reference(g, None)
    assert np.array_equal(same, g) and abs(float(n0) - norm) <= 1e-7 * norm


# ---------------------------------------------------------------------------------------------- gloo ranks on CPU tensors
def _dp_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from deepcomp_amd import dp_learner as dp
        reduce = dp.group_reduce(dist.group.WORLD)
        ok = True
        # the global standardisation: every rank its own slice of one batch, scales that differ by rank
        n = 257
        whole = torch.randn(world * n, generator=torch.Generator().manual_seed(11)) * torch.arange(1, world * n + 1).remainder(7).add(1) + 3.0
        mine = whole[rank * n:(rank + 1) * n].clone()
        got = dp.drive(dp.standardize_phases(mine), reduce)
        w64 = whole.double()
        mean = float(w64.sum()) / (world * n)
        std = math.sqrt(max(0.0, float((w64 * w64).sum()) / (world * n) - mean * mean))
        want = ((mine.double() - mean) / max(1e-4, std)).float()
        ok &= got.dtype == torch.float32 and got.shape == mine.shape
        # the reduced moments are sums of per-rank sums: float64 re-association, ~2^-50 relative, which can move the final rounding to
        # float32 by one ulp at the most -- 2^-21 for a standardised value below 8
        ok &= float(want.abs().max()) < 8.0 and float((got - want).abs().max()) <= 2.0 ** -21
        every = [torch.zeros_like(got) for _ in range(world)]
        dist.all_gather(every, got)
        cat = torch.cat(every).double()
        ok &= abs(float(cat.mean())) < 1e-6 and abs(float(cat.std(unbiased=False)) - 1.0) < 1e-6
        # a constant batch: the 1e-4 floor, not a division by zero
        flat = dp.drive(dp.standardize_phases(torch.full((5,), 2.5)), reduce)
        ok &= bool((flat == 0).all())
        # the shard agreement: equal shards pass and give the rank's share; unequal shards and an indivisible minibatch raise on EVERY rank
        ok &= dp.drive(dp.shard_agreement_phases(4096, None, world), reduce) == 4096
        ok &= dp.drive(dp.shard_agreement_phases(4096, 2048 * world, world), reduce) == 2048
        ok &= dp.drive(dp.shard_agreement_phases(100, 4096 * world, world), reduce) == 100
        for rows, mb, word in ((4096 + (rank == world - 1), None, 'different numbers of rows'), (4096, 2048 * world + 1, 'multiple of the world size'),
                               (4096, 0, 'multiple of the world size')):
            try:
                dp.drive(dp.shard_agreement_phases(rows, mb, world), reduce)
                ok = False
            except ValueError as e:
                ok &= word in str(e)
        ret[rank] = bool(ok)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_standardisation_and_shard_agreement_under_gloo(world):
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    mp.spawn(_dp_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert dict(ret) == {r: True for r in range(world)}


def test_world_one_touches_no_process_group():
    """No group: every reduction is the identity, the phases still run."""
    from deepcomp_amd import dp_learner as dp
    reduce = dp.group_reduce(None)
    a = torch.arange(10, dtype=torch.float32)
    got = dp.drive(dp.standardize_phases(a), reduce)
    d = a.double()
    want = ((d - d.mean()) / d.std(unbiased=False)).float()
    assert float((got - want).abs().max()) <= 2.0 ** -23                  # (float64 both, rounded once: one float32 ulp of a value below 2)
    assert dp.drive(dp.shard_agreement_phases(77, None, 1), reduce) == 77
    assert not torch.distributed.is_initialized()
