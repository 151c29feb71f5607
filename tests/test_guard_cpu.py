"""The guard-band checker checked (round 17): tests/guard.py on CPU tensors, the way test_conn_order_cpu.py checks assert_conn_order -- a
checker that cannot fail proves nothing on the GPU.  Plus what the rows of tests/guard_cases.py claim about themselves."""
import re

import numpy as np
import pytest
import torch

from tests import guard
from tests import guard_cases as gc


@pytest.mark.parametrize('dtype', [torch.float32, torch.int32, torch.int16, torch.uint8, torch.float64])
def test_carve_layout(dtype):
    n = 37
    for phase in ((0, 4, 8, 12) if dtype in (torch.float32, torch.int32) else (0,)):
        p = guard.carve(n, dtype, 'cpu', phase_bytes=phase)
        raw, start, nbytes = p._guard
        assert p.numel() == n and p.dtype == dtype and p.is_contiguous()
        assert p.data_ptr() % 16 == phase, 'the payload starts at the requested phase of a 16-byte line'
        assert start == guard.GUARD_BYTES + phase and p.data_ptr() == raw.data_ptr() + start
        assert nbytes == n * p.element_size() and raw.numel() - start - nbytes >= guard.GUARD_BYTES
        assert bool((raw == guard.FILL).all()), 'guards AND payload hold the fill pattern'
        guard.assert_guards(p, 'fresh')
        with pytest.raises(AssertionError, match='first unwritten at byte offset 0,'):
            guard.assert_all_written(p, 'fresh')
    if dtype == torch.float32:
        assert guard.bits(p)[0] == np.int32(np.uint32(0xA5A5A5A5).astype(np.int32)) and np.isfinite(p[0].item()) and abs(p[0].item()) < 1e-15


def test_a_float_payload_cannot_start_off_its_own_alignment():
    with pytest.raises(AssertionError):
        guard.carve(4, torch.float64, 'cpu', phase_bytes=4)


@pytest.mark.parametrize('phase', [0, 4, 8, 12])
def test_one_byte_outside_the_payload_is_reported_with_side_and_offset(phase):
    n = 21
    for side, off in (('before', -1), ('after', 4 * n), ('before', -guard.GUARD_BYTES - phase), ('after', 4 * n + guard.GUARD_BYTES - 1)):
        p = guard.carve(n, torch.float32, 'cpu', phase_bytes=phase)
        p.zero_()
        raw, start, nbytes = p._guard
        raw[start + off] = 0
        with pytest.raises(AssertionError, match=re.escape(f'guard {side} the payload touched: bytes {off} .. {off} relative to the payload '
                                                           f'(its length is {4 * n}), 1 bytes changed')):
            guard.assert_guards(p, 'poke')
        guard.assert_all_written(p, 'poke')             # the payload itself is fine
    # an overrun of one row: starts exactly at the payload's end
    p = guard.carve(n, torch.float32, 'cpu', phase_bytes=phase)
    raw, start, nbytes = p._guard
    raw[start + nbytes:start + nbytes + 40] = 1
    with pytest.raises(AssertionError, match=re.escape(f'after the payload touched: bytes {nbytes} .. {nbytes + 39} ') + '.*, 40 bytes changed'):
        guard.assert_guards(p, 'overrun')


@pytest.mark.parametrize('dtype,unit', [(torch.float32, 4), (torch.int32, 4), (torch.int16, 2), (torch.uint8, 1), (torch.float64, 4)])
def test_one_unwritten_unit_is_reported(dtype, unit):
    n = 24
    units = n * torch.empty(0, dtype=dtype).element_size() // unit
    for k in (0, units // 2, units - 1):
        p = guard.carve(n, dtype, 'cpu')
        p.zero_()
        raw, start, nbytes = p._guard
        raw[start + k * unit:start + (k + 1) * unit] = guard.FILL
        with pytest.raises(AssertionError, match=re.escape(f'1 of {units} {unit}-byte units never written; first unwritten at byte offset {k * unit},')):
            guard.assert_all_written(p, 'hole')
        guard.assert_all_written(p, 'hole', allow=[k])
        with pytest.raises(AssertionError):
            guard.assert_all_written(p, 'hole', allow=[k + 1])
        guard.assert_guards(p, 'hole')


def test_a_word_is_unwritten_only_if_all_its_bytes_are():
    p = guard.carve(4, torch.float32, 'cpu')
    p.zero_()
    raw, start, _ = p._guard
    raw[start + 5] = guard.FILL                          # one byte of word 1 happens to be 0xA5: written
    raw[start + 10:start + 14] = guard.FILL              # four pattern bytes that straddle words 2 and 3: both written
    guard.assert_all_written(p, 'coincidence')


def test_legitimate_zeros_pass_and_refill_brings_the_pattern_back():
    p = guard.carve(30, torch.float32, 'cpu', phase_bytes=8)
    p.zero_()
    guard.assert_all_written(p, 'zeros')
    guard.assert_guards(p, 'zeros')
    assert not guard.bits(p).any()
    guard.refill(p)
    assert len(guard.unwritten(p)[0]) == 30
    guard.assert_guards(p, 'refilled')


def test_a_view_does_not_pass_for_a_carved_buffer():
    p = guard.carve(8, torch.float32, 'cpu')
    with pytest.raises(AssertionError, match='not a tensor carve'):
        guard.assert_guards(p.view(2, 4), 'view')


# ---------------------------------------------------------------------------------------------------- the case table
def test_case_table_covers_what_it_must():
    names = {c.name for c in gc.CASES}
    assert len(names) == len(gc.CASES)
    by = {c.name: c for c in gc.CASES}
    assert (by['narrow_32x10'].kind, by['narrow_16x32'].kind, by['narrow_10x5'].kind) == ('multi', 'central', 'central')
    assert by['tight_10x5'].env == {'DCOMP_TIGHT': '1'} and by['tight_5x32'].kind == 'central'
    assert by['wide_128x32'].env == {} and by['wide_128x32_pad24000'].env == {'DCOMP_WIDE_PAD_LDS': '24000'}
    assert {c.env.get('DCOMP_BIG_ROW_X4') for c in gc.CASES if 'row_x4' in c.name} == {'0', '1'}
    assert all(c.B > 32 and c.kind == 'multi' for c in gc.CASES if 'row_x4' in c.name)
    assert {(c.U, c.B) for c in gc.CASES if c.mode == 'dyn'} == {(6, 24), (6, 40)}
    assert any(c.mode == 'rollout' and c.tag is None for c in gc.CASES) and any(c.mode == 'rollout' and 'DCOMP_TIGHT' in c.env for c in gc.CASES)
    assert any(c.mode == 'rollout' and c.tag == 'big_kernel' for c in gc.CASES) and any(c.mode == 'rollout_steps' and 'DCOMP_NO_FUSED_BIG' in c.env for c in gc.CASES)
    assert any(c.sharing == 'maxcap' and 'max-cap' in gc.sharing_list(c) for c in gc.CASES)
    assert gc.PHASES == (0, 4, 8, 12)
    assert not gc.ALLOW, 'no buffer has a documented unwritten word'


@pytest.mark.parametrize('case', gc.CASES, ids=gc.IDS)
def test_case_shapes_leave_a_partial_wave_and_a_ragged_end(case):
    assert 1 <= case.E <= 7 and 3 <= gc.steps(case) <= 5
    M = gc.slots(case)
    assert case.lanes == (M if 'DCOMP_TIGHT' in case.env else max(1 << (M - 1).bit_length(), 1))
    if case.tag == 'big_kernel':
        assert case.epb == max(64, case.lanes) // case.lanes
    elif 'DCOMP_TIGHT' in case.env:
        assert case.epb == 4 * (64 // M)
    else:
        assert case.epb == 256 // case.lanes
    assert gc.partly_filled(case), 'the last wavefront / workgroup must be partly filled'
    assert gc.ragged_end(case) == gc.shape_allows_ragged_end(case), 'E must leave the end of obs inside a 16-byte line wherever some E can'
    if case.mode == 'dyn':
        assert M > case.U and gc.steps(case) > min(t for t, n in gc.ARRIVAL.items() if n < 0), 'a slot must die inside the checked steps'
