"""Guard bands and fill patterns around the buffers the env kernels write (round 17).

The parity tests compare the valid region of an output with the oracle, out of buffers the Python class sized, zeroed and aligned itself.
That leaves three things unseen: a store past the end of an output or of a state array (it lands in allocator slack), a word that was
skipped where the zero that was there happens to be right, and a store that is only right for a 16-byte-aligned destination.  Here every
buffer is carved out of a larger one filled with 0xA5: a guard band on either side, the payload at a chosen 16-byte phase, and the payload
itself filled with the pattern too -- a float payload reads 0xA5A5A5A5 = -2.87e-16, a 16-bit one 0xA5A5 (step / UE id 42 405), a byte 165
(an action above 64 stations): values no kernel here produces.

Works on CPU and GPU tensors (tests/test_guard_cpu.py checks the checker without a GPU).  Host copies only; nothing here launches a kernel.
"""
import ctypes

import numpy as np
import torch

FILL = 0xA5
GUARD_BYTES = 4096      # the largest single wave store is 1 KiB, one staging window at most 1 036 words (B = 32)
STATE_ARRAYS = ('pos', 'mv', 'conn', 'conn_hi', 'ewma', 'conn_since', 'uid', 'orig_consumed')
OUTPUT_ARRAYS = ('obs', 'reward', 'sum_utility', 'ue_dr', 'ue_utility', 'reward_before')


def carve(numel, dtype, device, guard_bytes=GUARD_BYTES, phase_bytes=0):
    """A contiguous payload of exactly `numel` elements that starts guard_bytes + phase_bytes into a byte buffer filled with 0xA5 (payload
    included), with at least guard_bytes behind it.  The returned tensor is what assert_guards / assert_all_written / refill take; give
    the kernels payload.view(shape) -- a view of it keeps the storage, not the bookkeeping."""
    item = torch.empty(0, dtype=dtype).element_size()
    assert guard_bytes % 16 == 0 and 0 <= phase_bytes < 16, (guard_bytes, phase_bytes)
    assert phase_bytes % item == 0, f'a {dtype} payload cannot start {phase_bytes} bytes into a 16-byte line'
    nbytes = int(numel) * item
    start = guard_bytes + phase_bytes
    total = (start + nbytes + guard_bytes + 15) // 16 * 16
    raw = torch.full((total,), FILL, dtype=torch.uint8, device=device)
    assert raw.data_ptr() % 16 == 0, 'the allocator hands out 16-byte-aligned buffers'
    payload = raw[start:start + nbytes].view(dtype)
    assert payload.numel() == numel and payload.is_contiguous() and payload.data_ptr() == raw.data_ptr() + start
    payload._guard = (raw, start, nbytes)
    return payload


def _parts(buf):
    g = getattr(buf, '_guard', None)
    assert g is not None, 'not a tensor carve() returned (a view of one does not carry the guard bookkeeping)'
    return g


def refill(buf):
    """The payload back to the fill pattern (before the next call that must write all of it)."""
    raw, start, nbytes = _parts(buf)
    raw[start:start + nbytes] = FILL


def assert_guards(buf, msg=''):
    """Every guard byte still holds 0xA5.  Names the side, the first and last touched byte relative to the payload's first byte (so an
    overrun starts at the payload's length), and how many bytes changed."""
    raw, start, nbytes = _parts(buf)
    h = raw.cpu().numpy()
    for side, lo, hi in (('before', 0, start), ('after', start + nbytes, h.size)):
        bad = np.nonzero(h[lo:hi] != FILL)[0]
        if bad.size:
            first, last = int(bad[0]) + lo - start, int(bad[-1]) + lo - start
            raise AssertionError(f'{msg}: guard {side} the payload touched: bytes {first} .. {last} relative to the payload '
                                 f'(its length is {nbytes}), {bad.size} bytes changed')


def _unit(buf):
    item = buf.element_size()
    return 4 if item >= 4 else item


def unwritten(buf):
    """Indices (in units of aligned 4-byte words; 2-byte units for 16-bit arrays, bytes for uint8) of the payload that still hold the fill
    pattern, and the unit."""
    raw, start, nbytes = _parts(buf)
    unit = _unit(buf)
    h = raw[start:start + nbytes].cpu().numpy().reshape(-1, unit)
    return np.nonzero((h == FILL).all(axis=1))[0], unit


def assert_all_written(buf, msg='', allow=None):
    """No unit of the payload still holds the fill pattern.  allow: unit indices a documented exception leaves alone (the tables of
    tests/guard_cases.py give each a reason; none exists for obs, obs_compact or reward)."""
    left, unit = unwritten(buf)
    if allow is not None and left.size:
        left = left[~np.isin(left, np.asarray(list(allow), dtype=np.int64))]
    if left.size:
        raise AssertionError(f'{msg}: {left.size} of {buf.numel() * buf.element_size() // unit} {unit}-byte units never written; '
                             f'first unwritten at byte offset {int(left[0]) * unit}, last at {int(left[-1]) * unit}')


def bits(t):
    """A tensor's payload as a flat host array of raw bits (int32 words; 16-bit and 8-bit arrays in their own width)."""
    t = t.detach().contiguous().reshape(-1)
    item = t.element_size()
    if item >= 4:
        return t.view(torch.int32).cpu().numpy().copy()
    return t.view(torch.int16 if item == 2 else torch.uint8).cpu().numpy().copy()


def rehome_state(env, dirty=True):
    """Moves every state array of a fresh BatchedMobileEnv into carved storage (16-byte aligned: nothing claims more for state) and rebuilds
    the dcomp_state the env hands to every call.  dirty: the payloads keep the fill pattern, so reset() meets garbage -- otherwise they are
    zeroed like the env's own.  `flags` stays the env's zeroed word: the kernels atomicOr error bits into it, a dirty one reads as an error.
    Returns {name: carved tensor}."""
    from deepcomp_amd import _lib
    carved = {}
    for name in STATE_ARRAYS:
        t = getattr(env, name)
        if t is None:
            continue
        c = carve(t.numel(), t.dtype, t.device)
        if not dirty:
            c.zero_()
        carved[name] = c
        setattr(env, name, c.view(t.shape))
    ptr = lambda name: carved[name].data_ptr() if name in carved else None      # noqa: E731
    env._st = _lib.DcompState(ptr('pos'), ptr('mv'), ptr('conn'), ptr('ewma'), env.flags.data_ptr(), ptr('conn_since'), ptr('uid'),
                              ptr('orig_consumed'), ptr('conn_hi'))
    env._st_ref = ctypes.byref(env._st)
    return carved


def rehome_outputs(env, phase_bytes=0):
    """Moves the env's own output tensors (what reset() / step() / rollout(out=None) write) into carved storage at the given phase and
    rebuilds the dcomp_out of those calls.  Returns {name: carved tensor}."""
    carved = {}
    for name in OUTPUT_ARRAYS:
        t = getattr(env, name)
        c = carve(t.numel(), t.dtype, t.device, phase_bytes=phase_bytes)
        carved[name] = c
        setattr(env, name, c.view(t.shape))
    env.__dict__.pop('_metric_views', None)
    env._out = env._make_out(env.obs, env.reward)
    env._out_ref = ctypes.byref(env._out)
    return carved
