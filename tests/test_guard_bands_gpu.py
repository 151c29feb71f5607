"""Guard bands, fill patterns and destination phases around every buffer the env kernels write (round 17; tests/guard.py has the why).

For every kernel family of tests/guard_cases.py:

1. TWIN envs step, roll out and write compact records into ordinary zeroed buffers and are held to the FP64 oracle with the helpers and bars of
   tests/parity.py (once per family: the reference is shared by the phases).
2. Envs with the same seed and actions write into carved buffers -- 4 KiB of 0xA5 either side, the payload filled with 0xA5 too, the payload
   at each 4-byte phase of a 16-byte line.  After every call every buffer handed to it has its guards intact, no word left at the fill
   pattern, and is BIT-identical to the twin's: phase and prior contents may change which store instructions run, never a value.
3. The state arrays behind guards, zeroed and filled with garbage before the first reset(): same trajectory, bit for bit.

Two positive controls show that the plumbing sees real kernel stores (a payload declared one row short; an output left out of dcomp_out).
include/dcomp_types.h states the contract these tests hold (dcomp_state comment).
"""
import types
import zlib

import numpy as np
import pytest

from tests import guard, parity
from tests import guard_cases as gc
from tests.threshold_cases import oracle_batch as _oracle

pytestmark = pytest.mark.gpu

SEED = 17
INFO = ('sum_utility', 'ue_dr', 'ue_utility', 'reward_before')


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _scenario(case):
    from deepcomp_amd import scenarios
    U = case.U
    scn = scenarios.grid_map(case.B, 'mixed').with_ues(num_static=U // 8, num_slow=U - U // 8 - U // 4, num_fast=U // 4)
    if gc.sharing_list(case):
        scn.bs_sharing = gc.sharing_list(case)
    return scn


def _make(case, scn):
    from deepcomp_amd.entities import build_from_scenario
    from deepcomp_amd.env import BatchedMobileEnv
    m, bs, ues = build_from_scenario(scn)
    env = BatchedMobileEnv(m, bs, ues, case.kind, num_envs=case.E, seed=SEED, rng='philox', rand_episodes=True,
                           ue_arrival=dict(gc.ARRIVAL) if case.mode == 'dyn' else None)
    env.enable_reward_before()                  # every output surface the kernels have
    return env


def _snap(env, names):
    return {k: guard.bits(getattr(env, k)) for k in names if getattr(env, k) is not None}


def _shapes(env, T):
    E, M = env.E, env.U
    return {'obs': (T,) + tuple(env.obs.shape), 'reward': (T,) + tuple(env.reward.shape), 'sum_utility': (T, E), 'ue_dr': (T, E, M),
            'ue_utility': (T, E, M), 'reward_before': (T, E, M)}


def _hold(case, M, got, o, msg, state=None):
    """One call's outputs (host float arrays) against the oracle's record of it: parity.py's helpers at their own bars.  Where the UE list
    changes, dead slots are held to zero and the rate bars apply to the listed UEs (parity.assert_obs as test_parity_gpu's dynamic test uses it)."""
    E, B, kind = case.E, case.B, case.kind
    if state is not None:
        assert np.array_equal(state['pos'], o['pos']), f'{msg}: FP64 positions not bit-exact'
        assert np.array_equal(state['conn'], o['conn']), f'{msg}: connection masks differ'
    r = o['rates']
    dr, ut = got['ue_dr'].reshape(E, M), got['ue_utility'].reshape(E, M)
    if case.mode != 'dyn':
        stub = types.SimpleNamespace(rates=lambda want_dr_rel=False: r)
        parity.assert_rates(None, stub, msg, ue_dr=dr, ue_utility=ut, ewma=got.get('ewma', False))
        parity.assert_obs(got['obs'].reshape(E, -1), o['obs'], kind, M, B, dr_rel=r['dr_rel'], msg=msg)
    else:
        n = o['n']
        np.testing.assert_allclose(dr[:, :n], r['curr_dr'][:, :n], rtol=parity.RTOL_RATE, atol=1e-30, err_msg=f'{msg}: per-UE data rate')
        np.testing.assert_allclose(ut[:, :n], r['utility'][:, :n], rtol=0, atol=parity.ATOL_UTIL, err_msg=f'{msg}: per-UE utility')
        for k in ('ue_dr', 'ue_utility', 'reward_before') + (('reward',) if kind == 'multi' else ()):
            assert not got[k].reshape(E, M)[:, n:].view(np.int32).any(), f'{msg}: {k} of a dead slot is not +0'
        rows = got['obs'].reshape(E, M, -1) if kind == 'multi' else None
        assert rows is None or not rows[:, n:].view(np.int32).any(), f'{msg}: observation row of a dead slot is not zero'
        parity.assert_obs(got['obs'].reshape(E, -1), o['obs'], kind, M, B, msg=msg)
    if o['rew'] is not None:
        tol = parity.ATOL_UTIL if kind == 'multi' else parity.ATOL_OBS
        np.testing.assert_allclose(got['reward'].reshape(o['rew'].shape), o['rew'], rtol=0, atol=tol, err_msg=f'{msg}: reward')


def _host(env):
    return {k: getattr(env, k).cpu().numpy() for k in guard.OUTPUT_ARRAYS}


_REF = {}


def _reference(torch, case):
    """Everything the carved runs are compared with, computed once per family with the family's environment switches in force: the oracle's
    record, and the bits twin envs wrote into ordinary buffers through every surface -- each twin held to the oracle."""
    if case.name in _REF:
        return _REF[case.name]
    from oracle import oracle as orc
    from deepcomp_amd.fragment import FragmentCodec
    scn = _scenario(case)
    E, B, kind, M, T = case.E, case.B, case.kind, gc.slots(case), gc.steps(case)
    dyn = case.mode == 'dyn'
    twin = _make(case, scn)
    assert twin.U == M
    if case.tag is not None:
        assert case.tag in twin.step_kernel_name, f'{case.name}: dispatched {twin.step_kernel_name}, expected {case.tag}'
    if case.tag != 'big_kernel':
        assert twin.lanes_per_env == case.lanes, f'{case.name}: {twin.lanes_per_env} lanes per env'
    if case.mode == 'rollout':
        assert twin.rollout_is_fused(T), f'{case.name}: this batch does not take a fused rollout kernel'
    if case.mode == 'rollout_steps':
        assert not twin.rollout_is_fused(T)
    assert (twin.conn_since is not None) == (case.sharing == 'maxcap')
    ob = _oracle(scn, kind, E, SEED, max_ues=M if dyn else None)
    sched = orc.arrival_schedule(100, gc.ARRIVAL) if dyn else None
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))

    def record(o_obs, o_rew=None, o_conn=None, o_pos=None):
        return dict(obs=o_obs, rew=o_rew, conn=o_conn, pos=o_pos, rates=ob.rates(want_dr_rel=True), n=ob.envs[0].num_ue() if dyn else M)

    # -- the step-by-step twin
    twin.reset()
    oracle = [record(ob.reset())]
    _hold(case, M, _host(twin), oracle[0], f'{case.name} twin reset')
    calls = [dict(out=_snap(twin, guard.OUTPUT_ARRAYS), state=_snap(twin, guard.STATE_ARRAYS))]
    acts = np.zeros((T, E, M), dtype=np.uint8)
    for t in range(T):
        pos = np.stack([o.state()['pos'] for o in ob.envs])
        a = parity.near_actions(rng, pos, scn.bs_pos)
        a[:, oracle[-1]['n']:] = 0
        acts[t] = a
        if sched is not None and (sched[t][0] or sched[t][1]):
            for o in ob.envs:
                o.set_event_counts(*sched[t])
        twin.step(torch.from_numpy(a).cuda())
        oracle.append(record(*ob.step(a)))
        got = _host(twin)
        if not dyn:
            got['ewma'] = twin.ewma.cpu().numpy()
        _hold(case, M, got, oracle[-1], f'{case.name} twin step {t}', state=twin.state_host())
        calls.append(dict(out=_snap(twin, guard.OUTPUT_ARRAYS), state=_snap(twin, guard.STATE_ARRAYS)))
    twin.check()
    if dyn:         # (oracle side) a slot is dead at a checked call, and a slot dies after having been live
        ns = [o['n'] for o in oracle]
        assert min(ns) < M and any(b < a for a, b in zip(ns, ns[1:])), ns
    assert any(c['state']['conn'].any() for c in calls), f'{case.name}: no UE ever connects'
    acts_dev = torch.from_numpy(acts).cuda()
    ref = dict(scn=scn, M=M, T=T, acts=acts, acts_dev=acts_dev, calls=calls, oracle=oracle, maxcap=ob.envs[0].max_cap_stations(),
               obs_last_dev=twin.obs.clone())

    # -- rollout(out=...): every step's outputs; rollout(out=None): the last step's
    tw = _make(case, scn)
    tw.reset()
    bufs = {k: torch.zeros(s, device='cuda') for k, s in _shapes(tw, T).items()}
    tw.rollout(acts_dev, out=bufs)
    tw.check()
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    for t in range(T):
        _hold(case, M, {k: v[t] for k, v in host.items()}, oracle[t + 1], f'{case.name} twin rollout step {t}',
              state=tw.state_host() if t == T - 1 else None)
    ref['roll'] = {k: guard.bits(v) for k, v in bufs.items()}
    ref['roll_state'] = _snap(tw, guard.STATE_ARRAYS)
    ref['roll_obs_dev'] = bufs['obs']
    tn = _make(case, scn)
    tn.reset()
    tn.rollout(acts_dev)
    tn.check()
    _hold(case, M, _host(tn), oracle[T], f'{case.name} twin rollout, last step only', state=tn.state_host())
    ref['last'] = _snap(tn, guard.OUTPUT_ARRAYS)

    # -- the compact record (multi-agent): unpacks to the very rows the twins above wrote
    if kind == 'multi':
        codec = FragmentCodec(M, B)
        rows = lambda pk: guard.bits(codec.unpack(pk))      # noqa: E731
        tc = _make(case, scn)
        pk, rew = torch.zeros((E, codec.words), dtype=torch.int32, device='cuda'), torch.zeros_like(tc.reward)
        tc.reset_compact(pk)
        assert np.array_equal(rows(pk), calls[0]['out']['obs']), f'{case.name}: compact record of reset'
        ref['compact'] = [guard.bits(pk)]
        for t in range(T):
            tc.step_compact(acts_dev[t], pk, rew)
            assert np.array_equal(rows(pk), calls[t + 1]['out']['obs']), f'{case.name}: compact record of step {t}'
            assert np.array_equal(guard.bits(rew), calls[t + 1]['out']['reward']), f'{case.name}: reward of compact step {t}'
            ref['compact'].append(guard.bits(pk))
        tc.check()
        trc = _make(case, scn)
        trc.reset()
        cb = {k: torch.zeros_like(v) for k, v in bufs.items() if k != 'obs'}
        cb['obs_compact'] = torch.zeros((T, E, codec.words), dtype=torch.int32, device='cuda')
        trc.rollout(acts_dev, out=cb)
        trc.check()
        assert np.array_equal(rows(cb['obs_compact']), ref['roll']['obs']), f'{case.name}: compact records of the rollout'
        for k in cb:
            if k != 'obs_compact':
                assert np.array_equal(guard.bits(cb[k]), ref['roll'][k]), f'{case.name}: {k} of the compact rollout'
        ref['roll_compact'] = guard.bits(cb['obs_compact'])
        ref['roll_compact_dev'] = cb['obs_compact']
        codec.check()
    _REF[case.name] = ref
    return ref


def _check(case, surface, bufs, want, msg):
    """After a call: every buffer handed to it has its guards, no unwritten unit, and the twin's bits."""
    for k, c in bufs.items():
        allow = gc.ALLOW.get((case.name, surface, k), gc.ALLOW.get(('*', surface, k), (None,)))[0]
        assert allow is None or k not in ('obs', 'obs_compact', 'reward')
        guard.assert_guards(c, f'{msg}: {k}')
        guard.assert_all_written(c, f'{msg}: {k}', allow=allow)
        got = guard.bits(c)
        if not np.array_equal(got, want[k]):
            bad = np.nonzero(got != want[k])[0]
            raise AssertionError(f'{msg}: {k} differs from the twin in {bad.size} units, first at {int(bad[0])}: {got[bad[0]]:#x} vs {want[k][bad[0]]:#x}')


def _refill(bufs):
    for c in bufs.values():
        guard.refill(c)


def _carve_outputs(torch, env, T, phase, names=guard.OUTPUT_ARRAYS):
    shp = _shapes(env, T)
    return {k: guard.carve(int(np.prod(shp[k])), torch.float32, 'cuda', phase_bytes=phase) for k in names}


@pytest.mark.parametrize('phase', gc.PHASES)
@pytest.mark.parametrize('case', gc.CASES, ids=gc.IDS)
def test_outputs_behind_guard_bands(torch_cuda, case, phase, monkeypatch):
    """Every output surface of one kernel family with every float / int32 destination `phase` bytes into a 16-byte line."""
    torch = torch_cuda
    from deepcomp_amd import _lib
    from deepcomp_amd.fragment import FragmentCodec
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    ref = _reference(torch, case)
    scn, M, T, acts, calls = ref['scn'], ref['M'], ref['T'], ref['acts_dev'], ref['calls']
    E, multi = case.E, case.kind == 'multi'
    tagm = f'{case.name} phase {phase}'

    # reset_into / step_into: obs and reward
    env = _make(case, scn)
    b = _carve_outputs(torch, env, 1, phase, ('obs', 'reward'))
    env.reset_into(b['obs'])
    _check(case, 'reset_into', {'obs': b['obs']}, calls[0]['out'], f'{tagm} reset_into')
    for t in range(T):
        _refill(b)
        env.step_into(acts[t], b['obs'], b['reward'])
        _check(case, 'step_into', b, calls[t + 1]['out'], f'{tagm} step_into {t}')
    env.check()

    # a plain step with every info tensor: the dcomp_out built here the way step_into builds its own
    env = _make(case, scn)
    b = _carve_outputs(torch, env, 1, phase)
    out = _lib.DcompOut(*[b[k].data_ptr() for k in guard.OUTPUT_ARRAYS], None)
    env.reset()
    for t in range(T):
        _refill(b)
        with torch.cuda.device(env.device):
            env._launch_step(acts[t], out)
        _check(case, 'step', b, calls[t + 1]['out'], f'{tagm} step with info tensors {t}')
    env.check()

    # rollout(out=...): step t's slice of every buffer is at a phase of its own; the guards sit at the ends of the whole fragment
    env = _make(case, scn)
    b = _carve_outputs(torch, env, T, phase)
    env.reset()
    env.rollout(acts, out=b)
    _check(case, 'rollout', b, ref['roll'], f'{tagm} rollout(out=...)')
    env.check()
    if phase == 0:          # heuristic_actions(out=): uint8, at a 16-byte-aligned address like every action buffer
        a_c = guard.carve(E * M, torch.uint8, 'cuda')
        env.heuristic_actions('3gpp', obs=ref['obs_last_dev'], out=a_c)
        _check(case, 'heuristic_actions', {'actions': a_c}, {'actions': guard.bits(env.heuristic_actions('3gpp', obs=ref['obs_last_dev']))},
               f'{tagm} heuristic_actions')

    # rollout(out=None): the last step's outputs land in the env's own tensors -- re-homed behind guards; reset() writes all of them too
    env = _make(case, scn)
    b = guard.rehome_outputs(env, phase)
    env.reset()
    _check(case, 'reset', b, calls[0]['out'], f'{tagm} reset')
    _refill(b)
    env.rollout(acts)
    _check(case, 'rollout_last', b, ref['last'], f'{tagm} rollout(out=None)')
    env.check()

    if not multi:
        return
    # reset_compact / step_compact, rollout(out={'obs_compact': ...}), FragmentCodec.pack(out=) / unpack(out=)
    codec = FragmentCodec(M, case.B)
    assert codec.words == gc.compact_words(case)
    env = _make(case, scn)
    b = {'obs_compact': guard.carve(E * codec.words, torch.int32, 'cuda', phase_bytes=phase),
         'reward': guard.carve(env.reward.numel(), torch.float32, 'cuda', phase_bytes=phase)}
    env.reset_compact(b['obs_compact'])
    _check(case, 'reset_compact', {'obs_compact': b['obs_compact']}, {'obs_compact': ref['compact'][0]}, f'{tagm} reset_compact')
    for t in range(T):
        _refill(b)
        env.step_compact(acts[t], b['obs_compact'], b['reward'])
        _check(case, 'step_compact', b, {'obs_compact': ref['compact'][t + 1], 'reward': calls[t + 1]['out']['reward']}, f'{tagm} step_compact {t}')
    env.check()
    env = _make(case, scn)
    b = _carve_outputs(torch, env, T, phase, ('reward',) + INFO)
    b['obs_compact'] = guard.carve(T * E * codec.words, torch.int32, 'cuda', phase_bytes=phase)
    env.reset()
    env.rollout(acts, out=b)
    _check(case, 'rollout_compact', b, {**ref['roll'], 'obs_compact': ref['roll_compact']}, f'{tagm} rollout(out=obs_compact)')
    env.check()
    pk_c = guard.carve(T * E * codec.words, torch.int32, 'cuda', phase_bytes=phase)
    codec.pack(ref['roll_obs_dev'], out=pk_c)
    _check(case, 'pack', {'obs_compact': pk_c}, {'obs_compact': guard.bits(codec.pack(ref['roll_obs_dev']))}, f'{tagm} FragmentCodec.pack')
    rows_c = guard.carve(ref['roll_obs_dev'].numel(), torch.float32, 'cuda', phase_bytes=phase)
    codec.unpack(ref['roll_compact_dev'], out=rows_c)
    _check(case, 'unpack', {'obs': rows_c}, {'obs': ref['roll']['obs']}, f'{tagm} FragmentCodec.unpack')
    codec.check()


def _since_mask(case, state, maxcap):
    """Entries of conn_since that mean something: [slot][b] with b a max-cap station the slot is connected to (dcomp_types.h)."""
    conn = state['conn'].view(np.uint32).astype(np.uint64)
    if 'conn_hi' in state:
        conn = conn | (state['conn_hi'].view(np.uint32).astype(np.uint64) << np.uint64(32))
    mask = np.zeros((conn.size, case.B), dtype=bool)
    for bs in maxcap:
        mask[:, bs] = ((conn >> np.uint64(bs)) & np.uint64(1)).astype(bool)
    return mask.reshape(-1)


def _check_state(case, ref, carved, want, msg, dirty, after_reset=False):
    for k, c in carved.items():
        guard.assert_guards(c, f'{msg}: state.{k}')
        got = guard.bits(c)
        if k == 'conn_since':
            m = _since_mask(case, want, ref['maxcap'])
            assert np.array_equal(got[m], want[k][m]), f'{msg}: conn_since of an existing max-cap connection differs from the twin'
            if not dirty:
                assert np.array_equal(got, want[k]), f'{msg}: conn_since differs from the twin'
            continue
        if dirty and after_reset:
            guard.assert_all_written(c, f'{msg}: state.{k} after reset() on a garbage-filled array')
        assert np.array_equal(got, want[k]), f'{msg}: state.{k} differs from the twin'


@pytest.mark.parametrize('dirty', [False, True], ids=['zeroed', 'garbage'])
@pytest.mark.parametrize('case', gc.CASES, ids=gc.IDS)
def test_state_behind_guard_bands(torch_cuda, case, dirty, monkeypatch):
    """pos, mv, conn, conn_hi, ewma, conn_since, uid and orig_consumed in carved storage: a padded lane or the lane of slot max_ues that
    writes state behind the last env goes red here.  garbage: the arrays hold 0xA5 before the first reset() -- reset initialises everything
    a later call reads, so state and outputs stay bit-identical to the twin's (conn_since: the entries of existing max-cap connections)."""
    torch = torch_cuda
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    ref = _reference(torch, case)
    scn, T, acts, calls = ref['scn'], ref['T'], ref['acts_dev'], ref['calls']
    msg = f'{case.name} {"garbage" if dirty else "zeroed"} state'
    env = _make(case, scn)
    st = guard.rehome_state(env, dirty=dirty)
    assert set(st) == set(calls[0]['state'])
    env.reset()
    _check_state(case, ref, st, calls[0]['state'], f'{msg} reset', dirty, after_reset=True)
    assert all(np.array_equal(v, calls[0]['out'][k]) for k, v in _snap(env, guard.OUTPUT_ARRAYS).items()), f'{msg}: outputs of reset'
    if case.mode in ('rollout', 'rollout_steps'):
        bufs = {k: torch.zeros(s, device='cuda') for k, s in _shapes(env, T).items()}
        env.rollout(acts, out=bufs)
        _check_state(case, ref, st, ref['roll_state'], f'{msg} rollout', dirty)
        for k, v in bufs.items():
            assert np.array_equal(guard.bits(v), ref['roll'][k]), f'{msg}: {k} of the rollout differs from the twin'
    else:
        for t in range(T):
            env.step(acts[t])
            _check_state(case, ref, st, calls[t + 1]['state'], f'{msg} step {t}', dirty)
            for k, v in _snap(env, guard.OUTPUT_ARRAYS).items():
                assert np.array_equal(v, calls[t + 1]['out'][k]), f'{msg} step {t}: {k} differs from the twin'
    env.check()
    host = env.state_host()
    assert np.array_equal(host['pos'], ref['oracle'][T]['pos']) and np.array_equal(host['conn'], ref['oracle'][T]['conn']), f'{msg}: final state against the oracle'


# ---------------------------------------------------------------------------------------------------- positive controls
def test_control_a_payload_one_row_short_is_an_overrun_of_one_row(torch_cuda):
    """The checker sees real kernel stores: reset() of 3 x 32 x 10 multi-agent envs writes 96 rows of 41 floats; a payload declared 95 rows long
    has its trailing guard touched from exactly its end, for one row (a reset row starts with connected = 0.0 and ends with utility = -1.0:
    neither its first nor its last byte is 0xA5)."""
    torch = torch_cuda
    from deepcomp_amd import _lib
    case = gc.CASES[0]
    assert case.name == 'narrow_32x10'
    env = _make(case, _scenario(case))
    row = 4 * case.B + 1
    short = guard.carve(env.obs.numel() - row, torch.float32, 'cuda')
    env.reset(_out=_lib.DcompOut(short.data_ptr(), env.reward.data_ptr(), None, None, None, None, None))
    env.check()
    n = 4 * short.numel()
    with pytest.raises(AssertionError, match=rf'guard after the payload touched: bytes {n} \.\. {n + 4 * row - 1} relative to the payload'):
        guard.assert_guards(short, 'one row short')
    guard.assert_all_written(short, 'one row short')


def test_control_b_an_output_left_out_stays_unwritten(torch_cuda):
    """ue_dr = NULL in dcomp_out: the step writes every other buffer, and the carved ue_dr is reported unwritten from offset 0."""
    torch = torch_cuda
    from deepcomp_amd import _lib
    case = gc.CASES[0]
    env = _make(case, _scenario(case))
    b = _carve_outputs(torch, env, 1, 0)
    env.reset()
    out = _lib.DcompOut(*[None if k == 'ue_dr' else b[k].data_ptr() for k in guard.OUTPUT_ARRAYS], None)
    with torch.cuda.device(env.device):
        env._launch_step(torch.zeros((env.E, env.U), dtype=torch.uint8, device='cuda'), out)
    env.check()
    n = env.E * env.U
    with pytest.raises(AssertionError, match=rf'{n} of {n} 4-byte units never written; first unwritten at byte offset 0,'):
        guard.assert_all_written(b['ue_dr'], 'left out')
    for k in guard.OUTPUT_ARRAYS:
        guard.assert_guards(b[k], k)
        if k != 'ue_dr':
            guard.assert_all_written(b[k], k)
