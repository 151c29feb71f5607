"""What the env tests share besides the bars of tests/parity.py: the golden fixtures and the entities built from one, the generic
kernel's scenario, the arrival schedule of the connection-order tests, the reference-run UE-arrival check that two files run, and a
free port for the gloo ranks.  No test module is imported here, and none imports another (tests/test_layout_cpu.py)."""
import os
import socket

import numpy as np
import pytest

from tests.parity import ATOL_OBS, ATOL_UTIL, RTOL_RATE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# UE arrival / departure of the connection-order tests (tests/test_conn_order_cpu.py, tests/test_conn_order_gpu.py)
CONN_ORDER_ARRIVAL = {2: 3, 5: -2, 9: 4, 14: -3, 20: 2, 21: 2, 30: -4, 33: 5, 37: -6}


def free_port():
    """Below the kernel's ephemeral range: a bind(0) port can be handed to any outgoing connection before rank 0 binds it."""
    import random
    for _ in range(64):
        port = random.randrange(20000, 32000)
        s = socket.socket()
        try:
            s.bind(('127.0.0.1', port))
            return port
        except OSError:
            continue
        finally:
            s.close()
    raise RuntimeError('no free port')


def bigb_scenario(U, B, sharing, pitch=45):
    from deepcomp_amd import scenarios
    n_static = max(1, U // 8)
    scn = scenarios.grid_map(B, 'mixed' if sharing == 'mixed' else sharing, pitch=pitch, border=25).with_ues(
        num_static=n_static, num_slow=U - n_static - U // 4, num_fast=U // 4)
    if sharing == 'max-cap':                                  # a few other models among the max-cap stations, one of them beyond 31
        for b, m in ((1, 'resource-fair'), (B - 1, 'rate-fair'), (B - 2, 'proportional-fair')):
            scn.bs_sharing[b] = m
    return scn


def entities_from_fixture(g):
    from deepcomp_amd.entities import Basestation, Map, Point, RandomWaypoint, User
    inv_sh = {0: 'resource-fair', 1: 'rate-fair', 2: 'max-cap', 3: 'proportional-fair'}
    w, h = (float(x) for x in g['cfg_map_wh_raw'])
    m = Map(w, h)
    bs = [Basestation(chr(65 + i), Point(x, y), inv_sh[int(s)]) for i, ((x, y), s) in enumerate(zip(g['cfg_bs_pos'], g['cfg_bs_sharing']))]
    vel = {-1: 'slow', -2: 'fast'}
    xy = [['random' if int(c) < 0 else int(c) for c in p] for p in g['cfg_ue_init_xy']]
    U = len(g['cfg_ue_vel'])
    pause = [int(v) for v in g['cfg_ue_pause']] if 'cfg_ue_pause' in g.files else [2] * U           # movement.py:87 defaults
    border = [int(v) for v in g['cfg_ue_border']] if 'cfg_ue_border' in g.files else [10] * U
    vnum = g['cfg_ue_vel_num'] if 'cfg_ue_vel_num' in g.files else [-1.0] * U           # velocities that are no integers (movement.py:116-117)
    ues = [User(str(i + 1), m, xy[i][0], xy[i][1],
                RandomWaypoint(m, float(vnum[i]) if vnum[i] >= 0 else vel.get(int(v), int(v)), pause_duration=pause[i], border_buffer=border[i]),
                util_func='log' if int(u) == 0 else 'step', dr_req=float(r))
           for i, (v, u, r) in enumerate(zip(g['cfg_ue_vel'], g['cfg_ue_util'], g['cfg_ue_dr_req']))]
    return m, bs, ues


def dyn_kwargs(g):
    arr = {int(t): int(n) for t, n in zip(g['cfg_arrival_t'], g['cfg_arrival_n'])} or None
    interval = int(g['cfg_new_ue_interval'])
    return dict(ue_arrival=arr, new_ue_interval=interval if interval > 0 else None, max_ues=int(g['cfg_max_ues']))


def check_golden_dynamic_ue_trajectory(torch, name, via_rollout):
    """UE arrival / departure (base.py:433-443, 592-618) against reference-run fixtures: slot order, ids, masks,
    FP64 positions exact (incl. the reference's reseed-by-list-position behaviour across episodes).  reseeddyn_*: with
    MobileEnv.seed() calls in the middle of episodes (base.py:132-143; listed UEs incl. arrived ones re-seeded by position, the
    departure / arrival-point generators restart)."""
    from deepcomp_amd.entities import Basestation, Map, Point, RandomWaypoint, User
    from deepcomp_amd.env import BatchedMobileEnv
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    inv_sh = {0: 'resource-fair', 1: 'rate-fair', 2: 'max-cap', 3: 'proportional-fair'}
    w, h = (float(x) for x in g['cfg_map_wh_raw'])
    m = Map(w, h)
    bs = [Basestation(chr(65 + i), Point(x, y), inv_sh[int(s)]) for i, ((x, y), s) in enumerate(zip(g['cfg_bs_pos'], g['cfg_bs_sharing']))]
    vel = {-1: 'slow', -2: 'fast'}
    ues = [User(str(i + 1), m, 'random', 'random', RandomWaypoint(m, vel.get(int(v), int(v)))) for i, v in enumerate(g['cfg_ue_vel'])]
    kind = 'central' if int(g['cfg_kind']) == 0 else 'multi'
    core = BatchedMobileEnv(m, bs, ues, kind, num_envs=1, seed=int(g['cfg_seed']), episode_length=int(g['cfg_eps_len']),
                            reward={0: 'avg', 1: 'sum', 2: 'min'}[int(g['cfg_reward'])], rand_episodes=bool(g['cfg_rand_episodes']),
                            rng='reference', tape_depth=48, **dyn_kwargs(g))
    M, B = core.U, core.B
    assert M == int(g['cfg_max_ues'])

    def cmp(prefix, i, with_reward):
        st = core.state_host()
        n = int(g[f'{prefix}_num_ue'][i])
        assert core.num_ue == n
        assert np.array_equal(st['uid'][0], g[f'{prefix}_ue_ids'][i]), f'{prefix}[{i}] ids'
        for k in ('pos', 'wp', 'vel'):
            assert np.array_equal(st[k][0], g[f'{prefix}_{k}'][i]), f'{prefix}[{i}] {k} not bit-exact'
        assert np.array_equal(st['pausing'][0], g[f'{prefix}_pausing'][i]) and np.array_equal(st['curr_pause'][0], g[f'{prefix}_curr_pause'][i])
        conn = ((st['conn'][0][:, None] >> np.arange(B, dtype=st['conn'].dtype)[None, :]) & 1).astype(np.uint8)
        assert np.array_equal(conn, g[f'{prefix}_conn'][i]), f'{prefix}[{i}] connection mask'
        np.testing.assert_allclose(st['ewma'][0], g[f'{prefix}_ewma'][i], rtol=RTOL_RATE, atol=1e-30)
        v = {k: t.cpu().numpy()[0] for k, t in core.obs_views().items()}
        assert np.array_equal(v['connected'].reshape(M, B), g[f'{prefix}_obs_connected'][i])
        np.testing.assert_allclose(v['dr'].reshape(M, B), g[f'{prefix}_obs_dr'][i], rtol=RTOL_RATE, atol=1e-30)
        np.testing.assert_allclose(v['utility'].reshape(M), g[f'{prefix}_obs_utility'][i], atol=ATOL_OBS, rtol=0)
        if kind == 'multi':
            np.testing.assert_allclose(v['ues_at_bs'], g[f'{prefix}_obs_ues_at_bs'][i], atol=1e-6, rtol=0)
            np.testing.assert_allclose(v['util_at_bs'], g[f'{prefix}_obs_util_at_bs'][i], atol=ATOL_OBS, rtol=0)
        if with_reward:
            np.testing.assert_allclose(core.ue_dr.cpu().numpy()[0], g['step_curr_dr'][i], rtol=RTOL_RATE, atol=1e-30)
            np.testing.assert_allclose(core.ue_utility.cpu().numpy()[0], g['step_utility'][i], atol=ATOL_UTIL, rtol=0)
            r = np.atleast_1d(core.reward.cpu().numpy()[0])
            np.testing.assert_allclose(r, g['step_reward'][i], atol=ATOL_UTIL if kind == 'multi' else ATOL_OBS, rtol=0)
            assert float(core.sum_utility.cpu().numpy()[0]) == pytest.approx(float(g['step_sum_utility'][i]), abs=ATOL_UTIL * M)

    seed_at = {int(t_): int(s_) for t_, s_ in g['cfg_seed_at']} if 'cfg_seed_at' in g.files else {}
    t = 0
    for ep in range(int(g['cfg_episodes'])):
        core.reset()
        cmp('reset', ep, False)
        if via_rollout:                                  # the same episode through rollout()'s event feed, in fragments of 1-7 steps
            L, frag = int(g['cfg_eps_len']), 1
            left = L
            while left:
                if t in seed_at:
                    core.seed(seed_at[t], immediate=True)
                n = min([frag, left] + [ts - t for ts in seed_at if ts > t])          # a fragment ends where the caller seeds
                acts = torch.from_numpy(g['actions'][t:t + n].astype(np.uint8).reshape(n, 1, -1)).cuda()
                core.rollout(acts)
                t += n; left -= n
                cmp('step', t - 1, True)
                frag = frag % 7 + 2
            core.check()
            continue
        for _ in range(int(g['cfg_eps_len'])):
            if t in seed_at:
                core.seed(seed_at[t], immediate=True)
            core.step(torch.from_numpy(g['actions'][t].astype(np.uint8).reshape(1, -1)).cuda())
            cmp('step', t, True)
            t += 1
        core.check()
