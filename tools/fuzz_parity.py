#!/usr/bin/env python3
"""Randomised differential test on the GPU box: random env configurations (shape, BS layout, sharing models incl. max-cap,
utility kinds, velocities, fixed start positions incl. UEs parked ON a BS, reward aggregation, agent kind) stepped with
random actions on the HIP path and on the CPU oracle (same Philox draws); masks / FP64 positions bit-exact, floats at the
parity bar.  `python tools/fuzz_parity.py [--cases 200] [--seed 0]`;  tests/test_parity_gpu.py runs a short fixed-seed slice.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import parity  # noqa: E402

RTOL_RATE, ATOL_UTIL, ATOL_OBS = parity.RTOL_RATE, parity.ATOL_UTIL, parity.ATOL_OBS        # one place for the bars (tests/parity.py)
SHARING = ['resource-fair', 'rate-fair', 'max-cap', 'proportional-fair']


_warned = []


class AmbiguousTie(Exception):
    """A max-cap station served a different UE than the oracle's, and the two UEs' FP64 rates are within an ulp of log10 of each other: the
    reference itself decides that case in the last bit of the host's np.log10 (AVX-512 SVML or libm) -- DESIGN.md section 6."""


def maxcap_libm_tie(core, ob, c, st):
    """The per-UE rates differ from the oracle's: is every difference a swapped max-cap winner between two UEs whose squared distances to the
    station agree to 1e-11 relative WITHOUT being equal (equal distances give bit-equal rate keys on every libm: the connection order
    decides, and that is checked, not excused), and are the two wrong rates the oracle's two rates swapped?  Returns a description, or
    None (a real mismatch)."""
    r = ob.rates(want_dr_rel=False)
    want = r['curr_dr']
    E, U = want.shape
    got = core.ue_dr.cpu().numpy().reshape(E, U).astype(np.float64)
    tol = lambda w: parity.RTOL_RATE * np.abs(w) + 1e-30       # noqa: E731
    bad = np.argwhere(np.abs(got - want) > tol(want))
    if len(bad) == 0 or len(bad) % 2:
        return None
    mc = [b for b, m in enumerate(c['sh']) if m == 'max-cap']
    notes = []
    for e in sorted(set(int(b[0]) for b in bad)):
        us = [int(b[1]) for b in bad if int(b[0]) == e]
        if len(us) != 2:
            return None
        u1, u2 = us
        if abs(got[e, u1] - want[e, u2]) > tol(want[e, u2]) or abs(got[e, u2] - want[e, u1]) > tol(want[e, u1]):
            return None                                        # not the oracle's two rates swapped
        pos, conn = st['pos'][e], st['conn'][e]                # (conn: one mask per UE, 64-bit above 32 stations)
        hit = None
        for b in mc:
            if (int(conn[u1]) >> b) & 1 and (int(conn[u2]) >> b) & 1:
                bx, by = c['bs_xy'][b]
                d1 = (pos[u1][0] - bx) ** 2 + (pos[u1][1] - by) ** 2
                d2 = (pos[u2][0] - bx) ** 2 + (pos[u2][1] - by) ** 2
                if d1 != d2 and abs(d1 - d2) <= 1e-11 * max(d1, d2):
                    hit = (b, d1, d2)
        if hit is None:
            return None
        notes.append(f'env {e}: UEs {u1} / {u2} at max-cap station {hit[0]}, d^2 {hit[1]!r} / {hit[2]!r}')
    return 'max-cap winner within an ulp of log10 (DESIGN.md section 6) -- ' + '; '.join(notes)


def random_spec(rng):
    """A random configuration as plain data (JSON-able); build_case() turns it into entity objects."""
    U = int(rng.choice([1, 2, 3, 5, 8, 10, 17, 32, 33, 64, 70, 128, 130]))
    B = int(rng.choice([1, 2, 3, 5, 7, 10, 12, 16, 19, 21, 23, 24, 25, 28, 32]))
    if U * B > 2500 and rng.random() < 0.75:       # most cases small; a quarter keeps the big shapes (wide kernel, 256 lanes per env)
        U = max(1, 2500 // B)
    E = int(rng.choice([1, 3, 8, 21]))
    w, h = int(rng.integers(60, 500)), int(rng.integers(60, 400))
    style = rng.integers(0, 4)
    if style == 0:
        sh = [SHARING[int(rng.integers(0, 4))]] * B
    elif style == 1:
        sh = [SHARING[int(x)] for x in rng.integers(0, 4, B)]
    elif style == 2:
        sh = [['resource-fair', 'rate-fair', 'proportional-fair'][b % 3] for b in range(B)]
    else:
        sh = [SHARING[int(x)] for x in rng.choice([0, 1, 3], B)]
    integer_bs = rng.random() < 0.5
    bs_xy = [[float(rng.integers(0, w + 1)), float(rng.integers(0, h + 1))] if integer_bs else
             [float(rng.uniform(0, w)), float(rng.uniform(0, h))] for _ in range(B)]
    vel, util, req, init = [], [], [], []
    for i in range(U):
        v = [0, 'slow', 'fast', int(rng.integers(1, 30))][int(rng.integers(0, 4))]
        if not isinstance(v, str) and rng.random() < 0.3:      # movement.py:116-117: any number is a velocity (2.5, 0.001, 300)
            v = [round(float(rng.uniform(0, 40)), 3), float(rng.uniform(0, 3)), float(rng.integers(256, 400))][int(rng.integers(0, 3))]
        uf = 'step' if rng.random() < 0.25 else 'log'
        rq = float(rng.choice([1.0, 0.5, 3.0, 20.0]))
        r = rng.random()
        if r < 0.15 and integer_bs:                    # parked on a BS: the d + 1e-16 path
            bx, by = bs_xy[int(rng.integers(0, B))]
            ix, iy = int(bx), int(by)
        elif r < 0.3:
            ix, iy = int(rng.integers(0, w + 1)), -1
        else:
            ix, iy = -1, -1
        vel.append(v); util.append(0 if uf == 'log' else 1); req.append(rq); init.append([ix, iy])
    kind = 'multi' if rng.random() < 0.6 else 'central'
    reward = ['avg', 'sum', 'min'][int(rng.integers(0, 3))]
    arrival = None
    if (U <= 20 or U >= 64) and rng.random() < 0.5:                 # UE arrival / departure (base.py:433-443), also > 1 wavefront
        arrival, cur, steps_max = {}, U, 44
        for t in sorted(set(int(x) for x in rng.integers(1, steps_max, int(rng.integers(1, 9))))):
            n = int(rng.integers(-3, 5))
            n = max(n, 1 - cur)                                      # keep at least one UE in the list
            n = min(n, 250 - cur)
            if n:
                arrival[t] = n
                cur += n
        arrival = arrival or None
    tape = rng.random() < 0.35                                  # reference-exact stdlib-random draws (rng='reference')
    seed = int(rng.integers(0, 2 ** 31))
    # round-2 features, drawn from a stream of their own so that the specs above stay what they were for a given seed:
    # RandomWaypoint(pause_duration, border_buffer) per UE (movement.py:87-104; fixed UE lists only) and stepping the HIP
    # path through the fused rollout kernel in fragments of 1-3 steps
    r2 = np.random.default_rng(seed ^ 0x2F0B5EED)
    pause = border = None
    if arrival is None and r2.random() < 0.4:
        bmax = max(1, min(255, (min(w, h) - 1) // 2))
        pause = [int(r2.choice([0, 1, 2, 3, 6, 20])) for _ in range(U)]
        border = [int(r2.integers(1, bmax + 1)) if r2.random() < 0.7 else min(10, bmax) for _ in range(U)]
    rollout = int(r2.integers(1, 4)) if (arrival is None and r2.random() < 0.35) else 0
    tight = bool(r2.random() < 0.5)                              # DCOMP_TIGHT: U lanes per env where eligible (U not a power of two, <= 32)
    # round 3 (again a stream of its own): envs whose UE list changes go through rollout()'s event feed in fragments of 1-4 steps
    r3 = np.random.default_rng(seed ^ 0x3C6EF372)
    if arrival is not None and r3.random() < 0.45:
        rollout = int(r3.integers(1, 5))
    return dict(pause=pause, border=border, rollout=rollout, tight=tight, **_spec_rest(arrival=arrival, tape=bool(tape), rand_episodes=bool(rng.random() < 0.5), kind=kind, reward=reward, E=E, U=U, B=B,
                w=w, h=h, bs_xy=bs_xy, sh=sh, vel=vel, util=util, req=req, init=init, seed=seed,
                base=int(rng.integers(0, 1000)), steps=int(rng.integers(15, 45)), p_noop=float(rng.choice([0.0, 0.5, 0.9]))))


def _spec_rest(**kw):
    return kw


def _clamp_arrival(arrival, U, cap):
    """A schedule drawn for another UE count: keep at least one UE in the list and at most `cap` slots."""
    if not arrival:
        return None
    cur, arr = U, {}
    for t in sorted(arrival, key=int):
        n = min(int(arrival[t]), cap - cur)
        n = max(n, 1 - cur)
        if n:
            arr[t] = n
            cur += n
    return arr or None


def many_stations(spec, frac):
    """Round 5 (a stream of its own, keyed by the case's seed: every older spec stays what it was): with probability `frac` the case gets
    33 ... 64 stations -- the generic kernel of csrc/dcomp_big.h.  The extra stations are drawn like the first ones; what the generic
    kernel did not have then was dropped from the case; since round 6 nothing is: compact-record twin, rollout fragments (its fused rollout) and arrival schedules stay)."""
    r5 = np.random.default_rng(spec['seed'] ^ 0x51ED270B)
    if r5.random() >= frac:
        return spec
    c = dict(spec)
    B0, B = c['B'], int(r5.choice([33, 34, 36, 40, 47, 48, 56, 63, 64]))
    if c['U'] * B > 5000:
        c['U'] = max(1, 5000 // B)
        for k in ('vel', 'util', 'req', 'init', 'pause', 'border'):
            if c.get(k) is not None:
                c[k] = c[k][:c['U']]
    integer_bs = all(float(x).is_integer() and float(y).is_integer() for x, y in c['bs_xy'])
    c['bs_xy'] = list(c['bs_xy']) + [[float(r5.integers(0, c['w'] + 1)), float(r5.integers(0, c['h'] + 1))] if integer_bs else
                                      [float(r5.uniform(0, c['w'])), float(r5.uniform(0, c['h']))] for _ in range(B - B0)]
    c['sh'] = list(c['sh']) + [c['sh'][b % B0] if len(set(c['sh'])) > 1 or r5.random() < 0.5 else SHARING[int(r5.integers(0, 4))] for b in range(B0, B)]
    c['arrival'] = _clamp_arrival(c.get('arrival'), c['U'], 250)
    c['B'], c['many_stations'] = B, True            # (round 6: the case keeps its UE arrival / departure schedule -- the generic kernel has the event phase)
    return c


def many_ues(spec, frac):
    """Round 5, like many_stations: with probability `frac` the case gets 257 ... 1 024 UEs in ONE env (512- / 1 024-lane workgroups of the generic
    kernel).  The extra UEs repeat the case's own UE specs cyclically; the station count shrinks until the rows fit the LDS; few envs, few steps
    (the oracle walks every UE x station pair on the host)."""
    r6 = np.random.default_rng(spec['seed'] ^ 0x6A09E667)
    if r6.random() >= frac:
        return spec
    c = dict(spec)
    U0, U = c['U'], int(r6.choice([257, 300, 400, 512, 600, 1000, 1024]))
    lanes = 512 if U <= 512 else 1024
    # (round 5 had to shrink the station count until the UEs' LDS rows fitted; the round-6 kernel keeps nothing per (UE, station) in LDS)
    for k in ('vel', 'util', 'req', 'init', 'pause', 'border'):
        if c.get(k) is not None:
            c[k] = [c[k][i % U0] for i in range(U)]
    c['U'], c['many_ues'] = U, True
    c['arrival'] = _clamp_arrival(c.get('arrival'), U, 1024)
    c['E'], c['steps'] = min(c['E'], 3), min(c['steps'], 16)
    return c


def build_case(spec):
    from deepcomp_amd.entities import Basestation, Map, Point, RandomWaypoint, User
    c = dict(spec)
    if c.get('arrival'):
        c['arrival'] = {int(k): int(v) for k, v in c['arrival'].items()}       # JSON keys are strings
    m = Map(c['w'], c['h'])
    c['m'] = m
    c['bs'] = [Basestation(f'B{i}', Point(*xy), s) for i, (xy, s) in enumerate(zip(c['bs_xy'], c['sh']))]
    c['init'] = [tuple(p) for p in c['init']]
    pause, border = c.get('pause') or [2] * c['U'], c.get('border') or [10] * c['U']
    c['ues'] = [User(str(i + 1), m, 'random' if ix < 0 else ix, 'random' if iy < 0 else iy,
                     RandomWaypoint(m, v, pause_duration=pause[i], border_buffer=border[i]),
                     util_func='log' if u == 0 else 'step', dr_req=rq)
                for i, (v, u, rq, (ix, iy)) in enumerate(zip(c['vel'], c['util'], c['req'], c['init']))]
    return c


def random_case(rng):
    return build_case(random_spec(rng))


def run_case(c, torch):
    from deepcomp_amd.env import BatchedMobileEnv
    from oracle import oracle as orc
    E, U, B, kind, reward = c['E'], c['U'], c['B'], c['kind'], c['reward']
    arrival = c.get('arrival')
    tape = bool(c.get('tape'))
    L = 1000 if not arrival else 64
    depth = 48
    os.environ['DCOMP_TIGHT'] = '1' if c.get('tight') else '0'
    try:
        core = BatchedMobileEnv(c['m'], c['bs'], c['ues'], kind, num_envs=E, seed=c['seed'], reward=reward,
                                rng='reference' if tape else 'philox', rand_episodes=c.get('rand_episodes', True) if tape else True,
                                env_id_base=c['base'], episode_length=L, ue_arrival=arrival, tape_depth=depth if tape else None)
    finally:
        os.environ.pop('DCOMP_TIGHT', None)
    U = core.U                                          # slots per env (max_ues when the list changes)
    sched = orc.arrival_schedule(L, arrival) if arrival else None
    envs = []
    for e in range(E):
        o = orc.OracleEnv(c['w'], c['h'], c['bs_xy'], c['sh'], c['vel'], kind=orc.MULTI if kind == 'multi' else orc.CENTRAL,
                          reward_agg={'avg': 0, 'sum': 1, 'min': 2}[reward], ue_util=c['util'], ue_dr_req=c['req'], init_xy=c['init'],
                          max_ues=U if arrival else None, pause=c.get('pause'), border=c.get('border'))
        if not tape:
            o.set_philox(c['seed'], c['base'] + e)
        envs.append(o)
    ob = orc.OracleBatch(envs)
    re = c.get('rand_episodes', True)
    tapes = dyn_tapes = None
    if tape and not arrival:
        tapes = [orc.RefRngTape(int(core.env_seeds[e]), c['w'], c['h'], c['vel'], init_xy=c['init'], depth=depth, rand_episodes=re,
                                border=c.get('border'))
                 for e in range(E)]
    elif tape:                                          # reference draws with a changing UE list (oracle.py: DynRefStreams)
        max_id = len(c['vel']) + sum(a for _, a in sched)
        dyn_tapes = [(orc.DynRefStreams(int(core.env_seeds[e]), c['w'], c['h'], c['vel'], depth=depth, rand_episodes=re, init_xy=c['init']),
                      orc.RefRngTape(int(core.env_seeds[e]), c['w'], c['h'], ['slow'] * max_id, depth=depth),
                      orc.RefEventDraws(int(core.env_seeds[e]), c['w'], c['h'], rand_episodes=re)) for e in range(E)]

    def oracle_reset(first):
        if dyn_tapes:
            for (init_t, new_t, ev), o in zip(dyn_tapes, envs):
                p0, t0 = init_t.draw_episode(*((None, None) if first else (o.end_of_episode_list(), o.orig_consumed())))
                p1, t1 = new_t.draw_episode()
                o.set_tape_ids(np.concatenate([p0, p1]), np.concatenate([t0, t1]))
                ev.new_episode()
        elif tape:                                      # hand every oracle env the reference's own draws for this episode
            for e, o in enumerate(envs):
                o.set_tape(*tapes[e].draw_episode(None if first else o.cursors()))
        elif not first:
            for o in envs:
                o.set_episode(1)
        return ob.reset()
    arng = np.random.default_rng(c['seed'] ^ 0x5bd1e995)

    def cmp(tag, obs_o, rew_o, conn_o, pos_o):
        st = core.state_host()
        if pos_o is not None:
            assert np.array_equal(st['pos'], pos_o), f'{tag}: positions not bit-exact'
            assert np.array_equal(st['conn'], conn_o), f'{tag}: connection masks differ'
            if arrival:
                assert core.num_ue == envs[0].num_ue(), f'{tag}: number of UEs'
                assert np.array_equal(st['uid'], np.stack([o.uids() for o in envs])), f'{tag}: UE ids differ'
            if 'max-cap' in c['sh']:                     # the connection order of every max-cap station (dcomp_state.conn_since) against the oracle's list
                if hasattr(parity, 'assert_conn_order'):
                    parity.assert_conn_order(core, envs, tag)
                elif not _warned:                        # this tool driven with a tests/parity.py older than the checker: say so, once
                    _warned.append(sys.stderr.write('fuzz_parity: tests/parity.py has no assert_conn_order -- the connection order is NOT checked\n'))
        # per-UE data rate, EWMA and the relative-SNR block 1e-5 RELATIVE against the oracle's FP64 values (tests/parity.py)
        try:
            r = parity.assert_rates(core, ob, tag)
        except AssertionError:
            why = maxcap_libm_tie(core, ob, c, st)
            if why:
                raise AmbiguousTie(f'{tag}: {why}')
            raise
        parity.assert_obs(core.obs.cpu().numpy(), obs_o, kind, U, B, dr_rel=r['dr_rel'], msg=tag)
        if rew_o is not None:
            tol = (ATOL_UTIL if kind == 'multi' else ATOL_OBS) * (U if reward == 'sum' else 1)
            np.testing.assert_allclose(core.reward.cpu().numpy(), rew_o, atol=tol, rtol=0, err_msg=f'{tag}: reward')

    # round 4: multi-agent envs also run a TWIN whose steps write the compact record themselves
    # (dcomp_out.obs_compact): unpack of it must be the core env's rows bit for bit, pack of the rows the record word for word
    twin = codec = packed = trew = None
    if kind == 'multi':                                 # (round 6: the generic kernel writes the record too -- two connection words per UE above 32 stations)
        from deepcomp_amd.fragment import FragmentCodec
        os.environ['DCOMP_TIGHT'] = '1' if c.get('tight') else '0'
        try:
            twin = BatchedMobileEnv(c['m'], c['bs'], c['ues'], kind, num_envs=E, seed=c['seed'], reward=reward,
                                    rng='reference' if tape else 'philox', rand_episodes=c.get('rand_episodes', True) if tape else True,
                                    env_id_base=c['base'], episode_length=L, ue_arrival=arrival, tape_depth=depth if tape else None)
        finally:
            os.environ.pop('DCOMP_TIGHT', None)
        codec = FragmentCodec(U, B)
        packed = torch.empty((E, codec.words), dtype=torch.int32, device='cuda')
        trew = torch.empty_like(twin.reward)

    def cmp_twin(tag):
        rows = codec.unpack(packed)
        assert torch.equal(rows.view(torch.int32), core.obs.view(torch.int32)), f'{tag}: unpack(compact record) differs from the rows'
        assert torch.equal(codec.pack(core.obs), packed), f'{tag}: compact record differs from pack(rows)'
        codec.check()

    core.reset()
    if twin is not None:
        twin.reset_compact(packed)
        cmp_twin('reset')
    cmp('reset', oracle_reset(True), None, None, None)
    te = 0                                              # env.time inside the episode
    frag = int(c.get('rollout') or 0)                   # > 0: the HIP path goes through the fused rollout, `frag` steps per call
    pend = []
    for t in range(c['steps']):
        if t == c['steps'] // 2:
            if pend:
                core.rollout(torch.from_numpy(np.stack(pend)).cuda()); pend = []
            core.reset()
            if twin is not None:
                twin.reset_compact(packed)
                cmp_twin('reset2')
            cmp('reset2', oracle_reset(False), None, None, None)
            te = 0
        a = arng.integers(0, B + 1, size=(E, U)).astype(np.uint8)
        a[arng.random((E, U)) < c['p_noop']] = 0
        if frag:                                            # (with UE arrival / departure: rollout()'s event feed)
            if arrival:
                n_rem, n_add = sched[te]
                if n_rem or n_add:
                    for e, o in enumerate(envs):
                        if dyn_tapes:
                            o.set_events(dyn_tapes[e][2].departures(n_rem, o.num_ue()), dyn_tapes[e][2].arrivals(n_add))
                        else:
                            o.set_event_counts(n_rem, n_add)
            pend.append(a)
            res = ob.step(a)
            te += 1
            if len(pend) == frag or t == c['steps'] - 1 or t + 1 == c['steps'] // 2:
                acts = torch.from_numpy(np.stack(pend)).cuda()
                core.rollout(acts)
                if twin is not None:                       # the twin's fragment: every step's record, the last one against the rows
                    tp = torch.empty((len(pend), E, codec.words), dtype=torch.int32, device='cuda')
                    twin.rollout(acts, out={'obs_compact': tp, 'reward': torch.empty((len(pend),) + tuple(twin.reward.shape), device='cuda')})
                    packed.copy_(tp[-1])
                    cmp_twin(f'step {t} (rollout x{frag})')
                pend = []
                cmp(f'step {t} (rollout x{frag})', *res)
            continue
        if arrival:
            n_rem, n_add = sched[te]
            if n_rem or n_add:
                for e, o in enumerate(envs):
                    if dyn_tapes:
                        o.set_events(dyn_tapes[e][2].departures(n_rem, o.num_ue()), dyn_tapes[e][2].arrivals(n_add))
                    else:
                        o.set_event_counts(n_rem, n_add)
        core.step(torch.from_numpy(a).cuda())
        if twin is not None:
            twin.step_compact(torch.from_numpy(a).cuda(), packed, trew)
            cmp_twin(f'step {t}')
            assert torch.equal(trew.view(torch.int32), core.reward.view(torch.int32)), f'step {t}: reward of the compact twin'
        cmp(f'step {t}', *ob.step(a))
        te += 1
    core.check()
    if twin is not None:
        twin.check()


def describe(c):
    return (f"{'MANY-UES ' if c.get('many_ues') else ''}{'MANY-STATIONS ' if c.get('many_stations') else ''}{'TIGHT ' if c.get('tight') else ''}{'ROLLOUT x' + str(c['rollout']) + ' ' if c.get('rollout') else ''}{'PAUSE/BORDER ' if c.get('pause') else ''}{'TAPE rand_episodes=' + str(c.get('rand_episodes')) + ' ' if c.get('tape') else ''}{'DYN ' + str(c['arrival']) + ' ' if c.get('arrival') else ''}{c['kind']} U={c['U']} B={c['B']} E={c['E']} map={c['w']}x{c['h']} reward={c['reward']} sharing={sorted(set(c['sh']))} "
            f"seed={c['seed']} base={c['base']} steps={c['steps']} p_noop={c['p_noop']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', type=int, default=200)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--many-stations', type=float, default=0.0, help='fraction of the cases that get 33 ... 64 stations (generic kernel, csrc/dcomp_big.h)')
    ap.add_argument('--many-ues', type=float, default=0.0, help='fraction of the cases that get 257 ... 1 024 UEs per env (generic kernel)')
    a = ap.parse_args()
    import torch
    rng = np.random.default_rng(a.seed)
    bad = tie = 0
    for i in range(a.cases):
        c = build_case(many_ues(many_stations(random_spec(rng), a.many_stations), a.many_ues))
        try:
            run_case(c, torch)
        except AmbiguousTie as ex:                     # the reference decides it in the last bit of the host's log10: neither side is wrong
            tie += 1
            print(f'case {i} AMBIGUOUS: {describe(c)}\n   {str(ex)[:600]}', flush=True)
        except (AssertionError, Exception) as ex:      # noqa: BLE001
            bad += 1
            print(f'case {i} FAILED: {describe(c)}\n   {str(ex)[:600]}', flush=True)
        if (i + 1) % 250 == 0:
            print(f'... {i + 1 - bad} / {i + 1} agree so far', flush=True)
    print(f'{a.cases - bad - tie} / {a.cases} random configurations agree with the oracle' + (f'; {tie} stopped at a max-cap tie the reference decides in the last bit of log10 (DESIGN.md section 6)' if tie else ''))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
