"""The max-cap connection ORDER on every kernel family.  A max-cap station serves the UE with the highest FP64 rate and, among equal rates,
the first of its connection list (station.py:183-187).  The kernels keep that list implicitly -- dcomp_state.conn_since, uint16 [E*U][B], the
step at which each connection was made; the list is the connected slots by (step, slot) -- and four winner searches read it.  The rates show
a wrong entry only when two FP64 rate keys are bit-equal, which Philox batches essentially never produce, so here the table itself is held to
the oracle's list (OracleEnv.state()['conn_order']) with tests/parity.py::assert_conn_order after reset() and after EVERY step, on every path
that writes, moves or reads it; tests/test_conn_order_cpu.py shows that (step, slot) order is the reference's order and that the checker goes red.
The last tests tie it to what users see: static UEs at integer mirror positions around max-cap stations, whose rates tie exactly and who connect
in an order that is not slot order.

Every parametrisation asserts, on the ORACLE's side, that it is not vacuous (parity.ConnOrderStats.require): >= 100 lists with >= 2 UEs,
>= 20 of them not in slot order, with arrival / departure >= 20 UEs that changed slot while holding a max-cap connection and, above 64 slots,
>= 5 of them across a 64-slot boundary.
"""
import numpy as np
import pytest

from tests import parity
from tests.env_support import CONN_ORDER_ARRIVAL as ARRIVAL
from tests.env_support import bigb_scenario as _scenario

pytestmark = pytest.mark.gpu

TAPE_DEPTH = 48


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _all_maxcap(U, B, pitch=45):
    scn = _scenario(U, B, 'mixed', pitch)
    scn.bs_sharing[:] = ['max-cap'] * B
    return scn


def _oracle(scn, E, seed, max_ues=None, philox=True):
    from oracle import oracle as orc
    envs = []
    for e in range(E):
        o = orc.OracleEnv(int(scn.width), int(scn.height), scn.bs_pos, scn.bs_sharing, [s['velocity'] for s in scn.ue_specs], kind=orc.MULTI, max_ues=max_ues)
        if philox:
            o.set_philox(seed, e)
        envs.append(o)
    return envs, orc.OracleBatch(envs)


def _ref_tapes(core, scn, arrival, L):
    """rng='reference' with a changing UE list: per env the stdlib-random streams of the initial UEs, of the UEs that arrive, and of the
    events (which UE leaves, where one arrives) -- what BatchedMobileEnv draws on the host and hands the kernels as ev_remove / ev_add_xy."""
    from oracle import oracle as orc
    vel = [s['velocity'] for s in scn.ue_specs]
    w, h = int(scn.width), int(scn.height)
    max_id = len(vel) + sum(a for _, a in orc.arrival_schedule(L, arrival))
    return [(orc.DynRefStreams(int(core.env_seeds[e]), w, h, vel, depth=TAPE_DEPTH, rand_episodes=True, init_xy=[(-1, -1)] * len(vel)),
             orc.RefRngTape(int(core.env_seeds[e]), w, h, ['slow'] * max_id, depth=TAPE_DEPTH),
             orc.RefEventDraws(int(core.env_seeds[e]), w, h, rand_episodes=True)) for e in range(core.E)]


def _make(scn, E, seed, L, arrival=None, rng='philox', **kw):
    from deepcomp_amd.entities import build_from_scenario
    from deepcomp_amd.env import BatchedMobileEnv
    m, bs, ues = build_from_scenario(scn)
    return BatchedMobileEnv(m, bs, ues, 'multi', num_envs=E, seed=seed, episode_length=L, rng=rng, rand_episodes=True, ue_arrival=arrival,
                            tape_depth=TAPE_DEPTH if rng == 'reference' else None, **kw)


def _live_since(core, oenvs):
    """conn_since restricted to what matters: live connections at max-cap stations (everything else zeroed)."""
    E, U, B = core.E, core.U, core.B
    since = core.conn_since.cpu().numpy().view(np.uint16).reshape(E, U, B).copy()
    conn = core.state_host()['conn'].astype(np.uint64)
    live = ((conn[:, :, None] >> np.arange(B, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    live[:, core.num_ue:] = False
    live[:, :, [b for b in range(B) if b not in oenvs[0].max_cap_stations()]] = False
    since[~live] = 0
    return since


def _drive(torch, core, oenvs, ob, scn, steps, L, arrival=None, stats=None, seed=3, t0=0, episode=0, fresh=True, twins=(), tapes=None, after_step=None):
    """`steps` steps from step t0 of `episode` (fresh: reset first), reset at the horizon L: device against oracle at every step -- UE ids,
    connection sets, positions exact, the order of every max-cap list.  `twins`: envs given the same calls (their state is compared by the
    caller, in after_step(msg) if given).  tapes: _ref_tapes() of an rng='reference' env -- the oracle gets the episode's draws and every step's
    departures / arrival points from the reference's streams instead of the Philox key.  Returns the actions [steps, E, U] and the (episode, time) reached."""
    from oracle import oracle as orc
    sched = orc.arrival_schedule(L, arrival) if arrival else [(0, 0)] * L
    bs = np.asarray(scn.bs_pos, float)
    rng = np.random.default_rng(seed)
    acts = []
    t, ep = t0, episode
    dev = core is not None                                     # (core=None: the oracle alone -- what sizes the shapes below)
    pos = None if fresh else np.stack([o.state()['pos'] for o in oenvs])

    def reset():
        for (init_t, new_t, ev), o in zip(tapes or (), oenvs):
            p0, t0_ = init_t.draw_episode(*((None, None) if ep == 0 else (o.end_of_episode_list(), o.orig_consumed())))
            p1, t1_ = new_t.draw_episode()
            o.set_tape_ids(np.concatenate([p0, p1]), np.concatenate([t0_, t1_]))
            ev.new_episode()
        if not tapes:
            for o in oenvs:
                o.set_episode(ep)
        for env in ((core,) + tuple(twins) if dev else ()):
            env.reset()
        ob.reset()
        if stats:
            stats.new_episode()
        if dev:
            assert core.num_ue == oenvs[0].num_ue()
            parity.assert_conn_order(core, oenvs, f'episode {ep} reset')
        return np.stack([o.state()['pos'] for o in oenvs])
    if fresh:
        pos = reset()
    for k in range(steps):
        if t == L:
            ep, t = ep + 1, 0
            pos = reset()
        a = parity.near_actions(rng, pos, bs)
        acts.append(a)
        n_rem, n_add = sched[t]
        if n_rem or n_add:
            for e, o in enumerate(oenvs):
                if tapes:
                    o.set_events(tapes[e][2].departures(n_rem, o.num_ue()), tapes[e][2].arrivals(n_add))
                else:
                    o.set_event_counts(n_rem, n_add)
        for env in ((core,) + tuple(twins) if dev else ()):
            env.step(torch.from_numpy(a).cuda())
        o_obs, o_rew, o_conn, pos = ob.step(a)
        msg = f'episode {ep} step {t}'
        if dev:
            st = core.state_host()
            assert core.num_ue == oenvs[0].num_ue(), msg
            if arrival:
                assert np.array_equal(st['uid'], np.stack([o.uids() for o in oenvs])), f'{msg}: UE ids differ'
            assert np.array_equal(st['conn'], o_conn), f'{msg}: connection sets'
            assert np.array_equal(st['pos'], pos), f'{msg}: positions'
            parity.assert_conn_order(core, oenvs, msg)
            if after_step:
                after_step(msg)
        if stats:
            stats.update()
        t += 1
    return np.stack(acts), ep, t


def _rollout_twin(torch, scn, E, seed, L, acts, core, oenvs, fused=True, **kw):
    """The same batch through rollout(T) in ONE call (T spans the horizon): the order after the call is the oracle's after T steps, and the
    table's live entries are those of the env that took the steps one by one."""
    twin = _make(scn, E, seed, L, **kw)
    assert twin.step_kernel_name == core.step_kernel_name and twin.rollout_is_fused(len(acts)) == fused and len(acts) > L
    twin.reset()
    twin.rollout(torch.from_numpy(acts).cuda(), horizon=L)
    assert twin.time == core.time and twin.episode == core.episode
    assert np.array_equal(twin.state_host()['conn'], core.state_host()['conn'])
    parity.assert_conn_order(twin, oenvs, f'after rollout({len(acts)})')
    assert np.array_equal(_live_since(twin, oenvs), _live_since(core, oenvs)), 'rollout: conn_since of live max-cap connections differs from the stepped env'
    twin.check()


# ---------------------------------------------------------------------------------------------------- fixed UE list
def _is_kernel(core, family, lanes):
    """The dispatch has not moved the case: step_kernel<B, lanes, MP_GENERIC = 0> / step_kernel_dyn<...> / big_kernel<lanes, RESET, DYN, ...>."""
    name, B = core.step_kernel_name, core.B
    want = {'step': f'step_kernel<{B}, {lanes}, 0>', 'dyn': f'step_kernel_dyn<{B}, {lanes}, 0>',
            'big': f'big_kernel<{lanes}, false, false, false, false, false>', 'bigdyn': f'big_kernel<{lanes}, false, true, false, false, false>'}[family]
    assert name == want and core.lanes_per_env == lanes and core.conn_since is not None, (name, core.lanes_per_env, want)


FIXED = [  # U, B, E, layout, kernel family, lanes per env
    (32, 10, 8, 'max-cap', 'step', 32),
    (20, 7, 12, 'all', 'step', 32),
    (128, 12, 3, 'max-cap', 'step', 128),
    (200, 9, 2, 'all', 'step', 256),
    (6, 35, 48, 'max-cap', 'big', 8),
    (20, 40, 8, 'max-cap', 'big', 32),
    (64, 64, 4, 'all', 'big', 64),
    (130, 48, 3, 'max-cap', 'big', 256),
    (1000, 36, 1, 'max-cap', 'big', 1024),
]


def _fixed_scn(U, B, layout):
    return _all_maxcap(U, B) if layout == 'all' else _scenario(U, B, 'max-cap')


@pytest.mark.parametrize('U,B,E,layout,kernel,lanes', FIXED)
def test_order_with_a_fixed_ue_list_steps_and_fused_rollout(torch_cuda, U, B, E, layout, kernel, lanes):
    """step_kernel<..., MP_GENERIC> (<= 32 stations; one env per lane group and envs of several wavefronts) and big_kernel (33 ... 64 stations,
    lane groups 8 ... 1 024, max-cap stations on both sides of station 31): 36 steps across a horizon of 24, then the same batch through the
    fused rollout (the specialised one / big_kernel<..., ROLL>) in one call."""
    L, T = 24, 36
    scn = _fixed_scn(U, B, layout)
    core = _make(scn, E, 77, L)
    _is_kernel(core, kernel, lanes)
    if B > 32:
        sh = list(scn.bs_sharing)
        assert 'max-cap' in sh[:32] and 'max-cap' in sh[32:]
    oenvs, ob = _oracle(scn, E, 77)
    stats = parity.ConnOrderStats(oenvs)
    acts, _, _ = _drive(torch_cuda, core, oenvs, ob, scn, T, L, stats=stats)
    core.check()
    stats.require()
    # (the specialised fused rollout serves envs of one lane group <= 64; wider envs take rollout()'s launch per step -- checked all the same)
    _rollout_twin(torch_cuda, scn, E, 77, L, acts, core, oenvs, fused=not (kernel == 'step' and lanes > 64))


# ---------------------------------------------------------------------------------------------------- UE arrival / departure
DYN = [  # U0, B, E, layout, kernel family, lanes per env, draws
    (9, 10, 12, 'max-cap', 'dyn', 32, 'philox'),              # <= 64 slots: the shuffle shift
    (40, 7, 6, 'all', 'dyn', 64, 'philox'),
    (130, 12, 3, 'max-cap', 'dyn', 256, 'philox'),            # > 64 slots: the LDS exchange
    (9, 48, 8, 'max-cap', 'bigdyn', 32, 'philox'),
    (130, 40, 3, 'max-cap', 'bigdyn', 256, 'philox'),
    (300, 36, 2, 'all', 'bigdyn', 512, 'philox'),
    (9, 10, 12, 'max-cap', 'dyn', 32, 'reference'),           # tape events: the leaver comes from ev_remove, the arrival point from ev_add_xy
    (130, 12, 3, 'max-cap', 'dyn', 256, 'reference'),
    (9, 48, 8, 'max-cap', 'bigdyn', 32, 'reference'),
    (130, 40, 3, 'max-cap', 'bigdyn', 256, 'reference'),
]


@pytest.mark.parametrize('U0,B,E,layout,kernel,lanes,rng', DYN)
def test_order_with_ue_arrival_and_departure(torch_cuda, U0, B, E, layout, kernel, lanes, rng, monkeypatch):
    """step_kernel_dyn and big_kernel<..., DYN>: Philox-keyed and tape (host-drawn, rng='reference') departures (several in one step: -4, -6)
    and arrivals, two episodes of 40 steps.  With DCOMP_FORCE_BIG=1 at <= 32 stations a twin env takes the same steps on the generic kernel:
    its table, restricted to live max-cap connections, is IDENTICAL to the specialised kernel's after every step."""
    L = 40
    scn = _fixed_scn(U0, B, layout)
    core = _make(scn, E, 5, L, ARRIVAL, rng, max_ues=U0 + 16)
    _is_kernel(core, kernel, lanes)
    assert core.U == U0 + 16
    twins = ()
    if B <= 32:
        monkeypatch.setenv('DCOMP_FORCE_BIG', '1')
        big = _make(scn, E, 5, L, ARRIVAL, rng, max_ues=U0 + 16)
        monkeypatch.delenv('DCOMP_FORCE_BIG')
        assert big.step_kernel_name.startswith('big_kernel<') and big.step_kernel_name.endswith(', false, true, false, false, false>')
        twins = (big,)
    oenvs, ob = _oracle(scn, E, 5, max_ues=U0 + 16, philox=rng == 'philox')
    tapes = _ref_tapes(core, scn, ARRIVAL, L) if rng == 'reference' else None
    stats = parity.ConnOrderStats(oenvs)

    def twin_check(msg):
        for tw in twins:
            parity.assert_conn_order(tw, oenvs, f'generic kernel, {msg}')
            assert np.array_equal(_live_since(tw, oenvs), _live_since(core, oenvs)), f'{msg}: generic and specialised kernels: conn_since of live max-cap connections differs'
    for ep in range(2):
        _drive(torch_cuda, core, oenvs, ob, scn, L, L, ARRIVAL, stats=stats, seed=3 + ep, episode=ep, twins=twins, tapes=tapes, after_step=twin_check)
    core.check()
    stats.require(dynamic=True, wide=U0 + 16 > 64)


@pytest.mark.parametrize('U,B,E', [(20, 7, 40), (128, 12, 3)])
def test_generic_and_specialised_kernels_keep_the_same_table(torch_cuda, U, B, E, monkeypatch):
    """DCOMP_FORCE_BIG=1 at <= 32 stations, fixed list: after EVERY step the two tables agree on every live max-cap connection."""
    L = 30
    scn = _scenario(U, B, 'max-cap')
    core = _make(scn, E, 5, L)
    monkeypatch.setenv('DCOMP_FORCE_BIG', '1')
    big = _make(scn, E, 5, L)
    monkeypatch.delenv('DCOMP_FORCE_BIG')
    assert core.step_kernel_name.startswith('step_kernel<') and big.step_kernel_name.startswith('big_kernel<')
    oenvs, ob = _oracle(scn, E, 5)
    stats = parity.ConnOrderStats(oenvs)
    t, ep, fresh = 0, 0, True
    for k in range(L):
        _, ep, t = _drive(torch_cuda, core, oenvs, ob, scn, 1, L, stats=stats, seed=100 + k, t0=t, episode=ep, fresh=fresh, twins=(big,))
        fresh = False
        parity.assert_conn_order(big, oenvs, f'generic kernel, step {k}')
        assert np.array_equal(_live_since(big, oenvs), _live_since(core, oenvs)), f'step {k}'
    stats.require()


# ---------------------------------------------------------------------------------------------------- checkpoints
@pytest.mark.parametrize('U0,B,E,arrival', [(32, 10, 8, None), (20, 40, 8, None), (9, 10, 12, ARRIVAL), (130, 40, 3, ARRIVAL)])
def test_order_survives_a_checkpoint(torch_cuda, U0, B, E, arrival):
    """state_dict() after 22 steps -> a fresh env that has run something else -> load_state_dict() -> 10 more steps: the order is still the
    oracle's at every step.  A checkpoint WITHOUT conn_since / conn_hi / uid zeroes those buffers instead of leaving the old contents."""
    torch = torch_cuda
    L = 40
    kw = dict(max_ues=U0 + 16) if arrival else {}
    scn = _scenario(U0, B, 'max-cap')
    a = _make(scn, E, 9, L, arrival, **kw)
    oenvs, ob = _oracle(scn, E, 9, max_ues=kw.get('max_ues'))
    stats = parity.ConnOrderStats(oenvs)
    _, ep, t = _drive(torch, a, oenvs, ob, scn, 22, L, arrival, stats=stats)
    sd = a.state_dict()
    assert sd['conn_since'] is not None
    b = _make(scn, E, 9, L, arrival, **kw)                                     # same configuration, another history in its buffers
    b.reset()
    rng = np.random.default_rng(0)
    for _ in range(6):
        b.step(torch.from_numpy(parity.near_actions(rng, b.state_host()['pos'], np.asarray(scn.bs_pos, float))).cuda())
    assert int(b.conn_since.ne(0).sum()) > 0
    old = {k: sd[k] for k in ('conn_since', 'conn_hi', 'uid')}
    sd.update(conn_since=None, conn_hi=None, uid=None)
    b.load_state_dict(sd)
    for k in old:
        assert getattr(b, k) is None or int(getattr(b, k).ne(0).sum()) == 0, f'{k} kept its old contents'
    sd.update(old)
    b.load_state_dict(sd)
    parity.assert_conn_order(b, oenvs, 'restored')
    _drive(torch, b, oenvs, ob, scn, 10, L, arrival, stats=stats, seed=8, t0=t, episode=ep, fresh=False)
    b.check()
    stats.require(dynamic=arrival is not None, wide=U0 + 16 > 64 and arrival is not None)


# ---------------------------------------------------------------------------------------------------- the order decides a rate
def _tie_case(B, U, groups, w=400, h=400):
    """Static UEs (velocity 0, fixed integer start points).  groups: {station: (slot_a, slot_b, slot_c)} -- the three UEs sit at the integer
    mirror points (x + 30, y), (x - 30, y), (x, y + 30) of their max-cap station: squared distance 900.0 for all three, the FP64 rate keys are
    bit-equal on any libm.  Every other UE sits far from the tied stations and never connects (it is there to depart)."""
    from deepcomp_amd.entities import Basestation, Map, Point, RandomWaypoint, User
    m = Map(w, h)
    cols = int(np.ceil(np.sqrt(B)))
    bs_xy = [[40.0 + 320.0 * (b % cols) / max(1, cols - 1), 40.0 + 320.0 * (b // cols) / max(1, cols - 1)] for b in range(B)]
    bs_xy = [[float(round(x)), float(round(y))] for x, y in bs_xy]
    init = [(5 + (i * 7) % 20, 395 - (i * 3) % 10) for i in range(U)]          # a corner of the map, out of range of the tied stations
    for b, slots in groups.items():
        x, y = int(bs_xy[b][0]), int(bs_xy[b][1])
        for s, (dx, dy) in zip(slots, ((30, 0), (-30, 0), (0, 30))):
            init[s] = (x + dx, y + dy)
    bs = [Basestation(f'B{i}', Point(*xy), 'max-cap') for i, xy in enumerate(bs_xy)]
    ues = [User(str(i + 1), m, ix, iy, RandomWaypoint(m, 0)) for i, (ix, iy) in enumerate(init)]
    return m, bs, ues, bs_xy, init


def _run_tie(torch, B, U, groups, E, arrival, kernel, lanes, steps=12):
    """Step 0: the HIGHEST slot of each group connects; step 1: the lowest; step 2: the middle one -- in the very step in which the first UEs
    depart (arrival[2] < 0).  The list is [c, a, b] by slot: 'lowest slot wins' serves a, 'oldest connection wins' serves c.  Later steps:
    more departures (the tied UEs shift, some leave), a disconnect / reconnect that sends the oldest to the back of the list."""
    from deepcomp_amd.env import BatchedMobileEnv
    from oracle import oracle as orc
    m, bs, ues, bs_xy, init = _tie_case(B, U, groups)
    L = 30
    core = BatchedMobileEnv(m, bs, ues, 'multi', num_envs=E, seed=11, episode_length=L, rng='philox', rand_episodes=True, ue_arrival=arrival)
    _is_kernel(core, kernel, lanes)
    assert core.U == U
    sched = orc.arrival_schedule(L, arrival) if arrival else [(0, 0)] * L
    oenvs = []
    for e in range(E):
        o = orc.OracleEnv(m.width, m.height, bs_xy, ['max-cap'] * B, [0] * U, kind=orc.MULTI, init_xy=init, max_ues=U if arrival else None)
        o.set_philox(11, e)
        oenvs.append(o)
    ob = orc.OracleBatch(oenvs)
    core.reset()
    parity.assert_step(core, ob, ob.reset(), None, None, None, 'multi', msg='reset')
    uid0 = {b: [s + 1 for s in slots] for b, slots in groups.items()}          # ids of the tied UEs (id = initial slot + 1)
    decided = 0
    for t in range(steps):
        ids = np.stack([o.uids() for o in oenvs])                              # [E, U] id per slot now
        a = np.zeros((E, U), np.uint8)
        for b, (ia, ib, ic) in uid0.items():
            who = {0: [ic], 1: [ia], 2: [ib], 5: [ic], 6: [ic], 8: [ia], 9: [ia]}.get(t, [])      # 5 / 6: the oldest leaves the list and joins at its end
            for i in who:
                a[ids == i] = b + 1
        n_rem, n_add = sched[t]
        if n_rem or n_add:
            for o in oenvs:
                o.set_event_counts(n_rem, n_add)
        core.step(torch.from_numpy(a).cuda())
        o_obs, o_rew, o_conn, o_pos = ob.step(a)
        msg = f'step {t}'
        assert core.num_ue == oenvs[0].num_ue(), msg
        if arrival:
            assert np.array_equal(core.state_host()['uid'], np.stack([o.uids() for o in oenvs])), f'{msg}: UE ids differ'
        parity.assert_conn_order(core, oenvs, msg)
        parity.assert_step(core, ob, o_obs, o_rew, o_conn, o_pos, 'multi', msg=msg)
        for o in oenvs[:8]:                                                    # (oracle side) the order decided a rate: the served UE is not the lowest slot
            s = o.state()
            for b in groups:
                lst = [int(v) for v in s['conn_order'][b] if v >= 0]
                decided += len(lst) >= 2 and lst[0] != min(lst)
    core.check()
    assert decided >= 8, f'the scenario never let the connection order decide a rate ({decided})'


def test_tied_rates_with_a_fixed_list(torch_cuda):
    """step_kernel<..., MP_GENERIC> and the generic kernel at 40 stations (tied stations 0 and 35), no departures: the served UE among three
    bit-equal rates is the oldest connection, not the lowest slot, at every step."""
    _run_tie(torch_cuda, 6, 12, {0: (3, 4, 5), 4: (8, 9, 10)}, 64, None, 'step', 16)
    _run_tie(torch_cuda, 40, 70, {0: (63, 64, 65), 35: (20, 21, 22)}, 64, None, 'big', 128)


def test_tied_rates_with_departures_on_the_specialised_dynamic_kernel(torch_cuda):
    """step_kernel_dyn, <= 64 slots and > 64 slots: the tied UEs shift (or leave) while they hold the tie."""
    arrival = {2: -1, 4: -2, 7: -3}
    _run_tie(torch_cuda, 6, 12, {0: (3, 4, 5), 4: (8, 9, 10)}, 256, arrival, 'dyn', 16)
    _run_tie(torch_cuda, 6, 70, {0: (63, 64, 65), 4: (20, 21, 22)}, 256, arrival, 'dyn', 128)


def test_tied_rates_across_a_wavefront_boundary_on_the_generic_kernel(torch_cuda):
    """big_kernel<..., DYN>, 132 slots (256 lanes per env), the tied UEs of station 0 in slots 63 / 64 / 65 and those of station 35 in slots
    127 / 128 / 129 -- each group straddles two wavefronts -- and the UE of slot 64 (128) connects in the very step in which a UE of a lower
    slot departs: the toggle's stamp of slot 64 is stored by lane 0 of one wavefront and read, for the row move, by lane 63 of the previous one.
    Until the removal loop got a barrier in front of that read the two were unordered (a data race; the stale step then travelled with the
    shifted UE and the wrong UE was served).  2 048 envs = 2 048 workgroups of 256 lanes, 8 per CU of the 256-CU MI355X, so wavefronts of many
    workgroups interleave on every CU.

    A race does not fire on demand: this test being green says nothing about its absence (that is argued from the code: barrier -> read ->
    barrier -> write in dcomp_big.h), and it neither loops nor re-runs to catch one.  It pins the behaviour, and it fails for the
    deterministic forms of the same mistake: the stamp dropped, the row not moved, the winner taken by slot alone."""
    arrival = {2: -1, 4: -2, 7: -3}
    _run_tie(torch_cuda, 40, 132, {0: (63, 64, 65), 35: (127, 128, 129)}, 2048, arrival, 'bigdyn', 256, steps=10)
