"""Shared assertions of the at-scale GPU parity tests: the HIP path against the FP64 CPU oracle at the bar north_star states --
connection masks / positions BIT-EXACT, SINR / data-rate floats within 1e-5 RELATIVE.

Round 2 compared the packed observation tensor with ``rtol=1e-5, atol=1e-5``: for the many relative-SNR entries of 1e-3 ... 1e-6
(far stations) the absolute term swallowed any relative error, and the per-UE data rates / EWMA were not compared at all above
8 envs.  Here the packed row is split by meaning:

* ``connected``                      exact
* ``dr`` (= snr_b / max snr, variants.py:276-284)   rtol 1e-5 against the oracle's FP64 value on EVERY entry a float32 observation can
                                     hold as a normal number (>= 2^-126 = 1.18e-38: far stations of the 32-station map sit at 1e-13, a
                                     UE a metre from a station pushes the others to 1e-10 ... 1e-30); entries below that -- a UE
                                     standing ON a station pushes the others to 1e-50 -- must come out flushed or denormal
                                     (round 4 used atol = 1e-9, which left everything below 1e-9 unchecked)
* ``ues_at_bs`` (count / U)          atol 1e-6
* ``util_at_bs``, ``utility``        atol 5e-6 on [-1, 1]: utility is 10 log10(rate), a 1e-5 RELATIVE rate error is 4.3e-5 / 20 = 2.2e-6
* per-UE data rate ``ue_dr`` (station.py:129-220 summed, user.py:64-69) and ``ewma`` (user.py:148-157)
                                     rtol 1e-5, atol 1e-30 against the oracle's FP64 curr_dr / ewma
* per-UE utility on [-20, 20]        atol 5e-5 (= 4.3e-5, what the 1e-5 rate bar implies, + float32 rounding of a value near 20;
                                     measured <= 2.1e-5; rounds 1-4: 1e-4)
"""
import numpy as np

RTOL_RATE = 1e-5
MAX_CAP = 2                                                # sharing code of a max-cap station (deepcomp_amd._lib.SHARING, oracle.SHARING_CODE)
F32_MIN_NORMAL = float(np.finfo(np.float32).tiny)          # 2^-126
ATOL_OBS = 5e-6
ATOL_UTIL = 5e-5


def assert_dr_obs(got, want, msg=''):
    """obs['dr'] -- relative SNR in (0, 1], variants.py:276-284.  RELATIVE on every entry float32 holds as a normal number; what lies
    below must be flushed / denormal on the device too.  want: FP64 (oracle / fixture) or the oracle's float32 rows."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f'{msg}: obs dr shape {got.shape} vs {want.shape}'
    normal = want >= F32_MIN_NORMAL
    if normal.any():
        rel = np.abs(got[normal] - want[normal]) / want[normal]
        k = int(np.argmax(rel))
        assert rel[k] <= RTOL_RATE, (f'{msg}: obs dr (relative SNR) off by {rel[k]:.3e} relative at value {want[normal][k]:.3e} '
                                     f'(got {got[normal][k]:.9e}); bar {RTOL_RATE}')
    if (~normal).any():
        assert np.all(np.abs(got[~normal]) <= 1.0000001 * F32_MIN_NORMAL), f'{msg}: obs dr entries below the float32 normal range are not flushed / denormal'


def split_packed(obs, kind, U, B):
    """Packed device observation -> dict of [E, U, ...] arrays (multi: [E, U, 4B+1]; central: connected | dr | utility blocks)."""
    E = obs.shape[0]
    if kind == 'multi':
        o = obs.reshape(E, U, 4 * B + 1)
        return {'connected': o[..., :B], 'dr': o[..., B:2 * B], 'ues_at_bs': o[..., 2 * B:3 * B], 'util_at_bs': o[..., 3 * B:4 * B],
                'utility': o[..., 4 * B]}
    o = obs.reshape(E, -1)
    return {'connected': o[:, :U * B].reshape(E, U, B), 'dr': o[:, U * B:2 * U * B].reshape(E, U, B), 'utility': o[:, 2 * U * B:]}


def assert_obs(got_packed, oracle_obs, kind, U, B, dr_rel=None, msg=''):
    """got_packed: device observation (numpy); oracle_obs: OracleBatch's [E, U, 4B+1 | 2B+1] float32 rows; dr_rel: the oracle's FP64
    relative SNR [E, U, B] (OracleBatch.rates(want_dr_rel=True)) -- without it the float32 rows are the reference."""
    g = split_packed(got_packed, kind, U, B)
    w_conn, w_dr = oracle_obs[:, :, :B], oracle_obs[:, :, B:2 * B]
    assert np.array_equal(g['connected'], w_conn), f'{msg}: connected flags differ'
    assert_dr_obs(g['dr'], w_dr if dr_rel is None else dr_rel, msg)
    if kind == 'multi':
        np.testing.assert_allclose(g['ues_at_bs'], oracle_obs[:, :, 2 * B:3 * B], rtol=0, atol=1e-6, err_msg=f'{msg}: ues_at_bs')
        np.testing.assert_allclose(g['util_at_bs'], oracle_obs[:, :, 3 * B:4 * B], rtol=0, atol=ATOL_OBS, err_msg=f'{msg}: util_at_bs')
        np.testing.assert_allclose(g['utility'], oracle_obs[:, :, 4 * B], rtol=0, atol=ATOL_OBS, err_msg=f'{msg}: utility')
    else:
        np.testing.assert_allclose(g['utility'], oracle_obs[:, :, 2 * B], rtol=0, atol=ATOL_OBS, err_msg=f'{msg}: utility')


def assert_rates(core, ob, msg='', ue_dr=None, ue_utility=None, ewma=None):
    """Per-UE data rate, utility and EWMA of the device batch against the oracle's FP64 values (1e-5 RELATIVE on the rates).
    ue_dr / ue_utility / ewma: host arrays to check instead of the core's current tensors (fragment buffers of a rollout)."""
    r = ob.rates(want_dr_rel=True)
    E, U = r['curr_dr'].shape
    dr = core.ue_dr.cpu().numpy() if ue_dr is None else ue_dr
    ut = core.ue_utility.cpu().numpy() if ue_utility is None else ue_utility
    np.testing.assert_allclose(dr.reshape(E, U), r['curr_dr'], rtol=RTOL_RATE, atol=1e-30, err_msg=f'{msg}: per-UE data rate')
    np.testing.assert_allclose(ut.reshape(E, U), r['utility'], rtol=0, atol=ATOL_UTIL, err_msg=f'{msg}: per-UE utility')
    if ewma is not False:
        ew = core.ewma.cpu().numpy() if ewma is None else ewma
        np.testing.assert_allclose(ew.reshape(E, U), r['ewma'], rtol=RTOL_RATE, atol=1e-30, err_msg=f'{msg}: EWMA rate state')
    return r


def assert_step(core, ob, o_obs, o_rew, o_conn, o_pos, kind, reward='avg', msg=''):
    """Everything one step produced, against the oracle batch that took the same step."""
    U, B = core.U, core.B
    st = core.state_host()
    if o_pos is not None:
        assert np.array_equal(st['pos'], o_pos), f'{msg}: FP64 positions not bit-exact'
        assert np.array_equal(st['conn'], o_conn), f'{msg}: connection masks differ'
    r = assert_rates(core, ob, msg)
    assert_obs(core.obs.cpu().numpy(), o_obs, kind, U, B, dr_rel=r['dr_rel'], msg=msg)
    if o_rew is not None:
        tol = (ATOL_UTIL if kind == 'multi' else ATOL_OBS) * (U if reward == 'sum' else 1)
        np.testing.assert_allclose(core.reward.cpu().numpy(), o_rew, rtol=0, atol=tol, err_msg=f'{msg}: reward')


def near_actions(rng, pos, bs, frac=0.6):
    """Actions biased towards stations that are in range, so that UEs hold several connections and stations several UEs.
    pos: host positions [E, U, 2]; bs: station positions [B, 2].  The one copy of the rule the Philox-batch tests draw their actions with."""
    E, U, B = pos.shape[0], pos.shape[1], len(bs)
    d = np.linalg.norm(pos[:, :, None, :] - np.asarray(bs, float)[None, None, :, :], axis=-1)     # [E, U, B]
    near = d < 68.0
    a = rng.integers(0, B + 1, size=(E, U))
    pick = np.where(near.any(-1), (near * rng.random((E, U, B))).argmax(-1) + 1, a)
    a = np.where(rng.random((E, U)) < frac, pick, a)
    a[rng.random((E, U)) < 0.15] = 0
    return a.astype(np.uint8)


def conn_order_lists(conn, conn_since, num_ue, b):
    """One env's device state -> the connection list of station b that it encodes: the slots u < num_ue whose bit b is set in conn[u],
    sorted by (conn_since[u, b] as uint16, u) -- the step of the connection, then the slot (dcomp_state.conn_since)."""
    slots = [u for u in range(num_ue) if (int(conn[u]) >> b) & 1]
    return sorted(slots, key=lambda u: (int(conn_since[u, b]), u))


def assert_conn_order(core, oracle_envs, msg=''):
    """The connection ORDER of every max-cap station (station.py:183-187: among equal FP64 rates the first UE of the station's list is served)
    against the oracle's list, exactly.  The device keeps the list implicitly: dcomp_state.conn_since, uint16 [E*U][B], the step at which
    each connection was made; the list is the connected slots by (step, slot).  The oracle exports the list itself
    (OracleEnv.state()['conn_order'], int32 [B, U], -1 padded).  Which stations are max-cap is taken from the oracle.
    Returns the number of lists compared.  Host copies only."""
    E, U, B = core.E, core.U, core.B
    assert len(oracle_envs) == E, f'{msg}: {len(oracle_envs)} oracle envs for {E} device envs'
    mc = oracle_envs[0].max_cap_stations()
    if not mc:
        return 0
    assert core.conn_since is not None, f'{msg}: the env has max-cap stations {mc} and no conn_since table'
    cs = core.conn_since
    cs = np.asarray(cs.cpu().numpy() if hasattr(cs, 'cpu') else cs)
    assert cs.size == E * U * B, f'{msg}: conn_since has {cs.size} entries, E*U*B = {E * U * B}'
    since = cs.astype(np.int16).view(np.uint16).reshape(E, U, B)
    conn = core.state_host()['conn']
    n = int(core.num_ue)
    checked = 0
    for e, o in enumerate(oracle_envs):
        assert o.num_ue() == n, f'{msg}: env {e}: {n} UEs on the device, {o.num_ue()} in the oracle'
        order = o.state()['conn_order']
        for b in mc:
            got = conn_order_lists(conn[e], since[e], n, b)
            w = order[b]
            stop = np.nonzero(w < 0)[0]
            want = [int(v) for v in (w[:stop[0]] if len(stop) else w)]
            if got != want:
                involved = sorted(set(got) | set(want))
                raise AssertionError(f'{msg}: env {e} max-cap station {b}: connection order {got} on the device, {want} in the oracle; '
                                     f'conn_since[slot] = {{{", ".join(f"{u}: {int(since[e, u, b])}" for u in involved)}}}')
            checked += 1
    return checked


class ConnOrderStats:
    """What keeps a connection-order test from being vacuous, counted on the ORACLE's side (so it does not depend on the code under test):
    max-cap lists with >= 2 UEs, those of them that are not in ascending slot order (the step decides, not the slot), UEs that changed
    slot while holding a max-cap connection, and those of them that crossed a 64-slot (wavefront) boundary.  update() after every step."""

    def __init__(self, oracle_envs):
        self.envs = list(oracle_envs)
        self.mc = self.envs[0].max_cap_stations()
        self.multi = self.nonasc = self.moved = self.cross64 = 0
        self._prev = None

    def update(self):
        cur = []
        for e, o in enumerate(self.envs):
            s, uid, n = o.state(), o.uids(), o.num_ue()
            for b in self.mc:
                w = [int(v) for v in s['conn_order'][b] if v >= 0]
                if len(w) >= 2:
                    self.multi += 1
                    self.nonasc += w != sorted(w)
            if self._prev is not None:
                p_uid, p_held = self._prev[e]
                old = {int(x): i for i, x in enumerate(p_uid) if x}
                for sl in range(n):
                    i = old.get(int(uid[sl]))
                    if i is not None and i != sl and p_held[i]:
                        self.moved += 1
                        self.cross64 += i // 64 != sl // 64
            cur.append((uid, s['conn'][:, self.mc].any(-1)))
        self._prev = cur

    def new_episode(self):
        self._prev = None

    def require(self, dynamic=False, wide=False):
        got = f'lists with >= 2 UEs {self.multi}, not in slot order {self.nonasc}, UEs moved with a max-cap connection {self.moved}, across a 64-slot boundary {self.cross64}'
        assert self.multi >= 100 and self.nonasc >= 20, f'the scenario does not exercise the connection order: {got}'
        assert not dynamic or self.moved >= 20, f'too few slot shifts of connected UEs: {got}'
        assert not wide or self.cross64 >= 5, f'too few slot shifts across a wavefront boundary: {got}'
