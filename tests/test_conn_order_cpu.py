"""tests/parity.py::assert_conn_order without a GPU: the checker against a HOST MODEL of dcomp_state.conn_since while the oracle steps.

The model is what the kernels are meant to do with the table (dcomp_device.h / dcomp_dyn.h / dcomp_big.h): a row [B] of uint16 per UE slot,
a successful connect to station b stamps the step into entry b, the row travels with its UE when a departure shifts the slots behind the
leaver, a freed or newly filled slot gets a zero row.  Two things are held here:

* the invariant the GPU tests rest on -- connected slots sorted by (step of connection, slot) ARE the reference's connection list
  (UEs act in list order within a step, later steps append behind, a departure removes without reordering): green over a fixed-list
  batch and two arrival / departure batches, one of them wider than a wavefront;
* the checker can go red: the same runs with ONE entry of the table wrong in each of the ways a kernel could get it wrong -- a connect that
  does not stamp, a row that stays behind on a departure, a row taken from the wrong neighbour, a stamp one step off -- must raise.
  The tampered entry is the first one of the run for which the mistake changes a list at all (a wrong entry of a UE that is alone at its
  station is invisible to any observer, the reference included).
"""
import numpy as np
import pytest

from tests import parity
from tests.env_support import CONN_ORDER_ARRIVAL as ARRIVAL
from tests.env_support import bigb_scenario as _bigb_scenario

TAMPERS = ['no_stamp', 'row_not_moved', 'wrong_neighbour', 'stamp_off_by_one']


def _masks(bits):
    """[..., B] flags -> one mask per UE as state_host() gives it (uint32, uint64 above 32 stations)."""
    B = bits.shape[-1]
    w = (bits.astype(np.uint64) << np.arange(B, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    return w if B > 32 else w.astype(np.uint32)


class HostTable:
    """Stand-in for BatchedMobileEnv: what assert_conn_order reads (E, U, B, num_ue, conn_since, state_host()['conn'])."""

    def __init__(self, oenvs, tamper=None):
        import torch
        self._torch = torch
        self.oenvs = oenvs
        self.E, self.U, self.B = len(oenvs), oenvs[0].U, oenvs[0].B
        self.mc = oenvs[0].max_cap_stations()
        self.since = np.zeros((self.E, self.U, self.B), np.uint16)
        self.bits = np.zeros((self.E, self.U, self.B), bool)
        self.uid = np.stack([o.uids() for o in oenvs])
        self.num_ue = oenvs[0].num_ue()
        self.tamper, self.tampered = tamper, None

    @property
    def conn_since(self):
        return self._torch.from_numpy(self.since.view(np.int16).reshape(-1).copy())

    def state_host(self):
        return {'conn': _masks(self.bits)}

    def _changes_a_list(self, good, bad, bits, n):
        m = _masks(bits)
        return any(parity.conn_order_lists(m, good, n, b) != parity.conn_order_lists(m, bad, n, b) for b in self.mc)

    def advance(self, t, actions):
        """The oracle has taken step t with `actions` ([E, U], by slot BEFORE the step's departures): bring the table up to date."""
        self.num_ue = self.oenvs[0].num_ue()
        for e, o in enumerate(self.oenvs):
            bits = o.state()['conn'].astype(bool)
            uid, n = o.uids(), o.num_ue()
            old = {int(x): i for i, x in enumerate(self.uid[e]) if x}
            src = [old.get(int(uid[sl])) for sl in range(n)]                # slot before the step (None: arrived in this step)
            good = np.zeros_like(self.since[e])
            stamps, moves = [], []
            for sl, i in enumerate(src):
                if i is None:
                    continue
                good[sl] = self.since[e, i]
                if i != sl:
                    moves.append((sl, i))
                b = int(actions[e, i]) - 1
                if b >= 0 and bits[sl, b] and not self.bits[e, i, b]:       # the connect succeeded and the UE is still here
                    good[sl, b] = t
                    stamps.append((sl, i, b))
            new = good
            if self.tamper and self.tampered is None:
                for bad, what in self._candidates(e, t, good, stamps, moves):
                    if self._changes_a_list(good, bad, bits, n):
                        new, self.tampered = bad, (t, e, what)
                        break
            self.since[e], self.bits[e], self.uid[e] = new, bits, uid

    def _candidates(self, e, t, good, stamps, moves):
        if self.tamper == 'no_stamp':                                       # the entry keeps what the row held before
            for sl, i, b in stamps:
                bad = good.copy(); bad[sl, b] = self.since[e, i, b]
                yield bad, f'slot {sl} station {b}: not stamped'
        elif self.tamper == 'stamp_off_by_one':
            for sl, i, b in stamps:
                if t > 0:
                    bad = good.copy(); bad[sl, b] = t - 1
                    yield bad, f'slot {sl} station {b}: stamped {t - 1} at step {t}'
        elif self.tamper == 'row_not_moved':                                # the slot keeps the row of the UE that sat there before
            for sl, i in moves:
                bad = good.copy(); bad[sl] = self.since[e, sl]
                yield bad, f'slot {sl}: row of the previous occupant'
        elif self.tamper == 'wrong_neighbour':                              # the row of the UE one slot further than the one that moved in
            for sl, i in moves:
                if i + 1 < self.U:
                    bad = good.copy(); bad[sl] = self.since[e, i + 1]
                    yield bad, f'slot {sl}: row of slot {i + 1} instead of {i}'


def _run(U0, B, E, arrival, tamper=None, L=40, seed=5):
    from oracle import oracle as orc
    scn = _bigb_scenario(U0, B, 'max-cap')
    M = U0 + 16 if arrival else None
    sched = orc.arrival_schedule(L, arrival) if arrival else [(0, 0)] * L
    oenvs = []
    for e in range(E):
        o = orc.OracleEnv(int(scn.width), int(scn.height), scn.bs_pos, scn.bs_sharing, [s['velocity'] for s in scn.ue_specs], kind=orc.MULTI, max_ues=M)
        o.set_philox(seed, e)
        oenvs.append(o)
    ob = orc.OracleBatch(oenvs)
    ob.reset()
    core = HostTable(oenvs, tamper)
    bs = np.asarray(scn.bs_pos, float)
    rng = np.random.default_rng(3)
    lists = 0
    lists += parity.assert_conn_order(core, oenvs, 'reset')
    stats = parity.ConnOrderStats(oenvs)
    for t in range(L):
        pos = np.stack([o.state()['pos'] for o in oenvs])
        a = parity.near_actions(rng, pos, bs)
        n_rem, n_add = sched[t]
        if n_rem or n_add:
            for o in oenvs:
                o.set_event_counts(n_rem, n_add)
        ob.step(a)
        stats.update()
        core.advance(t, a)
        lists += parity.assert_conn_order(core, oenvs, f'step {t}')
    return lists, stats, core


@pytest.mark.parametrize('U0,B,E,arrival', [(32, 10, 8, None), (9, 48, 8, ARRIVAL), (130, 40, 3, ARRIVAL)])
def test_step_and_slot_order_is_the_reference_list_order(U0, B, E, arrival):
    """Host model of the table, untampered: every max-cap list of every env at every step equals the oracle's, and the run is not vacuous."""
    lists, stats, _ = _run(U0, B, E, arrival)
    assert lists > 0
    stats.require(dynamic=arrival is not None, wide=U0 > 64)


@pytest.mark.parametrize('U0,B,E,arrival,tamper', [(32, 10, 8, None, 'no_stamp'), (32, 10, 8, None, 'stamp_off_by_one')] +
                         [(130, 40, 3, ARRIVAL, k) for k in TAMPERS] + [(9, 48, 8, ARRIVAL, 'row_not_moved'), (9, 48, 8, ARRIVAL, 'wrong_neighbour')])
def test_a_single_wrong_entry_turns_the_checker_red(U0, B, E, arrival, tamper):
    """One entry / row of the table wrong, once (rows only move where UEs depart): assert_conn_order must raise."""
    with pytest.raises(AssertionError, match='connection order') as ex:
        _run(U0, B, E, arrival, tamper)
    assert 'conn_since[slot]' in str(ex.value)


def test_checker_refuses_a_missing_table():
    """Max-cap stations and conn_since is None: a failure, not a pass (and not a skip)."""
    from oracle import oracle as orc
    scn = _bigb_scenario(8, 6, 'max-cap')
    o = orc.OracleEnv(int(scn.width), int(scn.height), scn.bs_pos, scn.bs_sharing, [s['velocity'] for s in scn.ue_specs], kind=orc.MULTI)
    o.set_philox(1, 0)
    o.reset()
    core = HostTable([o])
    assert parity.assert_conn_order(core, [o], 'reset') > 0

    class NoTable(HostTable):
        conn_since = None
    with pytest.raises(AssertionError, match='no conn_since table'):
        parity.assert_conn_order(NoTable([o]), [o], 'reset')
