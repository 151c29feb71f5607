"""What the tests of the per-UE advantage estimator share (tests/test_gae_uid_cpu.py, test_gae_uid_gpu.py, test_sampler_dyn_gpu.py;
include/dcomp_gae_uid.h): a host simulation of the UE lists of a dynamic env, the independent check that cuts every UE's trajectory out
and hands it to sampler.gae_reference, and the schedule the cases use.  A support module, not a test: nothing here touches a GPU."""
import numpy as np

BORN = 0x8000
# (departures, arrivals) per step of an episode of L = 6 steps: ue_arrival = {1: 2, 2: -1, 3: -2, 5: 1}
SCHEDULE = [(0, 0), (0, 2), (1, 0), (2, 0), (0, 0), (0, 1)]
UE_ARRIVAL = {1: 2, 2: -1, 3: -2, 5: 1}
HORIZON = 6
GAMMA, LAM = 0.99, 0.95


def make_trace(T, E, U, U0, schedule, L, seed, force=None):
    """T steps of E envs with U slots: every env starts an episode with the list [1 ... U0]; step t of an episode applies
    schedule[t] = (departures, arrivals) -- a departure is list.pop(i) with i drawn per env (or force(t, e, k, n) where that returns
    an index: batch step t, env e, k-th departure of the step, n UEs listed), an arrival appends (id of the last + 1) | bit 15, as
    csrc/dcomp_dyn.h does -- and after L steps the list is reset.  Returns (uid, uid_next, end): uint16 [T, E, U] before / after each
    step (after: before the reset), uint8 [T]."""
    rng = np.random.default_rng(seed)
    uid, uid_next, end = np.zeros((T, E, U), np.uint16), np.zeros((T, E, U), np.uint16), np.zeros(T, np.uint8)
    lists = [list(range(1, U0 + 1)) for _ in range(E)]
    time = 0
    for t in range(T):
        n_rem, n_add = schedule[time] if time < len(schedule) else (0, 0)
        for e, ues in enumerate(lists):
            uid[t, e, :len(ues)] = ues
            for k in range(n_rem):
                i = force(t, e, k, len(ues)) if force is not None else None
                ues.pop(int(rng.integers(len(ues))) if i is None else int(i))
            for _ in range(n_add):
                ues.append(((ues[-1] & 0x7FFF) + 1) | BORN)
            assert len(ues) <= U and len(set(ues)) == len(ues)
            uid_next[t, e, :len(ues)] = ues
        time += 1
        if time >= L:
            end[t], time = 1, 0
            lists = [list(range(1, U0 + 1)) for _ in range(E)]
    return uid, uid_next, end


def static_trace(T, E, U, ends=()):
    uid = np.broadcast_to(np.arange(1, U + 1, dtype=np.uint16), (T, E, U)).copy()
    end = np.zeros(T, np.uint8)
    end[list(ends)] = 1
    return uid, uid.copy(), end


def fill_values(uid, uid_next, seed, last=True, poison=True):
    """Rewards, values and (last=True, where the trace does not end on a boundary the caller passes it on) last_vf for a trace; poison:
    NaN wherever no counted row may read -- rewards at slots of uid_next that are dead or hold a UE that did not act in the step, values
    of rows that are dead or whose UE is gone after the step, last_vf at slots nobody's successor is."""
    rng = np.random.default_rng(seed)
    T, E, U = uid.shape
    reward = rng.uniform(-1, 1, size=(T, E, U)).astype(np.float32)
    vf = rng.normal(size=(T, E, U)).astype(np.float32)
    last_vf = rng.normal(size=(E, U)).astype(np.float32) if last else None
    if poison:
        acted = (uid_next[:, :, :, None] == uid[:, :, None, :]).any(axis=3) & (uid_next != 0)       # slot s' of uid_next holds a UE of uid
        stays = (uid[:, :, :, None] == uid_next[:, :, None, :]).any(axis=3) & (uid != 0)
        reward[~acted] = np.nan
        vf[~stays] = np.nan
        if last:
            last_vf[~acted[T - 1]] = np.nan
    return reward, vf, last_vf


def by_trajectory(reward, vf, uid, uid_next, last_vf=None, end=None, gamma=0.99, lam=1.0):
    """The independent check of gae_uid_reference: walks FORWARD, strings every UE's counted rows together as a trajectory of its own
    -- row (t, e, s) with its word at slot s' of uid_next[t] takes reward[t, e, s'] and is followed by row (t + 1, e, s') -- closes
    it at end[t], where the next row does not count, and at the batch end (there with last_vf[e, s'] unless end[T-1]), and runs
    sampler.gae_reference on each as an [n, 1] column.  Returns (advantages, value_targets, live) like gae_uid_reference."""
    from deepcomp_amd.sampler import gae_reference
    T, E, U = uid.shape
    reward, vf = np.asarray(reward, np.float32).reshape(T, E, U), np.asarray(vf, np.float32).reshape(T, E, U)
    uid, uid_next = np.asarray(uid).astype(np.uint16), np.asarray(uid_next).astype(np.uint16)
    adv, tgt, live = np.zeros((T, E, U), np.float32), np.zeros((T, E, U), np.float32), np.zeros((T, E, U), np.uint8)

    def close(rows, boot):
        if rows:
            a, v = gae_reference(np.array([[reward[t, e, sp]] for t, e, s, sp in rows]), np.array([[vf[t, e, s]] for t, e, s, sp in rows]),
                                 None if boot is None else np.array([boot], np.float32), None, gamma, lam)
            for (t, e, s, sp), x, y in zip(rows, a[:, 0], v[:, 0]):
                adv[t, e, s], tgt[t, e, s], live[t, e, s] = x, y, 1

    for e in range(E):
        arriving = {}                                      # slot at step t -> the rows so far of the trajectory that continues there
        for t in range(T):
            going = {}
            for s in range(U):
                rows = arriving.pop(s, [])
                w = uid[t, e, s]
                at = np.nonzero(uid_next[t, e] == w)[0] if w else []
                if len(at) == 0:                           # dead, or the UE departs in this step: what led here ends with next value 0
                    close(rows, None)
                    continue
                sp = int(at[0])
                rows = rows + [(t, e, s, sp)]
                if end is not None and end[t]:
                    close(rows, None)
                elif t == T - 1:
                    close(rows, None if last_vf is None else np.asarray(last_vf, np.float32).reshape(E, U)[e, sp])
                else:
                    going[sp] = rows
            assert not arriving
            arriving = going
    return adv, tgt, live


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a
