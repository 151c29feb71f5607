"""Host-side draw tapes for the reference-exact RNG mode.

The reference gives every UE two ``random.Random`` streams seeded ``seed + 100*(i+1)`` (base.py:132-143,
user.py:94-96) and draws, per reset, the start position (user.py:98-109) and, per movement reset, an optional
velocity plus a waypoint (movement.py:110-130).  The device kernels consume those draws from a pre-drawn
tape.  Two producers of the same tape:

* ``mt_tape``  -- the C++ CPython-compatible MT19937 inside libdcomp_hip.so (fast, stateless: always the
  first ``depth`` triples of freshly seeded streams; this is all ``rand_episodes=False`` needs because the
  reference re-seeds at every reset, base.py:171-173);
* ``StdlibStreams`` -- the stdlib generator itself, kept alive across episodes for ``rand_episodes=True``
  (streams continue where the previous episode stopped).
``deepcomp_amd.tape`` decides which producer an env draws from and owns the tape they fill.
"""
import ctypes
import random

import numpy as np

from . import _lib

SLOW, NEW_UE_BORDER = (1, 3), 10     # UEs that arrive during an episode: 'slow', default border (base.py:597-599)


def vel_range(v):
    """Velocity spec -> inclusive draw range (movement.py:112-117)."""
    if v == 'slow':
        return SLOW
    if v == 'fast':
        return 5, 10
    return int(v), int(v)


def mt_tape(cfg_struct, seeds, depth):
    """(pos0[E*U,2] int32, triples[E*U,depth,4] uint16) from the library's MT19937."""
    L = _lib.load()
    seeds = np.ascontiguousarray(seeds, dtype=np.int64)
    E, U = len(seeds), cfg_struct.num_ue
    pos0 = np.zeros((E * U, 2), dtype=np.int32)
    trip = np.zeros((E * U, depth, 4), dtype=np.uint16)
    _lib.check(L.dcomp_mt_draw_tape(ctypes.byref(cfg_struct), seeds.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), E, depth,
                                    pos0.ctypes.data, trip.ctypes.data))
    return pos0, trip


def draw_rows(gen, row, k0, k1, vel, border, w, h, states=None):
    """Triples k0 .. k1 of ONE UE's tape row (row[depth, 4]) from its movement generator, as RandomWaypoint.reset draws them
    (movement.py:110-130): a velocity where the spec is a range, then the waypoint inside the border.  states: a list that gets
    the generator's state after every triple (what the next episode, which continues the stream, is set back to)."""
    lo, hi = vel
    for k in range(k0, k1):
        row[k, :3] = (gen.randint(lo, hi) if lo != hi else lo, gen.randint(border, w - border), gen.randint(border, h - border))
        if states is not None:
            states.append(gen.getstate())


class StdlibStreams:
    """Per-UE stdlib ``random.Random`` pairs for E envs; supports continuing streams across episodes."""

    def __init__(self, seeds, map_w, map_h, vel_specs, init_xy, depth, border=None):
        self.border = [10] * len(vel_specs) if border is None else [int(b) for b in border]      # movement.py:87,126-127
        self.seeds = [int(s) for s in seeds]
        self.w, self.h, self.depth = int(map_w), int(map_h), int(depth)
        self.vel = [vel_range(v) for v in vel_specs]
        self.init_xy = list(init_xy)
        self.U = len(self.vel)
        self._seed_all()
        self._states = None
        self._shift = None
        self._trip = None

    def _seed_all(self):
        self.pos_rng = [[random.Random(s + 100 * (i + 1)) for i in range(self.U)] for s in self.seeds]
        self.mov_rng = [[random.Random(s + 100 * (i + 1)) for i in range(self.U)] for s in self.seeds]

    def _draw(self, trip, k0, k1, fresh=True):
        """Triples k0[e*U+i] .. k1 of every UE's row from its movement stream; fresh: the recorded states start over here."""
        if fresh:
            self._states = [[[mr.getstate()] for mr in env] for env in self.mov_rng]
        for e, env in enumerate(self.mov_rng):
            for i, mr in enumerate(env):
                r = e * self.U + i
                draw_rows(mr, trip[r], k0[r], k1, self.vel[i], self.border[i], self.w, self.h, self._states[e][i])

    def reseed_live(self, seeds, consumed=None):
        """MobileEnv.seed() on a live env (base.py:132-143): BOTH streams of every UE start over at once, from the new seeds.
        What a UE still draws in the running episode comes from the start of its new movement stream: returns the episode's
        triples with row (e, i) continued from position consumed[e*U+i] (the cursor field of the state) by the new stream --
        None when no episode has been drawn yet (the next reset() then simply starts the new streams)."""
        self.seeds = [int(s) for s in seeds]
        self._seed_all()
        if self._trip is None:
            self._states = None
            return None
        self._trip = self._trip.copy()
        self._shift = [int(c) for c in consumed]
        self._draw(self._trip, self._shift, self.depth)
        return self._pos0, self._trip

    def draw_episode(self, reseed, consumed=None):
        """consumed[E*U]: movement triples the previous episode used (the cursor field of the state)."""
        E, U, D = len(self.seeds), self.U, self.depth
        if reseed:
            self._seed_all()
        elif self._states is not None:
            assert consumed is not None
            for e in range(E):
                for i in range(U):
                    shift = self._shift[e * U + i] if self._shift else 0      # triples drawn before a live re-seed
                    self.mov_rng[e][i].setstate(self._states[e][i][int(consumed[e * U + i]) - shift])
        self._shift = None
        pos0 = np.zeros((E * U, 2), dtype=np.int32)
        for e in range(E):
            for i, (ix, iy) in enumerate(self.init_xy):
                pr = self.pos_rng[e][i]
                pos0[e * U + i] = (pr.randint(0, self.w) if ix < 0 else ix, pr.randint(0, self.h) if iy < 0 else iy)
        trip = np.zeros((E * U, D, 4), dtype=np.uint16)
        self._draw(trip, [0] * (E * U), D)
        self._pos0, self._trip = pos0, trip
        return pos0, trip

    def extend(self, new_depth):
        """Continue every movement stream beyond the tape drawn by draw_episode (an episode that runs longer than the
        tape was sized for: --cont-train never resets, main.py:48-51).  The generators still stand where the tape ended."""
        rows, D = len(self._trip), self.depth
        trip = np.zeros((rows, new_depth, 4), dtype=np.uint16)
        trip[:, :D] = self._trip
        self._draw(trip, [D] * rows, new_depth, fresh=False)
        self.depth, self._trip = new_depth, trip
        return self._pos0, trip


def arrival_schedule(episode_length, ue_arrival=None, new_ue_interval=None):
    """Per-step (n_remove, n_add) as MobileEnv.step applies them (base.py:433-443), indexed by env.time before the
    step.  A ue_arrival sequence disables the interval (base.py:52-56)."""
    sched = [(0, 0)] * int(episode_length)
    if ue_arrival:
        for t, n in ue_arrival.items():
            t, n = int(t), int(n)
            if 0 <= t < episode_length:
                sched[t] = (-n, 0) if n < 0 else (0, n)
    elif new_ue_interval:
        for t in range(1, int(episode_length)):
            if t % int(new_ue_interval) == 0:
                sched[t] = (0, 1)
    return sched


def max_num_ue(num_ue, episode_length, ue_arrival=None, new_ue_interval=None):
    """MobileEnv.get_max_num_ue (base.py:191-210)."""
    max_ues = num_ue
    if new_ue_interval is not None and not ue_arrival:
        max_ues = num_ue + int((episode_length - 1) / new_ue_interval)
    if ue_arrival:
        cur = max_ues = num_ue
        for _, n in sorted((int(t), int(n)) for t, n in ue_arrival.items()):
            cur += n
            max_ues = max(max_ues, cur)
    return max_ues


class DynamicStdlibStreams:
    """Reference-exact draws when UEs arrive / depart (`rng='reference'`), for E envs.

    * initial UEs: ``random.Random`` pairs that live as long as the env.  At reset the reference re-seeds
      (rand_episodes=False) the UEs of the list as it stood at the END of the previous episode, by their POSITION in
      that list (base.py:171-173 -> 138-143), then restores the original list (base.py:177-182): an initial UE that
      moved up gets another seed, one that had left keeps its old stream.  Kept exactly.
    * arriving UEs: always freshly seeded ``seed + 100*id`` and 'slow' (base.py:592-606): one tape per possible id.
    * departures: ``random.randint(0, num_ue-1)`` of the GLOBAL generator (base.py:611); arrivals:
      ``map.rand_border_point()`` (map.py:52-65); both seeded with the env seed by MobileEnv.seed (base.py:132-136).
    """

    def __init__(self, seeds, map_w, map_h, vel_specs, init_xy, depth, rand_episodes, max_id, border=None):
        self.border = [10] * len(vel_specs) if border is None else [int(b) for b in border]      # initial UEs; arriving ones: 10
        self.seeds = [int(s) for s in seeds]
        self.w, self.h, self.depth, self.rand_episodes = int(map_w), int(map_h), int(depth), bool(rand_episodes)
        self.vel = [vel_range(v) for v in vel_specs]
        self.init_xy = list(init_xy)
        self.U0, self.max_id = len(self.vel), int(max_id)
        self.pos_rng = [[random.Random(s + 100 * (i + 1)) for i in range(self.U0)] for s in self.seeds]
        self.mov_rng = [[random.Random(s + 100 * (i + 1)) for i in range(self.U0)] for s in self.seeds]
        self.map_rng = [random.Random(s) for s in self.seeds]
        self.glob = [random.Random(s) for s in self.seeds]
        self._states = None
        self._shift = None          # [e][i]: triples initial UE i had drawn before a live re-seed (reseed_live)
        self._live_born = {}        # (e, id) -> (seed, cursor): arrived UEs re-seeded live, for extend()

    def _draw(self, trip, e, i, k0, k1, fresh=True):
        """Triples k0 .. k1 of initial UE i of env e from its movement stream; fresh: its recorded states start over here."""
        mr = self.mov_rng[e][i]
        if fresh:
            self._states[e][i] = [mr.getstate()]
        draw_rows(mr, trip[e * (self.U0 + self.max_id) + i], k0, k1, self.vel[i], self.border[i], self.w, self.h, self._states[e][i])

    def _born_row(self, trip, e, uid, seed, k0, k1):
        """Triples k0 .. k1 of the UE that arrives in env e with id `uid`: a stream of its own, stateless (drawn again at any depth)."""
        draw_rows(random.Random(seed), trip[e * (self.U0 + self.max_id) + self.U0 + uid - 1], k0, k1, SLOW, NEW_UE_BORDER, self.w, self.h)

    def _born_rows(self, trip, e, depth):
        """The rows of every id that may arrive in env e: the configured seed's stream (base.py:601-604), behind the cursor of a live
        re-seed the stream of the list position the UE had then."""
        for uid in range(1, self.max_id + 1):
            self._born_row(trip, e, uid, self.seeds[e] + 100 * uid, 0, depth)
            if (e, uid) in self._live_born:
                self._born_row(trip, e, uid, *self._live_born[(e, uid)], depth)

    def reseed_live(self, seeds, lists, cursors):
        """MobileEnv.seed() while an episode with a changing UE list runs (base.py:132-143).  Per env: the global generator
        (departures, base.py:611) and the map's (arrival points, map.py:52-65) restart from the new seed; every UE of the CURRENT
        list -- initial or arrived -- gets `seed + 100*(position + 1)` for both streams.  lists[e] = [(id, born)] in list order,
        cursors[e][slot] = movement triples consumed so far.  Returns (pos0, triples) with the rows of the listed UEs continued
        from their cursor by the new streams.  UEs that arrive later are still seeded with the CONFIGURED seed (base.py:601-604:
        env_seed), initial UEs that have left keep their old stream, and reset() of a rand_episodes=False env re-seeds with the
        configured seed as always (self.seeds is not touched)."""
        E, U0, D = len(self.seeds), self.U0, self.depth
        trip = self._trip.copy()
        if self._shift is None:
            self._shift = [[0] * U0 for _ in range(E)]
        for e in range(E):
            s = int(seeds[e])
            self.map_rng[e].seed(s)
            self.glob[e].seed(s)
            for pos, (uid, born) in enumerate(lists[e]):
                sd, cur = s + 100 * (pos + 1), int(cursors[e][pos])
                if born:
                    self._live_born[(e, uid)] = (sd, cur)
                    self._born_row(trip, e, uid, sd, cur, D)
                    continue
                self.pos_rng[e][uid - 1].seed(sd)
                self.mov_rng[e][uid - 1].seed(sd)
                self._draw(trip, e, uid - 1, cur, D)
                self._shift[e][uid - 1] = cur
        self._trip = trip
        return self._pos0, trip

    def draw_episode(self, end_lists=None, consumed=None):
        """end_lists[e] = [(id, born)] of env e's list at the end of the previous episode; consumed[e][i] = movement
        triples initial UE i used in it.  Returns (pos0[E*U0,2], triples[E*(U0+max_id), depth, 4])."""
        E, U0, D = len(self.seeds), self.U0, self.depth
        if self._states is not None:
            for e in range(E):
                for i in range(U0):
                    shift = self._shift[e][i] if self._shift else 0
                    self.mov_rng[e][i].setstate(self._states[e][i][int(consumed[e][i]) - shift])
        self._shift, self._live_born = None, {}
        if not self.rand_episodes:
            for e, s in enumerate(self.seeds):
                self.map_rng[e].seed(s)
                self.glob[e].seed(s)
                order = [(i + 1, False) for i in range(U0)] if end_lists is None else end_lists[e]
                for pos, (uid, born) in enumerate(order):
                    if not born:
                        self.pos_rng[e][uid - 1].seed(s + 100 * (pos + 1))
                        self.mov_rng[e][uid - 1].seed(s + 100 * (pos + 1))
        pos0 = np.zeros((E * U0, 2), dtype=np.int32)
        trip = np.zeros((E * (U0 + self.max_id), D, 4), dtype=np.uint16)
        self._states = [[None] * U0 for _ in range(E)]
        for e in range(E):
            for i, (ix, iy) in enumerate(self.init_xy):
                pr = self.pos_rng[e][i]
                pos0[e * U0 + i] = (pr.randint(0, self.w) if ix < 0 else ix, pr.randint(0, self.h) if iy < 0 else iy)
                self._draw(trip, e, i, 0, D)
            self._born_rows(trip, e, D)
        self._pos0, self._trip = pos0, trip
        return pos0, trip

    def extend(self, new_depth):
        """As StdlibStreams.extend: initial UEs continue their generators, the (stateless) tapes of arriving ids are redrawn."""
        E, D = len(self.seeds), self.depth
        trip = np.zeros((len(self._trip), new_depth, 4), dtype=np.uint16)
        trip[:, :D] = self._trip
        for e in range(E):
            for i in range(self.U0):
                self._draw(trip, e, i, D, new_depth, fresh=False)
            self._born_rows(trip, e, new_depth)
        self.depth, self._trip = new_depth, trip
        return self._pos0, trip

    def departures(self, n_remove, num_ue):
        out = np.zeros((len(self.seeds), n_remove), dtype=np.int32)
        for e in range(len(self.seeds)):
            n = num_ue
            for k in range(n_remove):
                out[e, k] = self.glob[e].randint(0, n - 1)
                n -= 1
        return out

    def arrivals(self, n_add):
        out = np.zeros((len(self.seeds), n_add, 2), dtype=np.int32)
        for e in range(len(self.seeds)):
            r = self.map_rng[e]
            for k in range(n_add):
                x, y = r.randint(0, self.w), r.randint(0, self.h)
                border = r.choice(['left', 'right', 'top', 'bottom'])
                out[e, k] = {'left': (0, y), 'right': (self.w - 1, y), 'top': (x, self.h - 1), 'bottom': (x, 0)}[border]
        return out
