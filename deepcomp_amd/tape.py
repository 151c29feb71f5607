"""The owner of an env batch's draw tape in the reference-exact RNG mode (``rng='reference'``), host side.

The kernels consume pre-drawn ``(pos0, triples)`` arrays (see ``deepcomp_amd.rng``).  A ``DrawTape`` holds the seeds they are drawn
from, what they are drawn with and the ONE depth of the tape, and says when it must grow.  Which of its three kinds an env has is
decided once, by ``draw_tape()``.  It sees the device only through what the env read back -- the draw cursor per UE slot, the uid
words, ``orig_consumed`` and ``num_ue``, as numpy arrays / ints: no torch here.
"""
import numpy as np

from . import rng as _rng


def uid_fields(words):
    """uid words (dcomp_state.uid, int16 / uint16 array of any shape) -> (id, born): the UE's 1-based id among the initial UEs or
    among the arrived ones, and whether it arrived during the episode.  A tensor of such words (anything with .long() that is not a
    numpy array) stays a tensor on its device: the two fields as an int64 and a bool tensor."""
    id_bits, born_bit = 0x7FFF, 0x8000
    if not isinstance(words, np.ndarray) and hasattr(words, 'long'):
        words = words.long()                               # (int16 words: the sign extension is masked away)
        return words & id_bits, (words & born_bit) != 0
    words = np.asarray(words).astype(np.uint16)
    return (words & id_bits).astype(np.int64), (words & born_bit) != 0


def ue_lists(uid, num_ue):
    """uid[E, U] -> per env the UE list [(id, born)] in list order (the first num_ue slots)."""
    ids, born = uid_fields(uid[:, :num_ue])
    return [list(zip(i, b)) for i, b in zip(ids.tolist(), born.tolist())]


class DrawTape:
    """What every kind shares.  new_episode(**readback) -> (pos0, triples) of the next episode, readback (cursor[E, U]; with arrivals
    also uid[E, U], orig_consumed[E, U0], num_ue) being the state the previous one ended in, wanted once `started`;
    reseed_live(seeds, **readback) -> the RUNNING episode's tape with the new seeds' streams spliced in behind each cursor
    (seed(immediate=True)), None where no episode runs -- afterwards `self.seeds is seeds` where the new seeds are the configured
    ones from here on; needs_host_reset(): a new episode needs a tape the HOST draws, so a rollout with a horizon is cut at the
    episode boundaries (the fixed tape alone is replayed inside the kernel)."""
    started = False

    def __init__(self, seeds, depth, redraw_period):
        self.seeds, self.depth, self.redraw_period = seeds, int(depth), int(redraw_period)
        self._drop()

    def stage_seed(self, seeds):
        """seed() without immediate: in force from the next new_episode() on."""
        self.seeds = seeds
        self._drop()

    def grown(self, t):
        """The tape grown to cover step t of the episode, None if it already does.  A UE redraws at most once per redraw_period steps
        (arrive, pause, draw when it moves on: movement.py:158-181), so step t needs at most t // period + 2 triples.  Episodes that
        outlive the tape -- the reference's done() is always None and --cont-train never resets (main.py:48-51) -- get a longer
        one: the same draws, continued."""
        need = t // self.redraw_period + 3
        if need <= self.depth:
            return None
        self.depth = max(need, 2 * self.depth)
        return self._extend(self.depth)


class FixedTape(DrawTape):
    """rand_episodes=False: the library's MT19937 (stateless: any depth of any seeds' tape at any time), the same tape every episode
    (base.py:171-173) -- and after a live re-seed that tape with the new seeds' streams spliced in, until the next episode."""

    def __init__(self, cfg, *args):
        self.cfg = cfg
        DrawTape.__init__(self, *args)

    def _drop(self):
        self.drawn, self.live = None, None          # the configured seeds' tape; (new seeds, cursors) of a live re-seed

    def needs_host_reset(self):
        return self.live is not None                # a splice: only reset() puts the configured seeds' tape back

    def _extend(self, depth):
        """After a live re-seed row (e, i) = the configured seeds' triples up to the cursor at the time of seed(), the new seeds'
        stream from there on."""
        pos0, trip = _rng.mt_tape(self.cfg, self.seeds, depth)
        if self.live is None:
            self.drawn = pos0, trip
            return self.drawn
        seeds, cursor = self.live
        _, fresh = _rng.mt_tape(self.cfg, seeds, depth)
        for i, c in enumerate(cursor.tolist()):
            trip[i, c:] = fresh[i, :max(depth - c, 0)]
        return pos0, trip

    def new_episode(self):
        self.live = None
        if self.drawn is None or self.drawn[1].shape[1] != self.depth:      # (a live re-seed extended only the spliced tape)
            return self._extend(self.depth)
        return self.drawn

    def reseed_live(self, seeds, cursor=None):
        if cursor is None:                          # no episode runs: reset() draws from the configured seeds anyway
            return None
        self.live = seeds, cursor.astype(np.int64).reshape(-1)
        return self._extend(self.depth)


class ContinuedTape(DrawTape):
    """rand_episodes=True: stdlib streams that go on where the previous episode stopped.  geometry: (map_w, map_h, vel_specs,
    init_xy), then border: as rng.StdlibStreams takes them."""

    def __init__(self, geometry, border, *args):
        self.geometry, self.border = geometry, border
        DrawTape.__init__(self, *args)

    def _drop(self):
        self.streams = None

    started = property(lambda self: self.streams is not None)

    def needs_host_reset(self):
        return True

    def _extend(self, depth):
        return self.streams.extend(depth)

    def new_episode(self, cursor=None):
        if self.streams is None:
            self.streams, cursor = _rng.StdlibStreams(self.seeds, *self.geometry, self.depth, border=self.border), None
        return self.streams.draw_episode(reseed=False, consumed=None if cursor is None else cursor.reshape(-1))

    def reseed_live(self, seeds, cursor=None):
        self.seeds = seeds                          # the new streams are carried on
        return None if self.streams is None else self.streams.reseed_live(seeds, cursor.reshape(-1))


class ArrivalTape(ContinuedTape):
    """UEs arrive and depart (rng.DynamicStdlibStreams): streams per initial UE and per id that may arrive (max_id of them), and the
    draws of the departing list positions [E, n_remove] (base.py:611) / the arrival points [E, n_add, 2] (map.py:52-65) of a step."""

    def __init__(self, rand_episodes, max_id, *args):
        self.rand_episodes, self.max_id = bool(rand_episodes), max_id
        ContinuedTape.__init__(self, *args)

    def departures(self, n_remove, num_ue):
        return self.streams.departures(n_remove, num_ue)

    def arrivals(self, n_add):
        return self.streams.arrivals(n_add)

    def new_episode(self, cursor=None, uid=None, orig_consumed=None, num_ue=None):
        if self.streams is None:
            self.streams = _rng.DynamicStdlibStreams(self.seeds, *self.geometry, self.depth, self.rand_episodes, self.max_id, border=self.border)
            return self.streams.draw_episode()
        # triples every initial UE used: where it left (orig_consumed; 0xFFFF: never left), else the cursor of the slot it sits in
        consumed = orig_consumed.astype(np.uint16).astype(np.int64)
        ids, born = uid_fields(uid[:, :num_ue])
        for e, slot in zip(*np.nonzero(~born)):
            consumed[e, ids[e, slot] - 1] = cursor[e, slot]
        return self.streams.draw_episode(ue_lists(uid, num_ue), consumed.tolist())

    def reseed_live(self, seeds, cursor=None, uid=None, num_ue=None, orig_consumed=None):
        if self.streams is None:                    # no episode yet: the first reset() starts the new streams; a fixed-episode env
            if self.rand_episodes:                  #     re-seeds with the configured seed anyway (base.py:171-173)
                self.seeds = seeds
            return None
        return self.streams.reseed_live(seeds, ue_lists(uid, num_ue), cursor)


def draw_tape(cfg, seeds, depth, redraw_period, geometry, border, rand_episodes=False, max_id=None):
    """The tape owner of an env: cfg is the DcompCfg the library's MT19937 draws for, max_id (None: the UE list is fixed) the ids that
    may arrive during an episode, redraw_period the fewest steps between two redraws of a UE."""
    if max_id is not None:
        return ArrivalTape(rand_episodes, max_id, geometry, border, seeds, depth, redraw_period)
    if rand_episodes:
        return ContinuedTape(geometry, border, seeds, depth, redraw_period)
    return FixedTape(cfg, seeds, depth, redraw_period)
