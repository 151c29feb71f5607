"""deepcomp_amd.tape (the owner of the rng='reference' draw tape) and the decoders of the state words, without a GPU.

Every kind of tape is walked through new episode -> growth -> live re-seed -> growth -> next episode and held to ``random.Random``
sequences derived by hand from the reference's rules (base.py:132-143, 171-173, 592-611; user.py:94-109; movement.py:110-130); the fixed
kind draws with the library's host-only dcomp_mt_draw_tape."""
import random

import numpy as np
import pytest

W, H = 194, 120
VEL, VR, BORDER, INIT = ['slow', 5], [(1, 3), (5, 5)], [10, 20], [(-1, -1), (3, -1)]
GEOMETRY = (W, H, VEL, INIT)


@pytest.fixture(scope='module')
def lib():
    from deepcomp_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 on a GPU-less host
    return _lib.load()


def _seq(seed, n, vr=(1, 3), bb=10, skip=0):
    """Triples skip .. skip + n of random.Random(seed)'s movement stream."""
    r = random.Random(seed)
    return [[r.randint(*vr) if vr[0] != vr[1] else vr[0], r.randint(bb, W - bb), r.randint(bb, H - bb)] for _ in range(skip + n)][skip:]


def _pos(seed, init, nth=0):
    """Start position number `nth` of random.Random(seed)'s position stream (user.py:98-109: a fixed coordinate draws nothing)."""
    r = random.Random(seed)
    return [[r.randint(0, W) if init[0] < 0 else init[0], r.randint(0, H) if init[1] < 0 else init[1]] for _ in range(nth + 1)][nth]


def _rows(trip):
    assert trip.dtype == np.uint16 and trip.shape[2] == 4 and not trip[:, :, 3].any()
    return [r.tolist() for r in trip[:, :, :3]]


def test_state_word_decoders():
    import torch
    from deepcomp_amd.env import conn_mask, mv_cursor
    from deepcomp_amd.tape import ue_lists, uid_fields
    cur = [0, 1, 0x7FFF, 0x8000, 0xFFFF]                                     # (the top bit set: a negative int64 on the device)
    words = [(c << 48) | 0x8123_4567_89AB for c in cur]
    assert mv_cursor(np.array(words, dtype=np.uint64)).tolist() == cur
    assert mv_cursor(torch.from_numpy(np.array(words, dtype=np.uint64).view(np.int64))).tolist() == cur
    uid = np.array([[1, 0x8001, 0x7FFF, 0xFFFF, 0]], dtype=np.uint16)
    for w in (uid, uid.view(np.int16)):                                      # (the device tensor is int16)
        ids, born = uid_fields(w)
        assert ids.tolist() == [[1, 1, 0x7FFF, 0x7FFF, 0]] and born.tolist() == [[False, True, False, True, False]]
        assert ue_lists(w, 3) == [[(1, False), (1, True), (0x7FFF, False)]]
    lo, hi = np.array([-1, 5, 0], dtype=np.int32), np.array([1, -2 ** 31, 0], dtype=np.int32)
    assert conn_mask(lo).dtype == np.uint32 and conn_mask(lo).tolist() == [0xFFFFFFFF, 5, 0]
    assert conn_mask(lo, hi).dtype == np.uint64 and conn_mask(lo, hi).tolist() == [0x1_FFFF_FFFF, (1 << 63) | 5, 0]


def test_fixed_tape(lib):
    """rand_episodes=False: the same tape every episode; a live re-seed splices the new seeds' streams in behind each cursor until the
    next episode, growth included."""
    from deepcomp_amd import _lib, tape
    c = _lib.DcompCfg()
    c.num_envs, c.num_ue, c.num_bs, c.map_w, c.map_h = 2, 2, 1, W, H
    keep = [np.array([r[k] for r in VR], np.int32) for k in (0, 1)] + [np.array([p[k] for p in INIT], np.int32) for k in (0, 1)]
    c.ue_vel_lo, c.ue_vel_hi, c.ue_init_x, c.ue_init_y = [a.ctypes.data_as(_lib._ip) for a in keep]
    seeds, seeds2 = np.array([42, 20042]), np.array([977, 20977])
    t = tape.draw_tape(c, seeds, 3, 1, GEOMETRY, None, rand_episodes=False)
    assert isinstance(t, tape.FixedTape) and not t.started and not t.needs_host_reset()
    own = lambda s, n: [_seq(e + 100 * (i + 1), n, VR[i]) for e in s.tolist() for i in range(2)]      # noqa: E731  (default border 10)
    p0, t0 = t.new_episode()
    assert p0.tolist() == [_pos(e + 100 * (i + 1), INIT[i]) for e in (42, 20042) for i in range(2)] and _rows(t0) == own(seeds, 3)
    assert t.grown(0) is None and t.depth == 3                               # one redraw per step: step t needs t + 3 triples
    _, t1 = t.grown(2)                                                       # need 5: max(5, 2 * 3)
    assert t.depth == 6 and _rows(t1) == own(seeds, 6) and t.grown(3) is None
    assert t.reseed_live(seeds2) is None and not t.needs_host_reset()        # no cursors: no episode runs
    cur = np.array([[2, 1], [4, 6]])
    _, t2 = t.reseed_live(seeds2, cursor=cur)
    spliced = lambda n: [a[:k] + b[:n - k] for a, b, k in zip(own(seeds, n), own(seeds2, n), cur.reshape(-1).tolist())]      # noqa: E731
    assert _rows(t2) == spliced(6) and t.needs_host_reset() and t.seeds is seeds
    _, t3 = t.grown(10)
    assert t.depth == 13 and _rows(t3) == spliced(13)
    _, t4 = t.new_episode()                                                  # the configured seeds again, at the depth the tape has now
    assert _rows(t4) == own(seeds, 13) and not t.needs_host_reset()
    t.stage_seed(seeds2)
    assert _rows(t.new_episode()[1]) == own(seeds2, 13)


def test_continued_tape():
    """rand_episodes=True: every episode continues the movement streams behind the triples the last one consumed, positions from the
    position streams; a live re-seed restarts both and the new seeds stay."""
    from deepcomp_amd import tape
    seeds, seeds2 = np.array([42, 20042]), np.array([977, 20977])
    t = tape.draw_tape(None, seeds, 3, 1, GEOMETRY, BORDER, rand_episodes=True)
    assert type(t) is tape.ContinuedTape and not t.started and t.needs_host_reset()
    own = lambda s, n, skip: [_seq(e + 100 * (i + 1), n, VR[i], BORDER[i], k) for (e, i), k in      # noqa: E731
                              zip([(e, i) for e in s.tolist() for i in range(2)], skip)]
    pos = lambda s, nth: [_pos(e + 100 * (i + 1), INIT[i], nth) for e in s.tolist() for i in range(2)]       # noqa: E731
    p0, t0 = t.new_episode()
    assert t.started and p0.tolist() == pos(seeds, 0) and _rows(t0) == own(seeds, 3, [0] * 4)
    _, t1 = t.grown(4)                                                       # need 7: max(7, 6)
    assert t.depth == 7 and _rows(t1) == own(seeds, 7, [0] * 4)
    p2, t2 = t.new_episode(cursor=np.array([[2, 0], [7, 3]]))                # consumed in episode 0
    assert p2.tolist() == pos(seeds, 1) and _rows(t2) == own(seeds, 7, [2, 0, 7, 3])
    cur = np.array([[1, 0], [3, 7]])
    _, t3 = t.reseed_live(seeds2, cursor=cur)
    assert t.seeds is seeds2
    assert _rows(t3) == [a[:k] + b[:7 - k] for a, b, k in zip(_rows(t2), own(seeds2, 7, [0] * 4), cur.reshape(-1).tolist())]
    _, t4 = t.grown(7)                                                       # need 10: max(10, 14)
    assert t.depth == 14 and _rows(t4) == [a[:k] + b[:14 - k] for a, b, k in zip(_rows(t2), own(seeds2, 14, [0] * 4), cur.reshape(-1).tolist())]
    p5, t5 = t.new_episode(cursor=np.array([[4, 0], [3, 9]]))                # 3, 0, 0 and 2 triples of the NEW streams were consumed
    assert p5.tolist() == pos(seeds2, 0) and _rows(t5) == own(seeds2, 14, [3, 0, 0, 2])
    # a live re-seed before the first episode: that episode simply starts the new streams; a staged seed starts over as well
    t = tape.draw_tape(None, seeds, 3, 1, GEOMETRY, BORDER, rand_episodes=True)
    assert t.reseed_live(seeds2) is None and t.seeds is seeds2
    assert _rows(t.new_episode()[1]) == own(seeds2, 3, [0] * 4)
    t.stage_seed(seeds)
    assert not t.started and _rows(t.new_episode()[1]) == own(seeds, 3, [0] * 4)


@pytest.mark.parametrize('rand_episodes', [False, True])
def test_arrival_tape(rand_episodes):
    """UE arrival / departure, one env, initial UEs 1 and 2, ids 1 and 2 may arrive (rows 2 and 3: always 'slow', border 10, seeded
    seed + 100 * id).  A live re-seed seeds the UEs of the list by POSITION; reset() of a fixed-episode env does the same with the
    configured seed for the list as the episode left it, and an initial UE that has left keeps the stream it had."""
    from deepcomp_amd import tape
    s, s2 = 42, 977
    t = tape.draw_tape(None, np.array([s]), 3, 1, GEOMETRY, BORDER, rand_episodes=rand_episodes, max_id=2)
    assert type(t) is tape.ArrivalTape and not t.started and t.needs_host_reset()
    init = lambda seed, i, n, skip=0: _seq(seed, n, VR[i], BORDER[i], skip)      # noqa: E731
    p0, t0 = t.new_episode()
    assert t.started and p0.tolist() == [_pos(s + 100, INIT[0]), _pos(s + 200, INIT[1])]
    assert _rows(t0) == [init(s + 100, 0, 3), init(s + 200, 1, 3), _seq(s + 100, 3), _seq(s + 200, 3)]
    g, m = random.Random(s), random.Random(s)                                # the global generator / the map's (base.py:132-136)
    assert t.departures(1, 3).tolist() == [[g.randint(0, 2)]]
    x, y = m.randint(0, W), m.randint(0, H)
    assert t.arrivals(1).tolist() == [[list({'left': (0, y), 'right': (W - 1, y), 'top': (x, H - 1), 'bottom': (x, 0)}[m.choice(['left', 'right', 'top', 'bottom'])])]]
    _, t1 = t.grown(2)
    assert t.depth == 6 and _rows(t1) == [init(s + 100, 0, 6), init(s + 200, 1, 6), _seq(s + 100, 6), _seq(s + 200, 6)]
    # the list is now [UE 1, arrived id 1, UE 2] (4 slots); cursors 2, 1, 1
    uid = np.array([[1, 0x8001, 2, 0]], dtype=np.uint16).view(np.int16)
    _, t2 = t.reseed_live(np.array([s2]), cursor=np.array([[2, 1, 1, 0]]), uid=uid, num_ue=3, orig_consumed=np.array([[-1, -1]], dtype=np.int16))
    assert t.seeds is not s2 and t.seeds.tolist() == [s]                     # later arrivals and reset() keep the configured seed
    want = [init(s + 100, 0, 2) + init(s2 + 100, 0, 4), init(s + 200, 1, 1) + init(s2 + 300, 1, 5), _seq(s + 100, 1) + _seq(s2 + 200, 5), _seq(s + 200, 6)]
    assert _rows(t2) == want
    assert t.departures(1, 3).tolist() == [[random.Random(s2).randint(0, 2)]]             # both event generators restarted
    _, t3 = t.grown(5)                                                       # need 8: max(8, 12); the spliced rows survive
    assert t.depth == 12 and _rows(t3) == [init(s + 100, 0, 2) + init(s2 + 100, 0, 10), init(s + 200, 1, 1) + init(s2 + 300, 1, 11),
                                           _seq(s + 100, 1) + _seq(s2 + 200, 11), _seq(s + 200, 12)]
    # the episode ends with the list [UE 2, arrived id 1]: UE 1 left after 3 triples (one of its new stream), UE 2's cursor is 4
    uid = np.array([[2, 0x8001, 0, 0]], dtype=np.uint16).view(np.int16)
    p4, t4 = t.new_episode(cursor=np.array([[4, 2, 0, 0]]), uid=uid, num_ue=2, orig_consumed=np.array([[3, -1]], dtype=np.int16))
    if rand_episodes:                                                        # streams continue: UE 2 used 3 triples of its new stream
        assert p4.tolist() == [_pos(s2 + 100, INIT[0]), _pos(s2 + 300, INIT[1])]
        assert _rows(t4)[:2] == [init(s2 + 100, 0, 12, 1), init(s2 + 300, 1, 12, 3)]
    else:                                                                    # UE 2 stands first in the list: seed + 100; UE 1 is not listed
        assert p4.tolist() == [_pos(s2 + 100, INIT[0]), _pos(s + 100, INIT[1])]
        assert _rows(t4)[:2] == [init(s2 + 100, 0, 12, 1), init(s + 100, 1, 12)]
        assert t.departures(1, 3).tolist() == [[random.Random(s).randint(0, 2)]]
    assert _rows(t4)[2:] == [_seq(s + 100, 12), _seq(s + 200, 12)]                      # arriving ids: the configured seed, no splice left
    # before the first episode a live re-seed is the configured seed of a rand_episodes env only
    t = tape.draw_tape(None, np.array([s]), 3, 1, GEOMETRY, BORDER, rand_episodes=rand_episodes, max_id=2)
    seeds2 = np.array([s2])
    assert t.reseed_live(seeds2) is None and (t.seeds is seeds2) == rand_episodes


def test_each_idea_is_stated_once():
    """What the tape's owner and the decoders replaced does not come back: one shift for the cursor, the uid masks in tape.uid_fields only,
    one dcomp_set_tape / DcompPolicy / DcompOut site, one row-drawing loop, no source ladder in env.py."""
    import os
    import re
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'deepcomp_amd')
    src = {f: open(os.path.join(pkg, f)).read() for f in os.listdir(pkg) if f.endswith('.py')}
    count = lambda pat, files=src: {f: len(re.findall(pat, src[f])) for f in files if re.search(pat, src[f])}      # noqa: E731
    assert count(r'>> 48') == {'env.py': 1}
    assert count(r'0x7FFF\b') == {'tape.py': 1} and count(r'0x8000\b') == {'tape.py': 1}
    assert count(r'\.dcomp_set_tape\(', ['env.py', 'tape.py', 'rng.py']) == {'env.py': 1}
    assert count(r'\bDcompPolicy\(', ['env.py']) == {'env.py': 1} and count(r'\bDcompOut\(', ['env.py']) == {'env.py': 1}
    assert count(r'randint\(self\.border', ['rng.py']) == {} and count(r'randint\(border', ['rng.py']) == {'rng.py': 2}
    assert count(r'_dyn_streams|\b_streams\b|_fixed_tape|\b_live\b|_tape_depth_now', ['env.py']) == {}
