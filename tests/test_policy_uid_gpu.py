"""GPU tests of the policy set keyed by UE id (include/dcomp_policy_set_uid.h; deepcomp_amd.policy_set.PerIdActor / PerIdLearner /
policy_rows_by_id; sampler.collect(by_ue=True) with such a set).

The reference is what the project already holds to the float64 model: a member's own FcnetActor launch, the slot-keyed set, the
PPOLearner on given rows.  So every comparison is EXACT -- a row that goes through member id - 1 in the set's launch must come out as in
that member's own launch over the same batch, bit for bit, at the same address -- and slots without a policy hold zeros.

Shapes (tests/policy_uid_cases.py): B = 5; hidden 32 and 64 (MT 1 and 2) and 256 once; the schedule of tests/gae_uid_cases.py over a
horizon of 6, which lists ids up to U0 + 3 in U0 + 2 slots; E = 40 (one full env group and a partial one) and U0 = 66 with E = 4 (an env
wider than a wavefront, uid rows longer than one pass of the lanes)."""
import ctypes

import numpy as np
import pytest

from tests import fcnet_support as fs
from tests import gae_uid_cases as gc
from tests import guard
from tests import policy_uid_cases as pc
from tests.fcnet_cases import HYPER
from tests.fcnet_support import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

B = pc.B


def _packed(torch, obs, U):
    from deepcomp_amd.fragment import FragmentCodec
    return FragmentCodec(U, B).pack(obs.contiguous()).clone()


# ---------------------------------------------------------------------------------------------- 1: the static layout
@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
@pytest.mark.parametrize('H,act', [(32, 'tanh'), (64, 'relu')], ids=['h32', 'h64'])
def test_static_layout_equals_the_slot_keyed_set(torch_cuda, H, act, compact):
    """P = U members on a static env: the set by id with the words 1 ... U and the slot-keyed set with the identity map write the
    same bits -- sampled and arg-max, row_base != 0, with and without a value, and the value-only call."""
    torch = torch_cuda
    from deepcomp_amd.policy_set import PerIdActor, PerUEActor, static_uid_words
    E, U = 40, 5
    env = fs.env('multi', E, U, B)
    env.reset()
    g = torch.Generator(device='cuda').manual_seed(5)
    for _ in range(2):
        env.step(torch.randint(0, B + 1, (E, U), generator=g, device='cuda', dtype=torch.uint8))
    obs = _packed(torch, env.obs, U) if compact else env.obs.clone()
    mem = pc.members(U, H, act, U)
    by_id, by_slot = PerIdActor(mem), PerUEActor(mem)
    assert by_slot.slot_policy == list(range(U)) and by_id.num_policies == U and not isinstance(by_id, PerUEActor)
    assert by_id.member_of_id(3) is mem[2] and by_id.weights[1] is mem[1].weights and by_id.value_weights[4] is mem[4].value_weights
    uid = static_uid_words(E, U, 'cuda')
    assert uid.shape == (E, U) and uid.dtype == torch.int16 and uid.is_contiguous() and uid[7].tolist() == [1, 2, 3, 4, 5]
    assert static_uid_words(3, U, 'cuda').data_ptr() == uid.data_ptr()                 # held once
    for mode, kw in (('av', dict(sample=True, seed=7, step=3)), ('av', dict(sample=False)), ('a', dict(sample=True, seed=7, step=3)),
                     ('a', dict(sample=False)), ('av', dict(sample=True, seed=0x123456789, step=5, row_base=3 * U)), ('v', {})):
        pc.same(torch, pc.launch(torch, by_id, obs, compact, mode, uid=uid, **kw), pc.launch(torch, by_slot, obs, compact, mode, **kw))
    # act() on the static env takes the constant words itself
    assert torch.equal(by_id.act(env, sample=True), by_slot.act(env, sample=True))


# ---------------------------------------------------------------------------------------------- 2, 3: the dynamic layout
@pytest.mark.parametrize('U0,E,H,act,compact', pc.DYN_CASES, ids=pc.DYN_IDS)
def test_dynamic_layout_equals_each_members_own_launch(torch_cuda, U0, E, H, act, compact):
    """Nine steps over the horizon of six.  At every step every live row equals, in all four outputs, the row of member id - 1's own
    FcnetActor.actions over the same observations with the same seed and step; every dead slot holds 0 where the outputs held NaN;
    and with NaN in the observation rows of the dead slots the launch writes the same bits again."""
    torch = torch_cuda
    from deepcomp_amd.policy_set import PerIdActor
    env = pc.dyn_env(E, U0)
    U = env.U
    assert env.dynamic and U == U0 + 2 and env.max_id == U0 + 3 and env.max_id > env.U and env.schedule == pc.SCHEDULE
    P = env.max_id
    pset = PerIdActor(pc.members(U, H, act, P))
    env.reset()
    empty_tile = departure = arrival = any_dead = False
    for t in range(pc.STEPS):
        uid = env.uid.view(E, U).clone()
        obs = _packed(torch, env.obs, U) if compact else env.obs.clone()
        kw = dict(sample=True, seed=env.seed_value, step=env.time + max(env.episode, 0) * env.episode_length, row_base=env.env_id_base * U)
        got = pc.launch(torch, pset, obs, compact, 'av', uid=uid, **kw)
        ids = pc.ids_of(torch, uid)
        for p, m in enumerate(pset.members):
            rows = torch.nonzero(ids == p + 1).reshape(-1)
            if rows.numel():
                pc.same(torch, got, pc.launch(torch, m, obs, compact, 'av', **kw), rows=rows)
        dead = torch.nonzero(ids == 0).reshape(-1)
        assert int((ids > P).sum()) == 0
        any_dead = any_dead or dead.numel() > 0
        pc.all_zero(torch, got, dead)
        assert bool(torch.isfinite(got['logits']).all()) and bool(torch.isfinite(got['vf']).all())
        again = pc.launch(torch, pset, pc.poison_dead(torch, obs, uid, compact, U), compact, 'av', uid=uid, **kw)
        pc.same(torch, again, got)
        pc.same(torch, pc.launch(torch, pset, obs, compact, 'v', uid=uid), {'vf': got['vf']})
        listed = torch.stack([(ids.view(E, U) == p + 1).any(1) for p in range(P)], 1)                       # [E, P]
        empty_tile = empty_tile or any(not bool(listed[g0:g0 + 32, p].any()) for g0 in range(0, E, 32) for p in range(P))
        # act() is the same launch, from the env's own words
        assert torch.equal(pset.act(env, sample=True, obs=obs, compact=compact), got['act'].view(E, U))
        env.step(got['act'].view(E, U))
        after = env.uid.view(E, U)
        gone = [set(a) - set(b) - {0} for a, b in zip(uid.tolist(), after.tolist())]
        new = [set(b) - set(a) - {0} for a, b in zip(uid.tolist(), after.tolist())]
        departure, arrival = departure or any(gone), arrival or any(new)
        if env.time >= env.episode_length:
            env.reset()
    env.check()
    assert empty_tile and departure and arrival and any_dead


@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_equal_members_equal_the_shared_policy(torch_cuda, compact):
    torch = torch_cuda
    from deepcomp_amd.policy_set import PerIdActor
    E, U0, H = 40, 5, 32
    env, twin = pc.dyn_env(E, U0), pc.dyn_env(E, U0)
    U = env.U
    pset, single = PerIdActor(pc.members(U, H, 'tanh', env.max_id, same=True)), pc.member(U, H, 'tanh', 10)
    env.reset(); twin.reset()
    for t in range(pc.STEPS):
        live = torch.nonzero(env.uid != 0).reshape(-1)
        obs = _packed(torch, env.obs, U) if compact else None
        got, want = pc.fresh(torch, E, pset, 'av'), pc.fresh(torch, E, single, 'av')
        for actor, e, o in ((pset, env, got), (single, twin, want)):
            actor.act(e, sample=True, obs=obs, compact=compact, out=o['act'].view(E, U), logp=o['logp'], vf=o['vf'], logits=o['logits'])
        pc.same(torch, got, want, rows=live)
        pc.all_zero(torch, got, torch.nonzero(env.uid == 0).reshape(-1))
        for e in (env, twin):
            e.step(got['act'].view(E, U))
            if e.time >= e.episode_length:
                e.reset()
        assert torch.equal(env.obs.view(torch.int32), twin.obs.view(torch.int32)) and torch.equal(env.uid, twin.uid)


# ---------------------------------------------------------------------------------------------- 4: guard bands
@pytest.mark.parametrize('phase', [0, 4], ids=['phase0', 'phase4'])
def test_guard_bands_and_every_word_written(torch_cuda, phase):
    """The four outputs carved out of guarded, pattern-filled storage at two phases of a 16-byte line (the action bytes at phase and
    phase + 1): after the launch the guards are intact and no unit of any output still holds the fill -- live rows, dead slots, and
    with two members fewer than ids the rows beyond the set."""
    torch = torch_cuda
    from deepcomp_amd.policy_set import PerIdActor
    E, U0, H = 40, 5, 32
    env = pc.dyn_env(E, U0)
    U = env.U
    mem = pc.members(U, H, 'tanh', env.max_id)
    env.reset()
    env.step(torch.zeros((E, U), dtype=torch.uint8, device='cuda'))
    env.step(torch.zeros((E, U), dtype=torch.uint8, device='cuda'))                    # 7 listed: ids 1 ... 7
    uid, obs = env.uid.view(E, U).clone(), env.obs.clone()
    for pset in (PerIdActor(mem), PerIdActor(mem[:5])):
        for mode in ('av', 'a', 'v'):
            carved = []

            def carve(n, dtype):
                carved.append(guard.carve(n, dtype, 'cuda', phase_bytes=phase + (1 if dtype == torch.uint8 else 0)))
                return carved[-1]
            out = pc.fresh(torch, E, pset, mode, carve=carve)
            L = pset._L
            run = _run(E, U, sample=1, logits=out.get('logits'), logp=out.get('logp'))
            rc = L.dcomp_policy_set_actions_uid(pset._h, ctypes.byref(run), obs.data_ptr(), uid.data_ptr(), out['act'].data_ptr() if 'act' in out else None,
                                                out['vf'].data_ptr() if 'vf' in out else None, None)
            assert rc == 0, L.dcomp_last_error()
            torch.cuda.synchronize()
            for c in carved:
                guard.assert_guards(c, f'{mode} {c.dtype}')
                guard.assert_all_written(c, f'{mode} {c.dtype}')


# ---------------------------------------------------------------------------------------------- 5: ids above P, the host checks
def _run(E, U, sample=0, logits=None, logp=None, num_active=None, size=None):
    from deepcomp_amd import _lib
    return _lib.DcompActorRun(ctypes.sizeof(_lib.DcompActorRun) if size is None else size, 0, E, U if num_active is None else num_active, sample, 0, 0, 0,
                              logits.data_ptr() if logits is not None else None, logp.data_ptr() if logp is not None else None)


def test_ids_above_the_set_get_zeros_at_the_c_surface_and_raise_in_python(torch_cuda):
    torch = torch_cuda
    from deepcomp_amd.policy_set import PerIdActor
    from deepcomp_amd.sampler import collect
    E, U0, H = 40, 5, 32
    env = pc.dyn_env(E, U0)
    U = env.U
    mem = pc.members(U, H, 'tanh', env.max_id)
    whole, small = PerIdActor(mem), PerIdActor(mem[:5])
    env.reset()
    for _ in range(2):
        env.step(torch.zeros((E, U), dtype=torch.uint8, device='cuda'))
    uid, obs = env.uid.view(E, U).clone(), env.obs.clone()
    ids = pc.ids_of(torch, uid)
    beyond, within = torch.nonzero(ids > 5).reshape(-1), torch.nonzero((ids >= 1) & (ids <= 5)).reshape(-1)
    assert beyond.numel() == 2 * E and within.numel() == 5 * E
    want = pc.launch(torch, whole, obs, False, 'av', uid=uid, sample=True, seed=3, step=1)
    got = pc.fresh(torch, E, small, 'av')
    L = small._L
    run = _run(E, U, sample=1, logits=got['logits'], logp=got['logp'])
    run.seed, run.step = 3, 1
    assert L.dcomp_policy_set_actions_uid(small._h, ctypes.byref(run), obs.data_ptr(), uid.data_ptr(), got['act'].data_ptr(), got['vf'].data_ptr(), None) == 0
    torch.cuda.synchronize()
    pc.same(torch, got, want, rows=within)
    pc.all_zero(torch, got, beyond)
    pc.all_zero(torch, got, torch.nonzero(ids == 0).reshape(-1))
    assert bool(want['logits'][beyond].any())
    for call in (lambda: small.act(env), lambda: collect(env, small, 3, by_ue=True)):
        with pytest.raises(ValueError, match=r'(?s)\b8\b.*\b5 policies'):
            call()
    with pytest.raises(ValueError, match='by_ue=True'):
        collect(fs.env('multi', 4, U, B), whole, 3)
    with pytest.raises(ValueError):
        small.member_of_id(6)


def test_host_checks_of_the_entry_point(torch_cuda):
    """With a real set and pointers that are never dereferenced: each refusal returns its code and names the function, in
    actor_launch's order and then uid, num_active, action and vf; nothing reaches the device (the outputs keep their fill)."""
    torch = torch_cuda
    from deepcomp_amd import _lib
    from deepcomp_amd.policy_set import PerIdActor
    E, U, H = 4, 7, 32
    pset = PerIdActor(pc.members(U, H, 'tanh', 3))
    novalue = PerIdActor([pc.member(U, H, 'tanh', 1, value=False)])
    L, err = pset._L, pset._L.dcomp_last_error
    name, fake = b'dcomp_policy_set_actions_uid:', 4096
    out = pc.fresh(torch, E, pset, 'av')
    call = lambda s, r, obs=fake, uid=fake, action=fake, vf=fake: L.dcomp_policy_set_actions_uid(s._h, ctypes.byref(r), obs, uid, action, vf, None)      # noqa: E731
    assert call(pset, _run(E, U), obs=None) == _lib.EINVAL and name in err() and b'obs' in err()
    r = _run(E, U, logits=out['logits'])
    assert call(pset, r, action=None) == _lib.EINVAL and name in err() and b'value-only' in err()
    assert call(novalue, _run(E, U)) == _lib.EINVAL and name in err() and b'no value function' in err()
    assert call(pset, _run(0, U)) == _lib.EINVAL and name in err() and b'num_envs' in err()
    assert call(pset, _run(E, U, num_active=U + 1)) == _lib.EINVAL and name in err() and b'num_active' in err()
    assert call(pset, _run(E, U), uid=None) == _lib.EINVAL and name in err() and b'uid' in err()
    assert call(pset, _run(E, U, num_active=U + 1), uid=None) == _lib.EINVAL and b'outside' in err()      # (the run's range comes first)
    for n in (0, U - 1):
        assert call(pset, _run(E, U, num_active=n)) == _lib.EINVAL and name in err() and b'num_ue' in err()
    assert call(pset, _run(E, U, num_active=U - 1), uid=None) == _lib.EINVAL and b'uid must not be NULL' in err()
    assert call(pset, _run(E, U), action=None, vf=None) == _lib.EINVAL and name in err() and b'both NULL' in err()
    assert call(novalue, _run(E, U), action=None, vf=None) == _lib.EINVAL and b'both NULL' in err()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(out[k]).all()) for k in ('logits', 'logp', 'vf')) and bool((out['act'] == 0xEE).all())
    # Python's own: the uid tensor
    obs = torch.zeros((E, U, 4 * B + 1), device='cuda')
    for bad in (torch.zeros((E, U), dtype=torch.int32, device='cuda'), torch.zeros((E, U - 1), dtype=torch.int16, device='cuda'),
                torch.zeros((E, U), dtype=torch.int16), torch.zeros((E, 2 * U), dtype=torch.int16, device='cuda')[:, ::2], None):
        with pytest.raises(ValueError, match='uid'):
            pset.actions(obs, uid=bad)
    with pytest.raises(ValueError):
        novalue.value(obs, uid=torch.zeros((E, U), dtype=torch.int16, device='cuda'))
    # a member that gets its value function after the set exists: refused for this entry as for the others
    novalue.members[0].set_value(_value_weights(U, H))
    assert call(novalue, _run(E, U), vf=None) == _lib.EINVAL and name in err() and b'after the set was created' in err()


def _value_weights(U, H):
    from deepcomp_amd.actor import FcnetActor
    return FcnetActor.random_value_weights('multi', U, B, H, seed=3)


# ---------------------------------------------------------------------------------------------- 6: collect
@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_collect_by_ue_with_a_set_by_id_matches_the_plain_loop(torch_cuda, compact):
    """T = 9 over the horizon of 6, then a second batch into the same buffers that ends on a boundary (no bootstrap)."""
    torch = torch_cuda
    from deepcomp_amd.policy_set import PerIdActor
    from deepcomp_amd.sampler import collect
    E, U0, H, T = 16, 5, 32, pc.STEPS
    env, twin = pc.dyn_env(E, U0), pc.dyn_env(E, U0)
    actor = PerIdActor(pc.members(env.U, H, 'tanh', env.max_id))
    b = collect(env, actor, T, gamma=gc.GAMMA, lam=gc.LAM, compact=compact, dist_inputs=True, by_ue=True)
    dones, live = pc.check_batch(torch, env, twin, actor, b, T, compact, started=False)
    assert dones.tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0] and int(live.sum()) == 44 * E
    # the bootstrap went through each UE's own value trunk: with the words of a static layout it would differ
    last = b['new_obs_last']
    assert not torch.equal(actor.value(last, uid=actor.uid_of(env).flip(1).contiguous(), compact=compact), b['last_vf'])
    b2 = collect(env, actor, T, gamma=gc.GAMMA, lam=gc.LAM, compact=compact, dist_inputs=True, by_ue=True, out=b)
    dones, _ = pc.check_batch(torch, env, twin, actor, b2, T, compact, started=True)
    assert b2 is b and dones.tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 1]
    env.check(); twin.check()


# ---------------------------------------------------------------------------------------------- 7: the learner
_LEARN = {}


def _learn_case(torch, compact):
    """(env shape, the batch a set of distinct members collected, its rows per policy), collected once per format and left unchanged."""
    if compact not in _LEARN:
        from deepcomp_amd.policy_set import PerIdActor, policy_rows_by_id
        from deepcomp_amd.sampler import collect
        E, U0, H, T = 16, 5, 32, pc.STEPS
        env = pc.dyn_env(E, U0)
        batch = collect(env, PerIdActor(pc.members(env.U, H, 'tanh', env.max_id + 1)), T, gamma=gc.GAMMA, lam=gc.LAM, compact=compact, dist_inputs=True, by_ue=True)
        _LEARN[compact] = (env.U, env.max_id + 1, H, batch, policy_rows_by_id(batch, env.max_id + 1))
    return _LEARN[compact]


def _per_id(U, H, P, max_rows=64):
    from deepcomp_amd.policy_set import PerIdActor, PerIdLearner
    return PerIdLearner(PerIdActor(pc.members(U, H, 'tanh', P)), max_rows=max_rows, **dict(HYPER, lr=1e-3))


@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_per_id_update_is_each_members_own_update_on_its_rows(torch_cuda, compact):
    torch = torch_cuda
    from deepcomp_amd.learner import PPOLearner
    from deepcomp_amd.policy_set import policy_rows_by_id_reference
    from deepcomp_amd.sampler import live_rows
    U, P, H, batch, rows = _learn_case(torch, compact)
    ref = policy_rows_by_id_reference(batch, P)
    assert len(rows) == P and all(r.dtype == torch.int64 and r.is_cuda and np.array_equal(r.cpu().numpy(), w) for r, w in zip(rows, ref))
    assert torch.equal(torch.sort(torch.cat(rows)).values, live_rows(batch))
    assert rows[P - 1].numel() == 0 and all(r.numel() for r in rows[:P - 2])           # one id beyond env.max_id: a policy without rows
    learner = _per_id(U, H, P)
    before = learner.learners[P - 1].state_dict()
    stats = learner.update(batch, num_sgd_iter=2, minibatch_rows=64, seed=4)
    assert len(stats) == P and stats[P - 1] is None
    fs.same_state(learner.learners[P - 1].state_dict(), before)
    assert learner.learners[P - 1].state_dict()['step'] == 0
    for p in range(P):
        if rows[p].numel() == 0:
            assert stats[p] is None
            continue
        twin = PPOLearner(pc.member(U, H, 'tanh', 10 + p), max_rows=64, **dict(HYPER, lr=1e-3))
        want = twin.update(batch, num_sgd_iter=2, minibatch_rows=64, seed=4 + p, rows=rows[p])
        assert stats[p] == want and all(np.isfinite(v) for v in want.values()) and 'kl_coeff' in want
        fs.same_state(learner.learners[p].state_dict(), twin.state_dict(), stepped=True)
    assert len(learner.state_dict()) == P and len(learner.to_rllib_weights()) == P


@pytest.mark.parametrize('micro,clip', [(False, None), (True, None), (True, 0.5)], ids=['plain', 'micro', 'micro-clip'])
def test_grouped_update_equals_the_sequential_one(torch_cuda, micro, clip):
    """micro_rows is a weight-gradient chunk, the smallest micro-batch there is: a policy's minibatch of 64 rows is one micro-batch, and
    goes through the accumulators -- zero, accumulate, finish with the clip, apply."""
    torch = torch_cuda
    from deepcomp_amd.learner import chunk_unit
    U, P, H, batch, rows = _learn_case(torch, True)
    kw = dict(micro_rows=chunk_unit(), grad_clip=clip) if micro else {}
    seq, grp = (_per_id(U, H, P, chunk_unit() if micro else 64) for _ in range(2))
    want = seq.update(batch, num_sgd_iter=2, minibatch_rows=64, seed=4, **kw)
    got = grp.update(batch, num_sgd_iter=2, minibatch_rows=64, seed=4, grouped=True, **kw)
    fs.same_run(got, want, grp, seq)
    assert got[P - 1] is None and grp.learners[P - 1].state_dict()['step'] == 0 and sum(g is not None for g in got) >= P - 2


def test_on_a_static_env_the_learner_by_id_is_the_learner_by_slot(torch_cuda):
    torch = torch_cuda
    from deepcomp_amd.policy_set import PerIdActor, PerIdLearner, PerUEActor, PerUELearner
    from deepcomp_amd.sampler import collect
    E, U, H, T = 16, 5, 32, pc.STEPS
    hyper = dict(HYPER, lr=1e-3)
    by_id = PerIdLearner(PerIdActor(pc.members(U, H, 'tanh', U)), max_rows=64, **hyper)
    by_slot = PerUELearner(PerUEActor(pc.members(U, H, 'tanh', U)), max_rows=64, **hyper)
    b_id = collect(fs.env('multi', E, U, B), by_id.actor, T, gamma=gc.GAMMA, lam=gc.LAM, dist_inputs=True, by_ue=True)
    b_slot = collect(fs.env('multi', E, U, B), by_slot.actor, T, gamma=gc.GAMMA, lam=gc.LAM, dist_inputs=True)
    for k, t in b_slot.items():
        assert torch.equal(b_id[k].view(torch.uint8), t.view(torch.uint8)), k
    for grouped in (False, True):
        got = by_id.update(b_id, num_sgd_iter=2, minibatch_rows=64, seed=4, grouped=grouped)
        want = by_slot.update(b_slot, num_sgd_iter=2, minibatch_rows=64, seed=4, grouped=grouped)
        fs.same_run(got, want, by_id, by_slot)


# ---------------------------------------------------------------------------------------------- 8: refusals
def test_refusals(torch_cuda):
    from deepcomp_amd.policy_set import PerIdActor, PerIdLearner, PerUEActor, PerUELearner
    U, H = 7, 32
    central = pc.member(U, H, 'tanh', 1, value=False, kind='central')
    with pytest.raises(NotImplementedError, match='CENTRAL'):
        PerIdActor([central, central])
    shared = pc.member(U, H, 'tanh', 1, shared=True)
    with pytest.raises(NotImplementedError, match='shared'):
        PerIdActor([shared, shared])
    with pytest.raises(ValueError):
        PerIdActor([])
    with pytest.raises(ValueError):
        PerIdActor([pc.member(U, H, 'tanh', 1), pc.member(U, 64, 'tanh', 2)])
    mem = pc.members(U, H, 'tanh', 2)
    by_id, by_slot = PerIdActor(mem), PerUEActor(mem)
    with pytest.raises(ValueError, match='PerIdActor'):
        PerIdLearner(by_slot)
    with pytest.raises(ValueError, match='PerUEActor'):
        PerUELearner(by_id)
    with pytest.raises(ValueError):
        PerIdLearner(PerIdActor([mem[0], mem[0]]))                                     # the same actor twice
    learner = PerIdLearner(by_id, max_rows=64, **dict(HYPER, lr=1e-3))
    with pytest.raises(ValueError, match='by_ue=True'):
        learner.update({'actions': None})
    with pytest.raises(NotImplementedError, match='data-parallel'):
        learner.rows_of(64)                                                            # what DataParallelPerUELearner splits a batch with
