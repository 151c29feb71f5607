"""GPU tests of the per-UE policy set (include/dcomp_policy_set.h; deepcomp_amd.policy_set.PerUEActor / PerUELearner; PPOLearner.update(rows=)).

The reference is the existing shared-policy kernel and learner, which other tests hold to the float64 model, so every comparison here
is EXACT (torch.equal on the outputs, np.array_equal on learner states): a decision row that goes through member p's weights in the
set's launch must come out as in member p's own launch over the same batch, bit for bit, at the same address.

Three shapes, the smallest that reach every path of the kernel:
  (a) U 5, B 3, hidden 32 tanh, E 70: three tiles per slot, the last with 6 rows, E % 32 != 0
  (b) U 3, B 36, hidden 64 relu, E 33: two connection words per UE in the compact record, 145 inputs = two staging chunks, a last tile of 1 row
  (c) U 4, B 10, hidden 256 tanh, E 40: the widest instantiation
Observations come from a real env (reset + 3 random steps), computed once per shape and left unchanged."""
import ctypes

import numpy as np
import pytest

from tests import fcnet_cases as fc
from tests import fcnet_support as fs
from tests.fcnet_cases import HYPER
from tests.fcnet_support import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SHAPES, SLOTS, GUARD = fc.SET_SHAPES, fc.SET_SLOTS, fc.SET_GUARD
FORMATS = [('a', False), ('a', True), ('b', False), ('b', True), ('c', False)]
FORMAT_IDS = ['a-rows', 'a-compact', 'b-rows', 'b-compact', 'c-rows']


_OBS = {}


def _obs(torch, name):
    """{False: observation rows [E, U, 4B+1], True: the compact record [E, words]} of shape `name`."""
    if name not in _OBS:
        from deepcomp_amd.fragment import FragmentCodec
        U, B, _, _, E = SHAPES[name]
        env = fs.env('multi', E, U, B)
        env.reset()
        g = torch.Generator(device='cuda').manual_seed(5)
        for _ in range(3):
            env.step(torch.randint(0, B + 1, (E, U), generator=g, device='cuda', dtype=torch.uint8))
        rows = env.obs.clone()
        codec = FragmentCodec(U, B)
        packed = codec.pack(rows).clone()
        codec.check()
        _OBS[name] = {False: rows, True: packed}
    return _OBS[name]


VARIANTS = [(mode, sample) for mode in ('a', 'av') for sample in (True, False)] + [('v', False)]


def _kw(mode, sample):
    return {} if mode == 'v' else dict(sample=sample, seed=7, step=3)


# ---------------------------------------------------------------------------------------------- 1, 4: equal members, guard bands
@pytest.mark.parametrize('name,compact', FORMATS, ids=FORMAT_IDS)
def test_equal_members_reproduce_the_shared_policy(torch_cuda, name, compact):
    """P = U members built from one set of weights: actions, logits, logp and vf of the set equal FcnetActor's on the same
    observations -- sampled and greedy, with and without vf, and the value-only call.  On (a) every output also has a guard band
    behind it, which must be intact after every variant."""
    torch = torch_cuda
    from deepcomp_amd.policy_set import PerUEActor
    U = SHAPES[name][0]
    obs = _obs(torch, name)[compact]
    single = fs.set_member(name, 1)
    both = PerUEActor([fs.set_member(name, 1) for _ in range(U)])
    assert both.slot_policy == list(range(U)) and both.value_weights is not None and len(both.members) == U
    for mode, sample in VARIANTS:
        want = fs.set_run(torch, single, obs, compact, mode, **_kw(mode, sample))
        got = fs.set_run(torch, both, obs, compact, mode, guard=GUARD if name == 'a' else 0, **_kw(mode, sample))
        fs.set_same(torch, got, want)
    novalue = PerUEActor([fs.set_member(name, 1, value=False) for _ in range(U)])
    assert novalue.value_weights is None
    fs.set_same(torch, fs.set_run(torch, novalue, obs, compact, 'a', **_kw('a', True)), fs.set_run(torch, single, obs, compact, 'a', **_kw('a', True)))


# ---------------------------------------------------------------------------------------------- 2: distinct members
@pytest.mark.parametrize('name,compact', FORMATS, ids=FORMAT_IDS)
def test_every_slot_runs_its_own_member(torch_cuda, name, compact):
    """slot_policy [0, 1, 1, 0, 1] on (a), identity on (b) and (c): for every slot u the set's outputs at rows e U + u equal those of
    member slot_policy[u] run alone over the whole batch, at the same rows; again with row_base = 3 U and another step and seed."""
    torch = torch_cuda
    U, _, _, _, E = SHAPES[name]
    sp = SLOTS[name]
    obs = _obs(torch, name)[compact]
    pset = fs.set_distinct(name)
    slot_rows = [torch.arange(E, device='cuda') * U + u for u in range(U)]
    for kw in (dict(sample=True), dict(sample=True, row_base=3 * U, step=5, seed=0x123456789), dict(sample=False)):
        got = fs.set_run(torch, pset, obs, compact, 'av', **kw)
        alone = [fs.set_run(torch, m, obs, compact, 'av', **kw) for m in pset.members]
        for u in range(U):
            fs.set_same(torch, got, alone[sp[u]], rows=slot_rows[u])
        # the comparison discriminates: on the rows of slot 1 the members of slots 0 and 1 disagree, so a kernel that ignored the
        # table could not have matched both
        assert sp[0] != sp[1]
        for k in ('logits', 'vf'):
            x, y = (alone[sp[s]][k].reshape(E * U, -1)[slot_rows[1]] for s in (0, 1))
            assert not torch.equal(x, y), k
    gotv = fs.set_run(torch, pset, obs, compact, 'v')
    for u in range(U):
        fs.set_same(torch, gotv, fs.set_run(torch, pset.members[sp[u]], obs, compact, 'v'), rows=slot_rows[u])


# ---------------------------------------------------------------------------------------------- 3: unlisted slots
@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_unlisted_slots_get_action_zero_and_its_logp(torch_cuda, name):
    torch = torch_cuda
    U, _, _, _, E = SHAPES[name]
    sp = SLOTS[name]
    obs = _obs(torch, name)[False]
    pset = fs.set_distinct(name)
    kw = dict(sample=True, seed=11, step=2, num_active=U - 2)
    got = fs.set_run(torch, pset, obs, False, 'av', **kw)
    for u in range(U):
        rows = torch.arange(E, device='cuda') * U + u
        fs.set_same(torch, got, fs.set_run(torch, pset.members[sp[u]], obs, False, 'av', **kw), rows=rows)
        if u >= U - 2:
            assert not bool(got['act'][:, u].any())
            lsm = torch.log_softmax(got['logits'][rows].double(), -1)[:, 0]
            assert float((got['logp'][rows, 0].double() - lsm).abs().max()) < 1e-5      # (the logp of action 0; exactness is the line above)
        else:
            assert bool(got['act'][:, u].any())


# ---------------------------------------------------------------------------------------------- 5: the set follows a member's learner
def test_the_set_runs_what_a_members_learner_wrote(torch_cuda):
    """One grads + apply on member 1's PPOLearner, no call on the set: the set's next outputs at member 1's slots equal member 1's
    own fresh launch and differ from before; every other slot is bit-identical to before."""
    torch = torch_cuda
    from deepcomp_amd.learner import PPOLearner
    name = 'a'
    U, _, _, _, E = SHAPES[name]
    sp = SLOTS[name]
    obs = _obs(torch, name)[False]
    pset = fs.set_distinct(name)
    kw = dict(sample=True, seed=3, step=1)
    before = fs.set_run(torch, pset, obs, False, 'av', **kw)
    m = pset.members[1]
    own = fs.set_run(torch, m, obs, False, 'av', **kw)
    learner = PPOLearner(m, max_rows=E * U, **dict(HYPER, lr=1e-2))
    g = torch.Generator(device='cuda').manual_seed(8)
    adv = torch.randn(E * U, generator=g, device='cuda')
    learner.grads(obs.reshape(E * U, -1), own['act'].reshape(E * U, 1), own['logp'], own['logits'], adv, own['vf'] + adv, own['vf'].clone())
    learner.apply()
    after = fs.set_run(torch, pset, obs, False, 'av', **kw)
    fresh = fs.set_run(torch, m, obs, False, 'av', **kw)
    for u in range(U):
        rows = torch.arange(E, device='cuda') * U + u
        if sp[u] == 1:
            fs.set_same(torch, after, fresh, rows=rows)
            assert not torch.equal(after['logits'][rows], before['logits'][rows]) and not torch.equal(after['vf'][rows], before['vf'][rows])
        else:
            fs.set_same(torch, after, before, rows=rows)


# ---------------------------------------------------------------------------------------------- 6: collect
_T = fc.SET_T


def _equal_batches(torch, b1, b2):
    assert b1.keys() == b2.keys()
    for k in b1:
        assert torch.equal(b1[k], b2[k]), k


@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_collect_with_a_set_of_equal_members_is_collect_with_the_shared_policy(torch_cuda, compact):
    torch = torch_cuda
    from deepcomp_amd.policy_set import PerUEActor
    from deepcomp_amd.sampler import collect
    U, B, _, _, E = SHAPES['a']
    pset = PerUEActor([fs.set_member('a', 1) for _ in range(U)])
    got = collect(fs.env('multi', E, U, B), pset, _T, gamma=0.99, lam=0.95, compact=compact, dist_inputs=True)
    want = collect(fs.env('multi', E, U, B), fs.set_member('a', 1), _T, gamma=0.99, lam=0.95, compact=compact, dist_inputs=True)
    _equal_batches(torch, got, want)
    assert bool(torch.isfinite(got['advantages']).all()) and bool(got['actions'].any())


# ---------------------------------------------------------------------------------------------- 7: PPOLearner.update(rows=)
_FLAT = {'obs': 'num_in', 'actions': 'heads', 'action_logp': 'heads', 'action_dist_inputs': 'num_logits', 'advantages': None, 'value_targets': None,
         'vf_preds': None}


def _gathered(actor, rows_batch, rows):
    """The batch dict of the source rows `rows`, gathered tensor by tensor."""
    out = {}
    for k, per in _FLAT.items():
        t = rows_batch[k].reshape(-1) if per is None else rows_batch[k].reshape(-1, getattr(actor, per))
        out[k] = t.index_select(0, rows.long()).contiguous()
    return out


def _ppo(actor, **kw):
    from deepcomp_amd.learner import PPOLearner
    return PPOLearner(actor, max_rows=64, **dict(HYPER, lr=1e-3, **kw))


@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_update_on_given_rows_is_update_on_the_gathered_batch(torch_cuda, compact):
    torch = torch_cuda
    U, _, _, _, E = SHAPES['a']
    batch, rows_batch = fs.set_batch(torch, compact)
    N = _T * E * U
    g = torch.Generator(device='cuda').manual_seed(21)
    subset = torch.randperm(N, generator=g, device='cuda')[:200].contiguous()           # distinct, in no order, across steps, envs and slots
    a, b, full = (_ppo(fs.set_member('a', 1)) for _ in range(3))
    out_a = a.update(batch, num_sgd_iter=2, minibatch_rows=64, seed=3, rows=subset)
    out_b = b.update(_gathered(b.actor, rows_batch, subset), num_sgd_iter=2, minibatch_rows=64, seed=3)
    assert out_a == out_b and all(np.isfinite(v) for v in out_a.values())
    s_a = a.state_dict()
    assert s_a['step'] == 8                                                            # 200 rows: three minibatches of 64 and one of 8, twice
    fs.same_state(s_a, b.state_dict(), stepped=True)
    c = _ppo(fs.set_member('a', 1))
    c.update(batch, num_sgd_iter=2, minibatch_rows=64, seed=3, rows=subset.to(torch.int32))      # int32 rows are the same rows
    fs.same_state(s_a, c.state_dict(), stepped=True)
    full.update(batch, num_sgd_iter=1, minibatch_rows=64, seed=3)                      # rows=None: the whole batch, as before
    assert full.state_dict()['step'] == -(-N // 64)


# ---------------------------------------------------------------------------------------------- 8, 9: PerUELearner
def _per_ue(name='a'):
    from deepcomp_amd.policy_set import PerUELearner
    pset = fs.set_distinct(name)
    return pset, PerUELearner(pset, max_rows=64, **dict(HYPER, lr=1e-3))


@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_per_ue_update_is_the_loop_over_the_members_sub_batches(torch_cuda, compact):
    torch = torch_cuda
    from deepcomp_amd.policy_set import policy_rows
    U, _, _, _, E = SHAPES['a']
    sp = SLOTS['a']
    batch, rows_batch = fs.set_batch(torch, compact)
    pset, learner = _per_ue()
    stats = learner.update(batch, num_sgd_iter=2, minibatch_rows=64, seed=4)
    assert len(stats) == 2 and all(np.isfinite(s['total_loss']) and 'kl_coeff' in s for s in stats)
    split = policy_rows(_T * E * U, U, sp, 2, 'cuda')
    assert [int(r.numel()) for r in split] == [2 * _T * E, 3 * _T * E]
    for p in range(2):                                                                 # the loop written out: fresh copies, gathered sub-batches, seed + p
        twin = _ppo(fs.set_member('a', 10 + p))
        want = twin.update(_gathered(twin.actor, rows_batch, split[p]), num_sgd_iter=2, minibatch_rows=64, seed=4 + p)
        assert stats[p] == want
        fs.same_state(learner.learners[p].state_dict(), twin.state_dict(), stepped=True)
    w = learner.get_weights()
    assert len(w) == 2 and len(learner.to_rllib_weights()) == 2 and not np.array_equal(w[0][0]['w1'], w[1][0]['w1'])
    obs = _obs(torch, 'a')[False]
    got = fs.set_run(torch, pset, obs, False, 'av', sample=True, seed=5)
    for u in range(U):
        fs.set_same(torch, got, fs.set_run(torch, pset.members[sp[u]], obs, False, 'av', sample=True, seed=5), rows=torch.arange(E, device='cuda') * U + u)


def test_checkpoint_and_resume(torch_cuda):
    """state_dict -> a new set and learner -> load_state_dict -> one more update: the state of the uninterrupted run, bit for bit."""
    torch = torch_cuda
    batch, _ = fs.set_batch(torch, True)
    _, run1 = _per_ue()
    run1.update(batch, num_sgd_iter=1, minibatch_rows=64, seed=1)
    saved = run1.state_dict()
    run1.update(batch, num_sgd_iter=1, minibatch_rows=64, seed=2)
    pset2, run2 = _per_ue()
    run2.load_state_dict(saved)
    run2.update(batch, num_sgd_iter=1, minibatch_rows=64, seed=2)
    for s1, s2 in zip(run1.state_dict(), run2.state_dict()):
        fs.same_state(s1, s2, stepped=True)
    assert len(saved) == 2 and saved[0]['step'] > 0
    with pytest.raises(ValueError):
        run2.load_state_dict(saved[:1])


# ---------------------------------------------------------------------------------------------- 10: refusals that need handles
def _c_create(members, slots=None):
    from deepcomp_amd import _lib
    L = _lib.load()
    arr = (ctypes.c_void_p * len(members))(*[m._h.value for m in members])
    sl = (ctypes.c_int32 * len(slots))(*slots) if slots is not None else None
    cfg = _lib.DcompPolicySetCfg(ctypes.sizeof(_lib.DcompPolicySetCfg), len(members), arr, sl)
    h = ctypes.c_void_p()
    rc = L.dcomp_policy_set_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = L.dcomp_last_error() if rc else b''
    if rc == 0:
        assert L.dcomp_policy_set_destroy(h) == 0
    else:
        assert h.value is None
    return rc, msg


def test_refusals_that_need_handles(torch_cuda):
    torch = torch_cuda
    from deepcomp_amd import _lib
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.policy_set import PerUEActor, PerUELearner
    U, B, H, _, E = SHAPES['a']
    base = fs.set_member('a', 1)
    differing = {'num_bs': fs.set_member('a', 2, B=B + 1), 'hidden': fs.set_member('a', 2, H=64), 'activation': fs.set_member('a', 2, activation='relu'),
                 'value function': fs.set_member('a', 2, value=False), 'num_ue': fs.set_member('a', 2, U=U + 1)}
    for field, other in differing.items():
        with pytest.raises(ValueError):
            PerUEActor([base, other])
        rc, msg = _c_create([base, base, other])
        assert rc == _lib.EINVAL and b'member 2' in msg and field.encode() in msg, (field, msg)
    central = FcnetActor.random('central', U, B, hidden=H, seed=1)
    with pytest.raises(NotImplementedError):
        PerUEActor([central, central])
    rc, msg = _c_create([central])
    assert rc == _lib.EUNSUPPORTED and b'CENTRAL' in msg
    rc, msg = _c_create([base, central])
    assert rc == _lib.EINVAL and b'obs_kind' in msg                                    # (disagreement comes before the refusal of a form)
    shared = fs.set_member('a', 1, shared=True)
    with pytest.raises(NotImplementedError):
        PerUEActor([shared, shared])
    rc, msg = _c_create([shared, shared])
    assert rc == _lib.EUNSUPPORTED and b'shared' in msg
    with pytest.raises(ValueError):
        PerUEActor([base, base], [0, 1, 2, 0, 1])                                      # an entry equal to P
    with pytest.raises(ValueError):
        PerUEActor([base, base], [0, 1, 0])                                            # not one entry per slot
    rc, msg = _c_create([base, base], [0, 1, 2, 0, 1])
    assert rc == _lib.EINVAL and b'slot_policy[2] = 2' in msg
    rc, msg = _c_create([base, base], [0, 1, -1, 0, 1])
    assert rc == _lib.EINVAL and b'slot_policy[2]' in msg
    assert _c_create([base, base], [0, 1, 1, 0, 1])[0] == _lib.OK and _c_create([base])[0] == _lib.OK

    # a real set: the run's own checks, and what only Python refuses
    pset = PerUEActor([base, base])
    obs = _obs(torch, 'a')[False]
    with pytest.raises(ValueError):
        pset.actions(obs, num_active=U + 1)
    with pytest.raises(ValueError):
        pset.actions(obs[:, :, :-1].contiguous())
    with pytest.raises(ValueError):
        pset.actions(obs, vf=torch.zeros(E * U - 1, device='cuda'))
    novalue = PerUEActor([fs.set_member('a', 1, value=False)])
    with pytest.raises(ValueError):
        novalue.actions(obs, vf=torch.zeros(E * U, device='cuda'))
    run = _lib.DcompActorRun(ctypes.sizeof(_lib.DcompActorRun), 0, E, U, 0, 0, 0, 0, None, None)
    vf = torch.zeros(E * U, device='cuda')
    L = _lib.load()
    assert L.dcomp_policy_set_actions_v(novalue._h, ctypes.byref(run), obs.data_ptr(), None, vf.data_ptr(), None) == _lib.EINVAL
    assert b'dcomp_policy_set_actions_v' in L.dcomp_last_error() and b'no value function' in L.dcomp_last_error()
    dyn = fs.env('multi', 6, 4, B, ue_arrival={2: 2, 4: -1})
    dset = PerUEActor([fs.set_member('a', 1, U=dyn.U)])
    dyn.reset()
    with pytest.raises(NotImplementedError):
        dset.act(dyn)
    with pytest.raises(ValueError):
        PerUELearner(base)
    with pytest.raises(ValueError):
        PerUELearner(pset)                                                             # the same actor twice: two Adam states on one handle
    lr = _ppo(fs.set_member('a', 1))
    with pytest.raises(ValueError):
        lr.update(fs.set_batch(torch, False)[0], num_sgd_iter=1, minibatch_rows=64, rows=torch.arange(64, device='cuda'), num_active=3)
    for bad in (torch.arange(64), torch.arange(64, device='cuda').float(), torch.tensor([0, _T * E * U], device='cuda'), torch.tensor([3, 1, -1], device='cuda'),
                torch.tensor([5, 9, 5], device='cuda'), torch.zeros(0, dtype=torch.int64, device='cuda')):
        with pytest.raises(ValueError):
            lr.update(fs.set_batch(torch, False)[0], num_sgd_iter=1, minibatch_rows=64, rows=bad)
    assert lr.state_dict()['step'] == 0


def test_a_value_function_attached_after_the_set_exists_is_refused_on_the_host(torch_cuda):
    """The set's table holds the trunks the members had at create.  Members without a value function, the set, then set_value on the
    members: the set keeps saying it has no value function, and every launch is refused before it reaches the device -- at the Python
    surface and at the C surface, with a trunk of its own and with the shared form, after one member and after all."""
    torch = torch_cuda
    from deepcomp_amd import _lib
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.policy_set import PerUEActor
    from deepcomp_amd.sampler import collect
    U, B, H, _, E = SHAPES['a']
    obs = _obs(torch, 'a')[False]
    L = _lib.load()
    run = _lib.DcompActorRun(ctypes.sizeof(_lib.DcompActorRun), 0, E, U, 0, 0, 0, 0, None, None)
    act, vf = torch.zeros((E, U), dtype=torch.uint8, device='cuda'), torch.zeros(E * U, device='cuda')
    for shared in (False, True):
        members = [fs.set_member('a', 1, value=False), fs.set_member('a', 2, value=False)]
        pset = PerUEActor(members)
        before = pset.actions(obs, sample=False).clone()
        for k, m in enumerate(members):
            m.set_value(FcnetActor.random_value_weights('multi', U, B, H, seed=3, shared=shared), shared=shared)
            assert pset.value_weights is None
            with pytest.raises(ValueError):
                pset.actions(obs, vf=vf)
            with pytest.raises(ValueError):
                pset.value(obs)
            with pytest.raises(ValueError):
                pset.actions(obs)
            with pytest.raises(ValueError):
                collect(fs.env('multi', E, U, B), pset, 2)
            for call in (lambda: L.dcomp_policy_set_actions_v(pset._h, ctypes.byref(run), obs.data_ptr(), act.data_ptr(), vf.data_ptr(), None),
                         lambda: L.dcomp_policy_set_actions_v(pset._h, ctypes.byref(run), obs.data_ptr(), None, vf.data_ptr(), None),
                         lambda: L.dcomp_policy_set_actions(pset._h, ctypes.byref(run), obs.data_ptr(), act.data_ptr(), None)):
                assert call() == _lib.EINVAL and b'got a value function after the set was created' in L.dcomp_last_error(), k
        torch.cuda.synchronize()
        if shared:
            with pytest.raises(NotImplementedError):
                PerUEActor(members)
        else:                                                                          # a new set over the same members has the value
            again = PerUEActor(members)
            assert again.value_weights is not None
            assert torch.equal(again.actions(obs, sample=False, vf=vf), before) and bool(torch.isfinite(vf).all())
