"""GPU tests of the fcnet kernels over tests/fcnet_cases.py: every instantiation of actor_kernel<MT, RELU, VF, PER>, learner_kernel<MT,
RELU, IDX>, wgrad_block<MB, NB> and wgrad_bias<NB>, and the host-side branches on shape, held to a reference.

The bars are the project's existing ones and the constructions are those of the tests that introduced them
(tests/fcnet_support.py and tests/fcnet_cases.py hold what both run):
  relu   integer data (tests/test_actor_gpu.py, test_critic_gpu.py, test_learner_gpu.py): logits, values and all twelve gradient arrays
         equal the float64 reference EXACTLY, the action is the first maximum
  tanh   random-init weights on the rows of a real env (reset + 3 steps, fs.actor_case's recipe -- the env takes every shape of the
         table, 63 and 64 stations and 1 024 UE slots included, so no case uses synthetic rows): within 2 x the error the CPU bf16 chain
         itself has against the float64 model
  sets   a slot's rows equal its member's own launch bit for bit (the member's launch is held to the reference above)
  index  grads_indexed equals grads on the gathered rows bit for bit
and two that are new: logp against float64 log-softmax of the EXACT logits at magnitudes past expf's float32 range, and the loss
epilogue alone (per-row outputs and db3 of the real loss on an exact forward pass), both inside bounds that tests/fcnet_cases.py
derives and tests/test_fcnet_matrix_cpu.py shows reachable with a float32 emulation.  Measured: profiles/r13_fcnet_matrix.txt."""
import numpy as np
import pytest

from tests import fcnet_cases as fc
from tests import fcnet_support as fs
from tests.fcnet_cases import HYPER
from tests.fcnet_support import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

IDS = [fc.sid(s) for s in fc.ACTOR_SHAPES]
LIDS = [fc.sid(s) for s in fc.LEARNER_SHAPES]


# ================================================================================================ actor and value head
def _exact(got, ref, what):
    ref = np.asarray(ref).astype(np.float32).reshape(got.shape)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f'{what}: {len(bad)} of {ref.size} differ, first at {bad[0]}: {got[tuple(bad[0])]} != {ref[tuple(bad[0])]}'


def _logp_check(shape, variant, c, act, logp, what):
    """logp of the greedy action against float64 log-softmax of the EXACT logits: (NA + 8) 2^-24 max(1, max |logit|) per head."""
    B = shape[3]
    lg = c['logits'].reshape(c['rows'], -1, B + 1)
    want = np.take_along_axis(fc.log_softmax64(lg), act.reshape(c['rows'], -1, 1).astype(np.int64), -1)[..., 0]
    err, bound = float(np.abs(logp.astype(np.float64) - want).max()), fc.lse_bound(B + 1, np.abs(lg).max())
    print(f'logp on exact logits {fc.sid(shape)} seed {variant[0]} {what}: max |logit| {np.abs(lg).max():.0f}  max abs err {err:.3e}  bound {bound:.3e}')
    assert np.isfinite(logp).all() and err <= bound, (what, err, bound)


def _relu_exact(torch, shape, variant, forms):
    """One integer variant of a shape through VF 0 (no vf asked), and per value form in `forms` VF 1 / 2 and the value-only call."""
    from deepcomp_amd.actor import FcnetActor
    kind, E, U, B, H = shape
    c = fc.actor_int_case(shape, *variant)
    rows, obs = c['rows'], torch.from_numpy(c['x']).cuda()
    first = c['logits'].reshape(rows, -1, B + 1).argmax(axis=-1)
    base = None
    for form in forms:
        actor = FcnetActor(kind, U, B, c['w'], activation='relu', value_weights=c['v'][form])
        assert actor.value_shared == (form == 'shared')
        if base is None:                                                              # VF = 0: dcomp_actor_actions
            base = fs.actor_run(torch, actor, obs, rows, sample=False)
            _exact(base[1], c['logits'], f'{form} logits without vf')
            assert np.array_equal(base[0].reshape(rows, -1), first)
            _logp_check(shape, variant, c, base[0], base[2], 'VF 0')
        vf = torch.full((rows,), float('nan'), device='cuda')
        act, logits, logp = fs.actor_run(torch, actor, obs, rows, sample=False, vf=vf)
        _exact(logits, c['logits'], f'{form} logits with vf')
        _exact(vf.cpu().numpy(), c['vf'][form], f'{form} vf')
        assert np.array_equal(act.reshape(rows, -1), first)
        assert np.array_equal(fs.bits(logp), fs.bits(base[2]))                           # (the walk is the same code on the same logits)
        only = torch.full((rows + 64,), float('nan'), device='cuda')
        actor.value(obs, out=only[:rows])
        got = only.cpu().numpy()
        _exact(got[:rows], c['vf'][form], f'{form} value-only call')
        assert np.isnan(got[rows:]).all()


@pytest.mark.parametrize('shape', fc.ACTOR_SHAPES, ids=IDS)
def test_actor_relu_integer_data_exact(torch_cuda, shape):
    """relu x VF 0 / 1 / 2 and the value-only calls on integer data: logits and vf exact, the action the first maximum, logp inside
    the bound; the second variant's head bias puts the logits of one head more than 88.7 apart."""
    for variant in fc.INT_VARIANTS:
        _relu_exact(torch_cuda, shape, variant, ('own', 'shared'))


@pytest.mark.parametrize('shape', fc.LOOP_SHAPES, ids=[fc.sid(s) for s in fc.LOOP_SHAPES])
def test_actor_grid_stride_loop_exact(torch_cuda, shape):
    """2 200 tiles on a grid of at most 2 048 wavefronts: relu with a value trunk of its own, the exact bar."""
    assert fc.tiles_of(*shape[:3]) > fc.grid_tiles(torch_cuda.cuda.get_device_properties(torch_cuda.cuda.current_device()).multi_processor_count)
    for variant in fc.LOOP_VARIANTS:
        _relu_exact(torch_cuda, shape, variant, ('own',))


@pytest.mark.parametrize('shape', fc.ACTOR_SHAPES, ids=IDS)
def test_actor_tanh_numerics(torch_cuda, shape):
    """tanh x VF 0 / 1 / 2 on the rows of a real env: the assertions of test_actor_gpu's test_tanh_numerics and
    test_greedy_is_first_maximum_of_own_logits, and per value form those of test_critic_gpu's test_value_tanh_numerics,
    test_policy_outputs_are_bit_identical_with_vf and test_value_only_call_is_bit_identical, at this shape."""
    fs.check_tanh_numerics(torch_cuda, shape)
    fs.check_greedy_is_first_maximum_of_own_logits(torch_cuda, shape)
    for form in fc.FORMS:
        fs.check_value_tanh_numerics(torch_cuda, shape, form)
        fs.check_policy_outputs_are_bit_identical_with_vf(torch_cuda, shape, form)
        fs.check_value_only_call_is_bit_identical(torch_cuda, shape, form)


def test_num_active_zero(torch_cuda):
    """num_active = 0: every action is 0 and logp is the log-softmax of the kernel's own logits at action 0."""
    torch = torch_cuda
    shape = fc.NO_ACTIVE_SHAPE
    c = fs.actor_case(torch, shape)
    for sample in (False, True):
        act, logits, logp = fs.actor_run(torch, c['actor'], c['obs'], c['rows'], sample=sample, seed=3, step=1, num_active=0)
        assert not act.any()
        assert np.array_equal(fs.bits(logits), fs.bits(c['logits']))
        lg = logits.astype(np.float64).reshape(c['rows'], -1, shape[3] + 1)
        err = np.abs(logp.astype(np.float64) - fc.log_softmax64(lg)[..., 0]).max()
        assert err <= fc.lse_bound(shape[3] + 1, np.abs(lg).max()), err


def test_1024_slots_rows_and_compact_record_agree(torch_cuda):
    """2 048 rows, slot = row mod 1 024: the rows of the env and FragmentCodec.pack of them give bit-identical actions, logits, logp
    and vf, for both value forms, sampled and greedy."""
    torch = torch_cuda
    from deepcomp_amd.fragment import FragmentCodec
    shape = fc.COMPACT_SHAPE
    kind, E, U, B, H = shape
    codec = FragmentCodec(U, B)
    for form in fc.FORMS:
        c = fs.value_case(torch, shape, form)
        packed = codec.pack(c['obs']).clone()
        codec.check()
        assert torch.equal(codec.unpack(packed).view(torch.int32), c['obs'].view(torch.int32))
        for sample in (False, True):
            kw = dict(sample=sample, seed=0xC0FFEE, step=12, row_base=64)
            vf = torch.full((c['rows'],), float('nan'), device='cuda')
            got = fs.actor_run(torch, c['actor'], packed, c['rows'], compact=True, vf=vf, **kw)
            for x, y in zip(got, c['with', sample]):
                assert np.array_equal(fs.bits(x) if x.dtype == np.float32 else x, fs.bits(y) if y.dtype == np.float32 else y)
            assert np.array_equal(fs.bits(vf.cpu().numpy()), fs.bits(c['vf', sample]))
        assert np.array_equal(fs.bits(c['actor'].value(packed, compact=True).cpu().numpy()), fs.bits(c['only']))


# ================================================================================================ policy set
_SET_OBS = {}


def _set_obs(torch, U, B, E):
    if (U, B, E) not in _SET_OBS:
        env = fs.env('multi', E, U, B)
        env.reset()
        g = torch.Generator(device='cuda').manual_seed(5)
        for _ in range(3):
            env.step(torch.randint(0, B + 1, (E, U), generator=g, device='cuda', dtype=torch.uint8))
        _SET_OBS[U, B, E] = env.obs.clone()
    return _SET_OBS[U, B, E]


def _set_against_members(torch, pset, obs, modes):
    """Every slot's rows of the set's launch equal its member's own launch, bit for bit, with guard bands behind every output."""
    E, U = obs.shape[0], pset.U
    sp = pset.slot_policy
    slot_rows = [torch.arange(E, device='cuda') * U + u for u in range(U)]
    by_member = {}
    for u in range(U):
        by_member.setdefault(sp[u], []).append(slot_rows[u])
    for mode in modes:
        kws = [{}] if mode == 'v' else [dict(sample=True, seed=7, step=3), dict(sample=False)]
        for kw in kws:
            got = fs.set_run(torch, pset, obs, False, mode, guard=fc.SET_GUARD, **kw)
            for p, rows in by_member.items():
                fs.set_same(torch, got, fs.set_run(torch, pset.members[p], obs, False, mode, **kw), rows=torch.cat(rows))
            for k, t in got.items():
                if t.dtype.is_floating_point:
                    assert bool(torch.isfinite(t).all()), k


@pytest.mark.parametrize('value', [False, True], ids=['novalue', 'own'])
@pytest.mark.parametrize('activation', fc.ACTIVATIONS)
@pytest.mark.parametrize('H', fc.POLICY_SET_HIDDEN)
def test_policy_set_every_instantiation(torch_cuda, H, activation, value):
    """Shape (a) of test_policy_set_gpu (U 5, B 3, E 70, slots [0, 1, 1, 0, 1]) at every hidden width, activation and value form."""
    torch = torch_cuda
    from deepcomp_amd.policy_set import PerUEActor
    ps = fc.POLICY_SET
    assert (ps['U'], ps['B'], ps['E']) == (fc.SET_SHAPES['a'][0], fc.SET_SHAPES['a'][1], fc.SET_SHAPES['a'][4]) and ps['slots'] == fc.SET_SLOTS['a']
    obs = _set_obs(torch, ps['U'], ps['B'], ps['E'])
    members = [fs.set_member('a', 10 + p, value, H=H, activation=activation) for p in range(max(ps['slots']) + 1)]
    pset = PerUEActor(members, ps['slots'])
    _set_against_members(torch, pset, obs, ('a', 'av', 'v') if value else ('a',))
    # the comparison discriminates: the two members disagree on the same rows
    a0, a1 = (fs.set_run(torch, m, obs, False, 'a', sample=False)['logits'] for m in members)
    assert not torch.equal(a0, a1)


def test_policy_set_1024_slots(torch_cuda):
    """U 1 024, three members, slot_policy[u] = u % 3, E 2: 1 024 tiles of two rows."""
    torch = torch_cuda
    from deepcomp_amd.policy_set import PerUEActor
    pw = fc.POLICY_SET_WIDE
    obs = _set_obs(torch, pw['U'], pw['B'], pw['E'])
    members = [fs.set_member('a', 10 + p, True, U=pw['U'], B=pw['B'], H=pw['H'], activation='tanh') for p in range(pw['P'])]
    pset = PerUEActor(members, [u % pw['P'] for u in range(pw['U'])])
    _set_against_members(torch, pset, obs, ('a', 'av', 'v'))


# ================================================================================================ learner
@pytest.mark.parametrize('shape', fc.LEARNER_SHAPES, ids=LIDS)
def test_learner_backward_integer_data_exact(torch_cuda, shape):
    """test_learner_gpu's test_backward_integer_data_exact at this shape: all twelve arrays equal the float64 reference exactly."""
    fs.check_backward_integer_data_exact(torch_cuda, shape)


@pytest.mark.parametrize('shape', fc.LEARNER_SHAPES, ids=LIDS)
def test_learner_tanh_numerics(torch_cuda, shape):
    """test_learner_gpu's test_loss_and_gradient_numerics at this shape: statistics and gradients within 2 x the chain's error.
    (At multi4x6x64h128 -- 24 rows, 65 logits -- the entropy statistic was one f32 step off, 3.47e-07 against the chain's 1.30e-07,
    while the tile's row terms were summed in f32: profiles/r13_fcnet_matrix.txt.)"""
    fs.check_loss_and_gradient_numerics(torch_cuda, shape)


@pytest.mark.parametrize('shape', fc.LEARNER_SHAPES, ids=LIDS)
def test_learner_repacked_weights(torch_cuda, shape):
    """test_learner_gpu's test_repacked_weights_are_what_create_packs at this shape: after three updates the handle's actor equals
    a fresh FcnetActor from the master weights bit for bit."""
    fs.check_repacked_weights_are_what_create_packs(torch_cuda, shape)


def test_learner_row_split_with_mult_2(torch_cuda):
    """264 250 rows: the weight-gradient chunk grows to 2 x 2 048 rows (65 chunks); relu, integer data, exact."""
    torch = torch_cuda
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.learner import PPOLearner, ARRAYS
    kind, E, U, B, H = fc.MULT2_SHAPE
    w, v, x, dl, dv, ref = fc.mult2_int_case(1)
    assert fc.row_split(len(x)) == dict(mult=2, chunk_rows=4096, nchunks=65)
    actor = FcnetActor(kind, U, B, w, activation='relu', value_weights=v)
    learner = PPOLearner(actor, max_rows=len(x))
    stats = learner.grads(fs.cuda(torch, x), dlogits=fs.cuda(torch, dl), dvalue=fs.cuda(torch, dv))
    got = learner.read('grads')
    assert np.array_equal(stats.cpu().numpy(), np.zeros(5, dtype=np.float32))
    for n in ARRAYS:
        _exact(got[n], ref[n], n)
    print(f'mult 2: largest gradient entry {max(np.abs(ref[n]).max() for n in ARRAYS):.0f}')


def _bad_entry(torch, idx, n_src):
    bad = idx.clone()
    bad[len(bad) // 2] = n_src
    return bad


@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
@pytest.mark.parametrize('activation', fc.ACTIVATIONS)
@pytest.mark.parametrize('H', fc.INDEXED_HIDDEN)
def test_learner_indexed_every_instantiation(torch_cuda, H, activation, compact):
    """('multi', E 16, U 5, B 4, T 2), 160 source rows, a shuffled index of 70: grads_indexed equals grads on the gathered rows bit
    for bit (statistics, gradients, per-row outputs; evaluate too).  Then the same index with one entry out of range: that position's
    outputs are zeros, every other position's outputs are unchanged to the bit, statistics and gradients stay finite (the gathered
    call has no way to express a position that counts in 1 / N and reads nothing)."""
    torch = torch_cuda
    from deepcomp_amd.learner import ARRAYS
    ix = fc.INDEXED
    kind, E, U, B, T = ix['kind'], ix['E'], ix['U'], ix['B'], ix['T']
    w, vw, batch = fs.collected(torch, kind, E, U, B, H, activation, T, compact)
    learner = fs.ppo_learner(kind, U, B, w, vw, activation, max_rows=E * U * T)
    src = fs.source(batch, learner.actor)
    n_src = E * U * T
    assert ('obs_compact' in src) == compact
    idx = fs.shuffled(torch, n_src, 70, 11)
    _, _, want = fs.check_against_gathered(torch, learner, src, idx)
    bad = _bad_entry(torch, idx, n_src)
    got = fs.outputs(torch, 70, 1)
    stats = learner.grads_indexed(src, bad, **got)
    grads = learner.read('grads')
    assert bool(torch.isfinite(stats).all()) and all(np.isfinite(grads[n]).all() for n in ARRAYS)
    others = torch.ones(70, dtype=torch.bool, device='cuda')
    others[35] = False
    for k in fs.OUTS:
        assert bool((got[k][~others] == 0).all()), k
        assert torch.equal(fs.tbits(torch, got[k][others]), fs.tbits(torch, want[k][others])), k


def test_learner_handle_reused_across_calls(torch_cuda):
    """One learner of 6 400 rows through grads (6 400 rows), grads (37), evaluate (37), upstream grads (37), grads_indexed (50 entries,
    two out of range) and grads (6 400) again: after every step statistics, the twelve arrays and every per-row output equal those
    of a FRESH learner that made only that call, bit for bit, and step 6 equals step 1.  (The H / D workspaces are not zeroed at
    create: every call must rewrite what it later reads.)"""
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    shape = fc.REUSE_SHAPE
    assert shape == fc.LEARNER_BASE_SHAPES[6]
    c = fs.learner_case(torch, shape)
    rows, actor, dev = c['rows'], c['actor'], c['dev']
    assert rows == 6400
    small = {k: t[:37].contiguous() for k, t in dev.items()}
    g = torch.Generator(device='cuda').manual_seed(12)
    up = dict(dlogits=torch.randn((37, actor.num_logits), generator=g, device='cuda'), dvalue=torch.randn(37, generator=g, device='cuda'))
    index = torch.randint(0, rows, (50,), generator=g, device='cuda', dtype=torch.int32)
    index[7], index[31] = -5, rows + 3
    source = dict(dev)

    def outs(n):
        return {k: torch.full((n, actor.heads) if k == 'logp' else (n,), float('nan'), device='cuda') for k in fs.OUTS}

    def step(learner, i):
        """-> (tensors to compare, gradient arrays or None)"""
        if i in (1, 6):
            o = outs(rows)
            st = learner.grads(**dev, **o)
        elif i == 2:
            o = outs(37)
            st = learner.grads(**small, **o)
        elif i == 3:
            return list(learner.evaluate(small['obs'], small['actions'])), None
        elif i == 4:
            o = {'vf': torch.full((37,), float('nan'), device='cuda')}
            st = learner.grads(small['obs'], **up, **o)
        else:
            o = outs(50)
            st = learner.grads_indexed(source, index, **o)
        return [st.clone()] + [o[k] for k in sorted(o)], learner.read('grads')

    one = lm.PPOLearner(actor, max_rows=rows, **HYPER)
    first = None
    for i in range(1, 7):
        got_t, got_g = step(one, i)
        want_t, want_g = step(lm.PPOLearner(actor, max_rows=rows, **HYPER), i)
        for j, (x, y) in enumerate(zip(got_t, want_t)):
            assert torch.equal(fs.tbits(torch, x), fs.tbits(torch, y)), (i, j)
        if got_g is not None:
            for n in lm.ARRAYS:
                assert np.array_equal(fs.bits(got_g[n]), fs.bits(want_g[n])), (i, n)
                assert np.isfinite(got_g[n]).all(), (i, n)
        if i == 1:
            first = (got_t, got_g)
            assert np.array_equal(got_t[0].cpu().numpy(), c['stats'])
        if i == 5:
            assert bool((got_t[1][[7, 31]] == 0).all())                              # (entropy of the two positions that read nothing)
    for x, y in zip(got_t, first[0]):
        assert torch.equal(fs.tbits(torch, x), fs.tbits(torch, y))
    for n in lm.ARRAYS:
        assert np.array_equal(fs.bits(got_g[n]), fs.bits(first[1][n])), n


@pytest.mark.parametrize('run', list(fc.EPILOGUE_RUNS))
@pytest.mark.parametrize('shape', fc.EPILOGUE_SHAPES, ids=[fc.sid(s) for s in fc.EPILOGUE_SHAPES])
def test_loss_epilogue_on_exact_logits(torch_cuda, shape, run):
    """The relu integer net through the real loss: the forward pass is exact, so nothing but the epilogue's own f32 arithmetic is in
    the comparison with the float64 reference.  With b = (NA + 8) 2^-24 max(1, max |logit|) per head: logp within b, entropy and kl
    within 2 heads b, ratio within ratio (heads b + 2^-22), vf exact, db3 per column within 2^-8 mean_r |dlogit64| + 1e-6 of the
    float64 mean of dlogits.  One of the kl, entropy and surrogate terms alive at a time (a wrong sign or coefficient of a term is
    an error of order 1 of db3), then all three."""
    torch = torch_cuda
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.learner import PPOLearner
    kind, E, U, B, H = shape
    c = fc.epilogue_case(shape)
    hy = fc.EPILOGUE_RUNS[run]
    adv = c['advantages'] if fc.EPILOGUE_ADV[run] else c['zero_adv']
    r64, bars = fc.epilogue_f64(c, hy, adv), fc.epilogue_bars(c)
    rows, heads = c['rows'], c['heads']
    actor = FcnetActor(kind, U, B, c['w'], activation='relu', value_weights=c['v']['own'])
    learner = PPOLearner(actor, max_rows=rows, **hy)
    out = {k: torch.full((rows, heads) if k == 'logp' else (rows,), float('nan'), device='cuda') for k in fs.OUTS}
    cu = lambda a: fs.cuda(torch, a)      # noqa: E731
    stats = learner.grads(cu(c['x'].reshape(rows, -1)), cu(c['actions']), cu(c['old_logp']), cu(c['old_logits']), cu(adv), cu(c['value_targets']),
                          cu(c['old_vf']), **out)
    got = {k: t.cpu().numpy().astype(np.float64) for k, t in out.items()}
    grads = learner.read('grads')
    assert np.isfinite(stats.cpu().numpy()).all()
    err = {k: float(np.abs(got[k] - r64[k]).max()) for k in ('logp', 'entropy', 'kl')}
    rel = float((np.abs(got['ratio'] - r64['ratio']) / r64['ratio']).max())
    e3, b3 = fc.b3_gradient_check(grads['b3'], r64['dlogits'])
    print(f'epilogue {fc.sid(shape)} {run}: max |logit| {np.abs(c["lg"]).max():.0f}  logp {err["logp"]:.3e} / {bars["logp"]:.3e}  entropy {err["entropy"]:.3e} / '
          f'{bars["entropy"]:.3e}  kl {err["kl"]:.3e} / {bars["kl"]:.3e}  ratio (rel) {rel:.3e} / {bars["ratio_rel"]:.3e}  db3 worst err / bound {(e3 / b3).max():.3f}')
    for k in ('logp', 'entropy', 'kl'):
        assert err[k] <= bars[k], (k, err[k], bars[k])
    assert rel <= bars['ratio_rel'], (rel, bars['ratio_rel'])
    _exact(out['vf'].cpu().numpy(), c['vf']['own'], 'vf')
    assert (e3 <= b3).all(), (float((e3 / b3).max()), int((e3 / b3).argmax()))
