"""GPU tests of the PPO learner (include/dcomp_learner.h, deepcomp_amd/learner.py).

Bars: (1) on integer data with upstream gradients every entry of all twelve gradient arrays equals the float64 reference EXACTLY
(any fragment map, k permutation, padding or row-split error shows); (2) at unchanged weights logp and vf are the actor's bit for
bit, every ratio is 1.0 and every kl 0; (3) with tanh and random-init weights the five statistics and each gradient array are within
2 x the error the CPU bf16 chain itself has against the float64 model; (4) bit-identical repeats, also inside a larger handle;
(5) nothing is written past the batch and rows behind it contribute nothing; (6) unlisted rows / heads contribute nothing, NaN
inputs included; (7) Adam is adam_reference to the bit; (8) the repacked fragments are what dcomp_actor_create packs; (9) the loss
falls, judged by the float64 reference; (10) collect -> update, checkpoint and resume.  Measured: profiles/r09_learner_numerics.txt.

The shapes are those of test_actor_gpu plus a padded hidden width and a batch of more than three weight-gradient row chunks.  The
padded width is 96 (packed as 128), not 48: dcomp_actor_create takes multiples of 32 only (tests/test_actor_cpu.py holds it to
that), so 96 / 160 / 192 / 224 are the widths whose packed copies carry padding."""
import ctypes

import numpy as np
import pytest

from tests import fcnet_cases as fc
from tests import fcnet_support as fs
from tests.fcnet_cases import HYPER
from tests.fcnet_support import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SHAPES, IDS = fc.LEARNER_BASE_SHAPES, fc.LEARNER_BASE_IDS


# ---------------------------------------------------------------------------------------------- (1) exact backward
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_backward_integer_data_exact(torch_cuda, shape):
    fs.check_backward_integer_data_exact(torch_cuda, shape)


# ---------------------------------------------------------------------------------------------- (2) unchanged weights
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_unchanged_weights_give_the_actors_logp_and_ratio_one(torch_cuda, shape):
    torch = torch_cuda
    c = fs.learner_case(torch, shape)
    actor, learner, rows, obs = c['actor'], c['learner'], c['rows'], c['dev']['obs']
    logits = torch.full((rows, actor.num_logits), float('nan'), device='cuda')
    logp, vf = torch.full((rows, actor.heads), float('nan'), device='cuda'), torch.full((rows,), float('nan'), device='cuda')
    act = actor.actions(obs, sample=True, seed=9, step=4, logits=logits, logp=logp, vf=vf).reshape(rows, -1).contiguous()
    e_logp, e_ent, e_vf = learner.evaluate(obs, act)
    assert torch.equal(e_logp, logp) and torch.equal(e_vf, vf)
    assert bool((e_ent > 0).all())
    ratio, kl = torch.full((rows,), float('nan'), device='cuda'), torch.full((rows,), float('nan'), device='cuda')
    g_logp = torch.full((rows, actor.heads), float('nan'), device='cuda')
    second = type(learner)(actor, max_rows=rows, **HYPER)                    # (the case's own gradients stay as they are)
    stats = second.grads(obs, act, logp, logits, c['dev']['advantages'], c['dev']['value_targets'], vf, ratio=ratio, kl=kl, logp=g_logp)
    assert torch.equal(g_logp, logp)
    assert torch.equal(ratio, torch.ones_like(ratio)), (ratio - 1).abs().max()
    assert torch.equal(kl, torch.zeros_like(kl)), kl.abs().max()
    assert float(stats[3]) == 0.0


# ---------------------------------------------------------------------------------------------- (3) numerics
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_loss_and_gradient_numerics(torch_cuda, shape):
    fs.check_loss_and_gradient_numerics(torch_cuda, shape)


# ---------------------------------------------------------------------------------------------- (4) determinism
@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[4], SHAPES[6]], ids=[IDS[1], IDS[4], IDS[6]])
def test_gradients_are_deterministic(torch_cuda, shape):
    from deepcomp_amd import learner as lm
    c = fs.learner_case(torch_cuda, shape)
    for max_rows in (c['rows'], c['rows'] + 5000):                            # the same handle size again, and the rows inside a larger one
        other = lm.PPOLearner(c['actor'], max_rows=max_rows, **HYPER)
        for _ in range(2):
            stats = other.grads(**c['dev']).cpu().numpy()
            got = other.read('grads')
            assert np.array_equal(stats, c['stats'])
            for n in lm.ARRAYS:
                assert np.array_equal(got[n], c['grads'][n]), n


# ---------------------------------------------------------------------------------------------- (5) nothing past the batch
@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[3], SHAPES[5]], ids=[IDS[0], IDS[3], IDS[5]])
def test_nothing_past_the_batch(torch_cuda, shape):
    """Outputs behind the batch stay as they were, and what lies behind the batch's inputs (NaN) reaches nothing: every shape here
    ends in a partial tile."""
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    c = fs.learner_case(torch, shape)
    rows, actor = c['rows'], c['actor']
    assert rows % 32
    pad = 70

    def padded(t):
        buf = torch.full((rows + pad,) + tuple(t.shape[1:]), float('nan') if t.dtype.is_floating_point else 255, dtype=t.dtype, device='cuda')
        buf[:rows] = t
        return buf
    bufs = {k: padded(t) for k, t in c['dev'].items()}
    outs = {k: torch.full((rows + pad, per), float('nan'), device='cuda') for k, per in
            (('logp', actor.heads), ('entropy', 1), ('kl', 1), ('vf', 1), ('ratio', 1))}
    other = lm.PPOLearner(actor, max_rows=rows + pad, **HYPER)
    stats = other.grads(**{k: b[:rows] for k, b in bufs.items()}, **{k: b[:rows].reshape(-1) if k != 'logp' else b[:rows] for k, b in outs.items()})
    got = other.read('grads')
    assert np.array_equal(stats.cpu().numpy(), c['stats'])
    for n in lm.ARRAYS:
        assert np.array_equal(got[n], c['grads'][n]), n
    for k, b in outs.items():
        assert bool(torch.isnan(b[rows:]).all()), k
        assert bool(torch.isfinite(b[:rows]).all()), k
    ref = c['chain'][2]
    assert np.abs(outs['vf'][:rows, 0].cpu().numpy() - ref['vf'].numpy()).max() < 0.05


# ---------------------------------------------------------------------------------------------- (6) num_active below U
@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[3]], ids=[IDS[1], IDS[3]])
def test_unlisted_rows_and_heads_contribute_nothing(torch_cuda, shape):
    """num_active = U - 3: a multi row of an unlisted slot / a central head beyond the listed ones changes neither the statistics
    nor the gradients, with NaN (and action 255) in everything that belongs to it.  Against the reference with the same mask, at
    the bar of the numerics test."""
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    c = fs.learner_case(torch, shape)
    kind, E, U, B, H = shape
    rows, na = c['rows'], U - 3
    dev = {k: t.clone() for k, t in c['dev'].items()}
    if kind == 'multi':
        off = (torch.arange(rows, device='cuda') % U) >= na
        for k, t in dev.items():
            t[off] = 255 if k == 'actions' else float('nan')
    else:
        dev['actions'][:, na:] = 255
        dev['old_logp'][:, na:] = float('nan')
        dev['old_logits'].reshape(rows, U, B + 1)[:, na:] = float('nan')
    other = lm.PPOLearner(c['actor'], max_rows=rows, **HYPER)
    stats = other.grads(**dev, num_active=na).cpu().numpy()
    got = other.read('grads')
    host = dict(c['host'], num_active=na)
    if kind == 'multi':
        host['num_ue'] = U
    ref64 = lm.ppo_loss_reference(c['w'], c['vw'], host, HYPER, 'tanh', 'float64')
    chain = lm.ppo_loss_reference(c['w'], c['vw'], host, HYPER, 'tanh', 'bf16')
    assert np.isfinite(stats).all() and all(np.isfinite(got[n]).all() for n in lm.ARRAYS)
    assert abs(ref64[0]['total_loss'] - c['ref64'][0]['total_loss']) > 1e-4      # (the mask does change the loss)
    worst = [(n, ek, ec) for n, ek, ec in fs.errors(lm, stats, got, ref64, chain) if not ek <= 2 * ec]
    assert not worst, worst


# ---------------------------------------------------------------------------------------------- (7) Adam
@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[5]], ids=[IDS[0], IDS[5]])
def test_adam_is_adam_reference(torch_cuda, shape):
    """Ten grads + apply steps: master weights and both moments read back equal adam_reference run on the gradients read back at
    each step, bit for bit."""
    from deepcomp_amd import learner as lm
    from deepcomp_amd.actor import FcnetActor
    c = fs.learner_case(torch_cuda, shape)
    kind, E, U, B, H = shape
    actor = FcnetActor(kind, U, B, c['w'], activation='tanh', value_weights=c['vw'])
    learner = lm.PPOLearner(actor, lr=1e-3, max_rows=c['rows'], **HYPER)
    w = learner.read('weights')
    m, v = {n: np.zeros_like(a) for n, a in w.items()}, {n: np.zeros_like(a) for n, a in w.items()}
    assert all(np.array_equal(w[n], a) for n, a in lm.join_weights(c['w'], c['vw']).items())
    for t in range(1, 11):
        learner.grads(**c['dev'])
        g = learner.read('grads')
        learner.apply()
        got = {k: learner.read(k) for k in ('weights', 'm', 'v')}
        assert learner.step == t
        for n in lm.ARRAYS:
            w[n], m[n], v[n] = lm.adam_reference(w[n], g[n], m[n], v[n], t, 1e-3)
            for k, want in (('weights', w), ('m', m), ('v', v)):
                assert np.array_equal(got[k][n], want[n]), (t, k, n, np.abs(got[k][n] - want[n]).max())
    assert np.abs(w['w2'] - c['w']['w2']).max() > 1e-3


# ---------------------------------------------------------------------------------------------- (8) repack
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_repacked_weights_are_what_create_packs(torch_cuda, shape):
    fs.check_repacked_weights_are_what_create_packs(torch_cuda, shape)


# ---------------------------------------------------------------------------------------------- (9) the loss improves
@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[3]], ids=[IDS[0], IDS[3]])
def test_update_lowers_the_reference_loss(torch_cuda, shape):
    """update(num_sgd_iter=10, lr=1e-3) on one fixed batch as one minibatch: ppo_loss_reference(form='float64') on the exported
    weights is below its value on the initial ones.  The float64 reference trainer (autograd gradients + adam_reference) on the
    same inputs improves too -- asserted here, and confirmed on the CPU for these weights with stand-in observations -- so the
    batch is one on which ten steps at this rate help."""
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    from deepcomp_amd.actor import FcnetActor
    c = fs.learner_case(torch, shape)
    kind, E, U, B, H = shape
    actor = FcnetActor(kind, U, B, c['w'], activation='tanh', value_weights=c['vw'])
    learner = lm.PPOLearner(actor, lr=1e-3, max_rows=c['rows'], **HYPER)
    out = learner.update(fs.collect_like(c, torch), num_sgd_iter=10)
    assert all(np.isfinite(out[n]) for n in lm.STATS)
    host = dict(c['host'])
    adv = host['advantages'].astype(np.float64)
    host['advantages'] = ((adv - adv.mean()) / max(1e-4, adv.std())).astype(np.float32)
    loss = lambda w, vw: lm.ppo_loss_reference(w, vw, host, HYPER, 'tanh', 'float64')[0]['total_loss']      # noqa: E731
    before, after = loss(c['w'], c['vw']), loss(*learner.get_weights())
    arrays = lm.join_weights(c['w'], c['vw'])
    m, v = {n: np.zeros_like(a) for n, a in arrays.items()}, {n: np.zeros_like(a) for n, a in arrays.items()}
    for t in range(1, 11):
        g = lm.ppo_loss_reference(*lm.split_weights(arrays), host, HYPER, 'tanh', 'float64')[1]
        for n in lm.ARRAYS:
            arrays[n], m[n], v[n] = lm.adam_reference(arrays[n], g[n].astype(np.float32), m[n], v[n], t, 1e-3)
    trained = loss(*lm.split_weights(arrays))
    print(f'update {shape}: reference loss {before:.5f} -> {after:.5f} (float64 reference trainer: {trained:.5f})')
    assert trained < before
    assert after < before


# ---------------------------------------------------------------------------------------------- (10) collect -> update
def test_collect_update_checkpoint_resume(torch_cuda):
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.sampler import collect
    kind, E, U, B, H, T = 'multi', 64, 5, 4, 64, 5
    w = FcnetActor.random_weights(kind, U, B, H, seed=1, bias_std=0.1)
    vw = FcnetActor.random_value_weights(kind, U, B, H, seed=1, bias_std=0.1)
    env = fs.env(kind, E, U, B)
    actor = FcnetActor(kind, U, B, w, activation='tanh', value_weights=vw)
    plain = collect(env, actor, T, gamma=0.99, lam=0.95)
    assert sorted(plain) == sorted(['obs', 'new_obs_last', 'actions', 'action_logp', 'vf_preds', 'rewards', 'advantages', 'value_targets', 'dones', 'last_vf'])
    batch = collect(env, actor, T, gamma=0.99, lam=0.95, dist_inputs=True)
    assert sorted(batch) == sorted(list(plain) + ['action_dist_inputs']) and batch['action_dist_inputs'].shape == (T, E * U, B + 1)
    lsm = torch.log_softmax(batch['action_dist_inputs'].double(), -1).gather(-1, batch['actions'].reshape(T, E * U, 1).long())
    assert float((lsm.float() - batch['action_logp']).abs().max()) < 1e-4    # the logits the actions were drawn from
    learner = lm.PPOLearner(actor, lr=1e-3, max_rows=512)
    out = learner.update(batch, num_sgd_iter=2, minibatch_rows=512, seed=3)  # 1 600 rows: three full minibatches and a partial one
    assert all(np.isfinite(out[n]) for n in lm.STATS) and out['kl'] >= 0 and out['kl_coeff'] in (0.2 * 0.5, 0.2, 0.2 * 1.5)
    new_w, _ = learner.get_weights()
    assert np.abs(new_w['w2'] - w['w2']).max() > 1e-4 and learner.step == 8
    with pytest.raises(ValueError):
        learner.update(plain)
    state = learner.state_dict()
    actor2 = FcnetActor(kind, U, B, w, activation='tanh', value_weights=vw)
    learner2 = lm.PPOLearner(actor2, lr=7.0, max_rows=512)
    learner2.load_state_dict(state)
    assert learner2.lr == learner.lr and learner2.hyper['kl_coeff'] == learner.hyper['kl_coeff']
    for l in (learner, learner2):
        l.update(batch, num_sgd_iter=1, minibatch_rows=512, seed=4)
    s1, s2 = learner.state_dict(), learner2.state_dict()
    assert s1['step'] == s2['step'] == 12
    for k in ('weights', 'm', 'v'):
        for n in lm.ARRAYS:
            assert np.array_equal(s1[k][n], s2[k][n]), (k, n)
    a1 = actor.actions(batch['obs'][0], sample=False)
    assert torch.equal(a1, actor2.actions(batch['obs'][0], sample=False))
    rl = learner.to_rllib_weights()
    assert np.array_equal(FcnetActor.map_rllib_weights(rl)['w3'], s1['weights']['w3'])


def test_refusals_that_need_a_handle(torch_cuda):
    torch = torch_cuda
    from deepcomp_amd import _lib, learner as lm
    from deepcomp_amd.actor import FcnetActor
    kind, U, B, H = 'multi', 4, 3, 32
    w = FcnetActor.random_weights(kind, U, B, H, seed=1)
    vw = FcnetActor.random_value_weights(kind, U, B, H, seed=1)
    with pytest.raises(ValueError):
        lm.PPOLearner(FcnetActor(kind, U, B, w))
    shared = FcnetActor(kind, U, B, w, value_weights=FcnetActor.random_value_weights(kind, U, B, H, seed=1, shared=True))
    with pytest.raises(NotImplementedError):
        lm.PPOLearner(shared)
    # the library's own refusals of the same handles
    L = _lib.load()
    host = {n: np.ascontiguousarray(a) for n, a in lm.join_weights(w, vw).items()}
    arr = lm._arrays_struct(host)
    cfg = _lib.DcompLearnerCfg(ctypes.sizeof(_lib.DcompLearnerCfg), 0, 64, 0.9, 0.999, 1e-8, 0, ctypes.pointer(arr))
    out = ctypes.c_void_p()
    assert L.dcomp_learner_create(FcnetActor(kind, U, B, w)._h, ctypes.byref(cfg), ctypes.byref(out)) == _lib.EINVAL and b'value trunk' in L.dcomp_last_error()
    assert L.dcomp_learner_create(shared._h, ctypes.byref(cfg), ctypes.byref(out)) == _lib.EUNSUPPORTED
    actor = FcnetActor(kind, U, B, w, value_weights=vw)
    learner = lm.PPOLearner(actor, max_rows=64)
    obs = torch.zeros((68, actor.num_in), device='cuda')
    with pytest.raises(ValueError):
        learner.grads(obs, dlogits=torch.zeros((68, B + 1), device='cuda'), dvalue=torch.zeros(68, device='cuda'))
    b = _lib.DcompPpoBatch(ctypes.sizeof(_lib.DcompPpoBatch), 0, 68, U, 0, obs.data_ptr(), *([None] * 11), obs.data_ptr(), obs.data_ptr())
    hy = _lib.DcompPpoHyper(ctypes.sizeof(_lib.DcompPpoHyper), 0.3, 10.0, 1.0, 0.0, 0.2)
    assert L.dcomp_learner_grads(learner._h, ctypes.byref(b), ctypes.byref(hy), ctypes.c_void_p(obs.data_ptr()), None) == _lib.EINVAL
    assert b'max_rows' in L.dcomp_last_error()
    b.rows, b.num_active = 64, U + 1
    assert L.dcomp_learner_grads(learner._h, ctypes.byref(b), ctypes.byref(hy), ctypes.c_void_p(obs.data_ptr()), None) == _lib.EINVAL
    assert b'num_active' in L.dcomp_last_error()
    for bad in (torch.zeros(64 * actor.num_in + 1, device='cuda'), torch.zeros((64, actor.num_in), dtype=torch.float64, device='cuda'), torch.zeros((64, actor.num_in))):
        with pytest.raises(ValueError):
            learner.evaluate(bad, torch.zeros((64, 1), dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        learner.evaluate(obs[:64], torch.zeros((63, 1), dtype=torch.uint8, device='cuda'))
