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

from tests import test_actor_gpu as tag

pytestmark = pytest.mark.gpu

CHUNK = 2048                      # dcomp_learner.hip CHUNK_UNIT: rows of a weight-gradient chunk (while the batch has <= 128 of them)
# (kind, E, U, B, hidden); the last: 6 400 rows = three chunks and a partial one
SHAPES = [('multi', 3, 7, 3, 32), ('multi', 5, 32, 10, 256), ('multi', 9, 5, 32, 64), ('central', 9, 10, 5, 256), ('central', 3, 32, 10, 64),
          ('multi', 4, 6, 10, 96), ('multi', 200, 32, 10, 256)]
IDS = [f'{k}{e}x{u}x{b}h{h}' for k, e, u, b, h in SHAPES]
assert 3 * CHUNK < 200 * 32 < 4 * CHUNK
HYPER = dict(clip_param=0.3, vf_clip_param=0.05, vf_loss_coeff=1.0, entropy_coeff=0.01, kl_coeff=0.2)


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------- (1) exact backward
def _int_case(kind, E, U, B, H, seed):
    """relu, inputs in {0, 1}, sparse +-1 weights and small integer biases in both trunks, dlogits with <= 2 entries of +-1 per row,
    dvalue in {-1, 0, 1}; the float64 reference of all twelve gradients, with both exactness bounds asserted."""
    from tests.test_critic_gpu import _int_value_weights
    rng = np.random.default_rng(500 + seed)
    rows = tag._rows(kind, E, U)
    nin, _, n3 = tag._dims(kind, U, B)
    w, v = tag._int_weights(kind, U, B, H, seed), _int_value_weights(kind, U, B, H, seed, 'own')
    x = rng.integers(0, 2, size=(rows, nin)).astype(np.float64)
    dl = np.zeros((rows, n3))
    for r in range(rows):
        cols = rng.choice(n3, size=min(2, n3), replace=False)
        dl[r, cols] = rng.choice([-1.0, 0.0, 1.0], size=len(cols))
    dv = rng.integers(-1, 2, size=rows).astype(np.float64)
    grads = {}

    def trunk(t, w3, d3, names):
        h1 = np.maximum(x @ t['w1'] + t['b1'], 0)
        h2 = np.maximum(h1 @ t['w2'] + t['b2'], 0)
        d2 = (d3 @ w3.T) * (h2 > 0)
        d1 = (d2 @ t['w2'].astype(np.float64).T) * (h1 > 0)
        for a in (h1, h2, d1, d2, d3):
            assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= 256          # integers, exact in bf16
        for (a, d), (wn, bn) in zip(((x, d1), (h1, d2), (h2, d3)), names):
            assert (np.abs(a).T @ np.abs(d)).max() < 2 ** 24                          # exact in f32 in any order
            assert np.abs(d).sum(0).max() < 2 ** 24
            grads[wn], grads[bn] = a.T @ d, d.sum(0)
    trunk(w, w['w3'].astype(np.float64), dl, (('w1', 'b1'), ('w2', 'b2'), ('w3', 'b3')))
    trunk(v, v['wv'].astype(np.float64).reshape(H, 1), dv.reshape(rows, 1), (('vw1', 'vb1'), ('vw2', 'vb2'), ('wv', 'bv')))
    grads['wv'] = grads['wv'].reshape(-1)
    return w, v, x.astype(np.float32), dl.astype(np.float32), dv.astype(np.float32), grads


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_backward_integer_data_exact(torch_cuda, shape):
    torch = torch_cuda
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.learner import PPOLearner, ARRAYS
    kind, E, U, B, H = shape
    for seed in (1, 2):
        w, v, x, dl, dv, ref = _int_case(kind, E, U, B, H, seed)
        actor = FcnetActor(kind, U, B, w, activation='relu', value_weights=v)
        learner = PPOLearner(actor, max_rows=len(x))
        stats = learner.grads(_cuda(torch, x), dlogits=_cuda(torch, dl), dvalue=_cuda(torch, dv))
        got = learner.read('grads')
        assert np.array_equal(stats.cpu().numpy(), np.zeros(5, dtype=np.float32))
        for n in ARRAYS:
            bad = np.argwhere(got[n] != ref[n].astype(np.float32))
            assert bad.size == 0, f'seed {seed} {n}: {len(bad)} of {got[n].size} entries differ, first at {bad[0]}: {got[n][tuple(bad[0])]} != {ref[n][tuple(bad[0])]}'
        assert any(np.abs(ref[n]).max() > 0 for n in ('w1', 'vw1'))


# ---------------------------------------------------------------------------------------------- the tanh case of a shape
_CASES = {}
RATIOS = (1.7, 0.5, 0.85, 1.15)            # row i's ratio, i % 4: beyond the clip on either side, and inside it
VF_SHIFT = (0.2, -0.02, -0.2, 0.02)        # old_vf - v: beyond vf_clip_param = 0.05 on either side, and inside it


def _old_policy_inputs(w, vw, x, actions, B):
    """old_logp, old_vf, advantages and value targets placed around what the CPU chain computes at the CURRENT weights, so that
    every branch of the loss occurs at every shape, the three-row one included, and no row sits on a kink (where a rounding would
    decide the branch): ratio = RATIOS[i % 4] up to the chain's error; advantages positive on rows 0-3 of every eight and negative
    on 4-7 (so 1.7 is clipped on the first, 0.5 on the second); old_vf = v + VF_SHIFT[i % 4]; value target v - 0.3 on rows 0 mod 4
    (the clipped branch is the larger), v - 0.4 on rows 2 mod 4 (the unclipped one is), v + noise elsewhere."""
    from deepcomp_amd.actor import FcnetActor
    rows, heads = actions.shape
    rng = np.random.default_rng(78)
    lg = FcnetActor.reference_logits_of(w, x, 'tanh', 'bf16').numpy().astype(np.float64).reshape(rows, heads, B + 1)
    lsm = lg - np.log(np.exp(lg - lg.max(-1, keepdims=True)).sum(-1, keepdims=True)) - lg.max(-1, keepdims=True)
    logp = np.take_along_axis(lsm, actions[..., None].astype(np.int64), -1)[..., 0]
    i = np.arange(rows)
    olp = (logp - np.log(np.array(RATIOS))[i % 4, None] / heads).astype(np.float32)
    v = FcnetActor.reference_value_of(w, vw, x, 'tanh', 'bf16').numpy().astype(np.float64)
    ovf = (v + np.array(VF_SHIFT)[i % 4]).astype(np.float32)
    adv = (np.abs(rng.normal(size=rows)) + 0.1) * np.where(i % 8 < 4, 1.0, -1.0)
    vt = np.where(i % 4 == 0, v - 0.3, np.where(i % 4 == 2, v - 0.4, v + rng.normal(size=rows) * 0.3))
    return olp, ovf, adv.astype(np.float32), vt.astype(np.float32)


def _case(torch, shape):
    """Per shape, computed once and left unchanged: real observation rows and the tanh weights of test_actor_gpu's case with a value
    trunk; actions and logits of an OLD policy (the weights perturbed) run by the actor kernel; old_logp, old_vf, advantages and
    value targets of _old_policy_inputs; the kernel's statistics and gradients; the float64 model and the CPU bf16 chain."""
    if shape in _CASES:
        return _CASES[shape]
    from deepcomp_amd import learner as lm
    from deepcomp_amd.actor import FcnetActor
    kind, E, U, B, H = shape
    base = tag._case(torch, shape)
    obs, rows = base['obs'], base['rows']
    w = base['actor'].weights
    vw = FcnetActor.random_value_weights(kind, U, B, H, seed=7, bias_std=0.1)
    rng = np.random.default_rng(77)
    pert = lambda d, s: {n: (a + rng.normal(size=a.shape).astype(np.float32) * np.float32(s * (a.std() + 0.02))) for n, a in d.items()}      # noqa: E731
    old = FcnetActor(kind, U, B, pert(w, 0.25), activation='tanh')
    logits = torch.zeros((rows, old.num_logits), device='cuda')
    act = old.actions(obs, sample=True, seed=3, step=1, logits=logits)
    x = obs.cpu().numpy().reshape(rows, -1)
    olp, ovf, adv, vt = _old_policy_inputs(w, vw, x, act.cpu().numpy().reshape(rows, -1), B)
    logp, vf = _cuda(torch, olp), _cuda(torch, ovf)
    actor = FcnetActor(kind, U, B, w, activation='tanh', value_weights=vw)
    learner = lm.PPOLearner(actor, max_rows=rows, **HYPER)
    dev = dict(obs=obs.reshape(rows, -1).contiguous(), actions=act.reshape(rows, -1).contiguous(), old_logp=logp, old_logits=logits,
               advantages=_cuda(torch, adv), value_targets=_cuda(torch, vt), old_vf=vf)
    stats = learner.grads(**dev)
    c = dict(actor=actor, learner=learner, dev=dev, rows=rows, w=w, vw=vw, stats=stats.cpu().numpy(), grads=learner.read('grads'))
    c['host'] = {k: t.cpu().numpy() for k, t in dev.items()}
    c['ref64'] = lm.ppo_loss_reference(w, vw, c['host'], HYPER, 'tanh', 'float64')
    c['chain'] = lm.ppo_loss_reference(w, vw, c['host'], HYPER, 'tanh', 'bf16')
    _CASES[shape] = c
    return c


def _errors(lm, got_stats, got_grads, ref64, chain):
    """(name, kernel error, chain error) for the five statistics and the twelve arrays: max abs against the float64 model."""
    out = []
    for i, n in enumerate(lm.STATS):
        out.append((n, abs(float(got_stats[i]) - ref64[0][n]), abs(chain[0][n] - ref64[0][n])))
    for n in lm.ARRAYS:
        out.append((n, float(np.abs(got_grads[n].astype(np.float64) - ref64[1][n]).max()), float(np.abs(chain[1][n].astype(np.float64) - ref64[1][n]).max())))
    return out


# ---------------------------------------------------------------------------------------------- (2) unchanged weights
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_unchanged_weights_give_the_actors_logp_and_ratio_one(torch_cuda, shape):
    torch = torch_cuda
    c = _case(torch, shape)
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
    """The kernel's statistics and gradients against the float64 model: allowed 2 x the max abs error the CPU bf16 chain has on the
    same inputs, per statistic and per array (the factor covers the accumulation order and a device tanh that flips single bf16
    roundings).  The old policy is a perturbed weight set: ratios fall on both sides of the clip and both branches of the value
    loss occur (asserted on the model)."""
    from deepcomp_amd import learner as lm
    c = _case(torch_cuda, shape)
    rows64 = c['ref64'][2]
    n = c['rows']
    assert 0 < float(rows64['clipped'].sum()) < n and 0 < float(rows64['vf_clipped'].sum()) < n
    assert float(rows64['ratio'].min()) < 0.7 and float(rows64['ratio'].max()) > 1.3
    assert np.isfinite(c['stats']).all()
    worst = []
    for name, ek, ec in _errors(lm, c['stats'], c['grads'], c['ref64'], c['chain']):
        print(f'learner numerics {shape} {name}: CPU chain max abs err {ec:.3e}  kernel {ek:.3e}  ratio {ek / ec if ec else float("nan"):.2f}')
        if not ek <= 2 * ec:
            worst.append((name, ek, ec))
    assert not worst, worst


# ---------------------------------------------------------------------------------------------- (4) determinism
@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[4], SHAPES[6]], ids=[IDS[1], IDS[4], IDS[6]])
def test_gradients_are_deterministic(torch_cuda, shape):
    from deepcomp_amd import learner as lm
    c = _case(torch_cuda, shape)
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
    c = _case(torch, shape)
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
    c = _case(torch, shape)
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
    worst = [(n, ek, ec) for n, ek, ec in _errors(lm, stats, got, ref64, chain) if not ek <= 2 * ec]
    assert not worst, worst


# ---------------------------------------------------------------------------------------------- (7) Adam
@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[5]], ids=[IDS[0], IDS[5]])
def test_adam_is_adam_reference(torch_cuda, shape):
    """Ten grads + apply steps: master weights and both moments read back equal adam_reference run on the gradients read back at
    each step, bit for bit."""
    from deepcomp_amd import learner as lm
    from deepcomp_amd.actor import FcnetActor
    c = _case(torch_cuda, shape)
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
    """After updates, the actor's handle (rewritten on the device, in both orientations) against a fresh FcnetActor built on the
    host from the learner's master weights: logits, logp, vf and actions bit-identical; and the learner's next gradients are those
    of a fresh learner on that fresh actor (the backward fragments, padding included)."""
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    from deepcomp_amd.actor import FcnetActor
    c = _case(torch, shape)
    kind, E, U, B, H = shape
    rows, obs = c['rows'], c['dev']['obs']
    actor = FcnetActor(kind, U, B, c['w'], activation='tanh', value_weights=c['vw'])
    learner = lm.PPOLearner(actor, lr=3e-3, max_rows=rows, **HYPER)
    for _ in range(3):
        learner.grads(**c['dev'])
        learner.apply()
    w, vw = learner.get_weights()
    assert np.abs(w['w1'] - c['w']['w1']).max() > 1e-3 and actor.weights is w
    fresh = FcnetActor(kind, U, B, w, activation='tanh', value_weights=vw)
    res = []
    for a in (actor, fresh):
        logits, logp = torch.full((rows, a.num_logits), float('nan'), device='cuda'), torch.full((rows, a.heads), float('nan'), device='cuda')
        vf = torch.full((rows,), float('nan'), device='cuda')
        act = a.actions(obs, sample=True, seed=5, step=2, logits=logits, logp=logp, vf=vf)
        res.append((act, logits, logp, vf))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert bool(torch.isfinite(res[0][1]).all())
    g1 = (learner.grads(**c['dev']).cpu().numpy(), learner.read('grads'))
    other = lm.PPOLearner(fresh, max_rows=rows, **HYPER)
    g2 = (other.grads(**c['dev']).cpu().numpy(), other.read('grads'))
    assert np.array_equal(g1[0], g2[0])
    for n in lm.ARRAYS:
        assert np.array_equal(g1[1][n], g2[1][n]), n


# ---------------------------------------------------------------------------------------------- (9) the loss improves
def _collect_like(c, torch):
    d = c['dev']
    return {'obs': d['obs'], 'actions': d['actions'], 'action_logp': d['old_logp'], 'action_dist_inputs': d['old_logits'],
            'advantages': d['advantages'], 'value_targets': d['value_targets'], 'vf_preds': d['old_vf']}


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[3]], ids=[IDS[0], IDS[3]])
def test_update_lowers_the_reference_loss(torch_cuda, shape):
    """update(num_sgd_iter=10, lr=1e-3) on one fixed batch as one minibatch: ppo_loss_reference(form='float64') on the exported
    weights is below its value on the initial ones.  The float64 reference trainer (autograd gradients + adam_reference) on the
    same inputs improves too -- asserted here, and confirmed on the CPU for these weights with stand-in observations -- so the
    batch is one on which ten steps at this rate help."""
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    from deepcomp_amd.actor import FcnetActor
    c = _case(torch, shape)
    kind, E, U, B, H = shape
    actor = FcnetActor(kind, U, B, c['w'], activation='tanh', value_weights=c['vw'])
    learner = lm.PPOLearner(actor, lr=1e-3, max_rows=c['rows'], **HYPER)
    out = learner.update(_collect_like(c, torch), num_sgd_iter=10)
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
    env = tag._env(kind, E, U, B)
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
