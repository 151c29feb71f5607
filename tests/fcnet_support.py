"""What the fcnet GPU tests (tests/test_actor_gpu.py ... tests/test_sgd_characterization_gpu.py) share: the builders that run the
device, the cases and sample batches that are computed once per session and left unchanged, and the checks that more than one file
holds a kernel to.  The tables and everything that needs no device are in tests/fcnet_cases.py and tests/group_cases.py; this module
reads them and no test module, and no module under tests/ imports a test module (tests/test_layout_cpu.py).

Every cache lives here, once: ACTOR_CASES, VALUE_CASES, LEARNER_CASES (per shape), COLLECTED (per collect() configuration), SET_BATCH
and GROUP_BATCH (collect() driven by a policy set), WHOLE and TERMS (the accumulated-gradient reference).  A batch that several test
files use is therefore collected once whichever file runs first."""
import ctypes

import numpy as np
import pytest

from tests import fcnet_cases as fc
from tests import group_cases
from tests.fcnet_cases import HYPER, RATIOS, VF_SHIFT

OUTS = ('logp', 'entropy', 'kl', 'vf', 'ratio')


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def tbits(torch, t):
    return t.contiguous().view(torch.int32)


# ================================================================================================ actor
def actor_run(torch, actor, obs, rows, **kw):
    logits = torch.full((rows, actor.num_logits), float('nan'), device='cuda')
    logp = torch.full((rows, actor.heads), float('nan'), device='cuda')
    act = actor.actions(obs, logits=logits, logp=logp, **kw)
    torch.cuda.synchronize()
    return act.cpu().numpy(), logits.cpu().numpy(), logp.cpu().numpy()


def env(kind, E, U, B, **kw):
    from deepcomp_amd import scenarios
    from deepcomp_amd.entities import build_from_scenario
    from deepcomp_amd.env import BatchedMobileEnv
    m, bs, ues = build_from_scenario(scenarios.grid_map(B, 'mixed').with_ues(num_slow=U))
    return BatchedMobileEnv(m, bs, ues, kind, num_envs=E, seed=42, episode_length=100, rng='philox', rand_episodes=True, **kw)


ACTOR_CASES = {}


def actor_case(torch, shape):
    """Per shape, computed once and left unchanged: observation rows of a real env (reset + 3 steps of random actions), a tanh
    actor with random-init weights (N(0, 1 / fan_in) kernels, N(0, 0.1) biases), the kernel's greedy run, the float64 reference
    and the CPU chain's own error against it."""
    if shape in ACTOR_CASES:
        return ACTOR_CASES[shape]
    from deepcomp_amd.actor import FcnetActor
    kind, E, U, B, H = shape
    e = env(kind, E, U, B)
    e.reset()
    g = torch.Generator(device='cuda').manual_seed(5)
    for _ in range(3):
        e.step(torch.randint(0, B + 1, (E, U), generator=g, device='cuda', dtype=torch.uint8))
    e.check()
    obs = e.obs.clone()
    w = FcnetActor.random_weights(kind, U, B, H, seed=7, bias_std=0.1)
    actor = FcnetActor(kind, U, B, w, activation='tanh')
    rows = fc.rows_of(kind, E, U)
    act, logits, logp = actor_run(torch, actor, obs, rows, sample=False)
    x = obs.cpu().numpy().reshape(rows, -1)
    ref64 = actor.reference_logits(x, form='float64').numpy()
    chain = actor.reference_logits(x, form='bf16').numpy().astype(np.float64)
    c = dict(actor=actor, obs=obs, rows=rows, act=act, logits=logits, logp=logp, ref64=ref64,
             err_chain=float(np.abs(chain - ref64).max()), err_kernel=float(np.abs(logits.astype(np.float64) - ref64).max()))
    ACTOR_CASES[shape] = c
    return c


def check_tanh_numerics(torch, shape):
    """Kernel logits against the float64 model: allowed 2 x the max abs error the CPU bf16 / f32 chain has on the same inputs (the
    factor covers the accumulation order and a device tanh that flips individual bf16 roundings).  Measured on the MI355X
    (profiles/r07_actor_numerics.txt): the kernel's max abs error equals the chain's to four digits at all seven shapes, 1.2e-3 ... 2.9e-3."""
    c = actor_case(torch, shape)
    print(f'actor numerics {shape}: logit std {c["ref64"].std():.3f}  CPU chain max abs err {c["err_chain"]:.3e}  kernel {c["err_kernel"]:.3e}  '
          f'ratio {c["err_kernel"] / c["err_chain"]:.2f}')
    assert np.isfinite(c['logits']).all()
    assert c['err_kernel'] <= 2 * c['err_chain'], (c['err_kernel'], c['err_chain'])


def check_greedy_is_first_maximum_of_own_logits(torch, shape):
    c = actor_case(torch, shape)
    B = shape[3]
    own = c['logits'].reshape(c['rows'], c['actor'].heads, B + 1).argmax(axis=-1)
    assert np.array_equal(c['act'].reshape(c['rows'], c['actor'].heads), own)


# ================================================================================================ value head
VALUE_CASES = {}


def value_case(torch, shape, form):
    """Per (shape, form), computed once and left unchanged: the observation rows and tanh actor weights of actor_case, random-init
    value weights (N(0, 0.1) biases), and the kernel's runs -- without vf, with vf, value only; greedy and sampled."""
    if (shape, form) in VALUE_CASES:
        return VALUE_CASES[(shape, form)]
    from deepcomp_amd.actor import FcnetActor
    kind, E, U, B, H = shape
    base = actor_case(torch, shape)
    obs, rows = base['obs'], base['rows']
    v = FcnetActor.random_value_weights(kind, U, B, H, seed=7, bias_std=0.1, shared=form == 'shared')
    actor = FcnetActor(kind, U, B, base['actor'].weights, activation='tanh', value_weights=v)
    c = dict(actor=actor, obs=obs, rows=rows)
    for sample in (False, True):
        kw = dict(sample=sample, seed=0xC0FFEE, step=12, row_base=64)
        c['plain', sample] = actor_run(torch, actor, obs, rows, **kw)
        vf = torch.full((rows,), float('nan'), device='cuda')
        c['with', sample] = actor_run(torch, actor, obs, rows, vf=vf, **kw)
        c['vf', sample] = vf.cpu().numpy()
    only = torch.full((rows,), float('nan'), device='cuda')
    assert actor.value(obs, out=only) is only
    c['only'] = only.cpu().numpy()
    x = obs.cpu().numpy().reshape(rows, -1)
    ref64 = actor.reference_value(x, form='float64').numpy()
    chain = actor.reference_value(x, form='bf16').numpy().astype(np.float64)
    c['ref64'] = ref64
    c['err_chain'] = float(np.abs(chain - ref64).max())
    c['err_kernel'] = float(np.abs(c['vf', False].astype(np.float64) - ref64).max())
    VALUE_CASES[(shape, form)] = c
    return c


def check_value_tanh_numerics(torch, shape, form):
    """Kernel vf against the float64 model on real observations: allowed 2 x the max abs error the CPU bf16 / f32 chain has on the
    same inputs (the factor covers the accumulation order and a device tanh that flips individual bf16 roundings).  Measured on the
    MI355X: profiles/r08_critic_numerics.txt."""
    c = value_case(torch, shape, form)
    print(f'critic numerics {shape} {form}: value std {c["ref64"].std():.3f}  CPU chain max abs err {c["err_chain"]:.3e}  kernel {c["err_kernel"]:.3e}  '
          f'ratio {c["err_kernel"] / c["err_chain"]:.2f}')
    assert np.isfinite(c['vf', False]).all()
    assert c['err_chain'] > 0
    assert c['err_kernel'] <= 2 * c['err_chain'], (c['err_kernel'], c['err_chain'])


def check_policy_outputs_are_bit_identical_with_vf(torch, shape, form):
    """actions, logits and logp of actions(..., vf=...) == those of the call without vf, greedy and sampled; and they are those of
    the actor without a value function (actor_case: the same weights, greedy)."""
    c = value_case(torch, shape, form)
    for sample in (False, True):
        (a0, l0, p0), (a1, l1, p1) = c['plain', sample], c['with', sample]
        assert np.array_equal(a0, a1), sample
        assert np.array_equal(bits(l0), bits(l1)), sample
        assert np.array_equal(bits(p0), bits(p1)), sample
    base = actor_case(torch, shape)
    assert np.array_equal(bits(c['with', False][1]), bits(base['logits'])) and np.array_equal(c['with', False][0], base['act'])
    assert not np.array_equal(c['with', False][0], c['with', True][0])            # (the sampled run did sample)


def check_value_only_call_is_bit_identical(torch, shape, form):
    c = value_case(torch, shape, form)
    assert np.isfinite(c['only']).all()
    assert np.array_equal(bits(c['only']), bits(c['vf', False]))
    assert np.array_equal(bits(c['only']), bits(c['vf', True]))         # the draws do not touch the value


# ================================================================================================ learner
def old_policy_inputs(w, vw, x, actions, B):
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


LEARNER_CASES = {}


def learner_case(torch, shape):
    """Per shape, computed once and left unchanged: real observation rows and the tanh weights of actor_case with a value trunk;
    actions and logits of an OLD policy (the weights perturbed) run by the actor kernel; old_logp, old_vf, advantages and value
    targets of old_policy_inputs; the kernel's statistics and gradients; the float64 model and the CPU bf16 chain."""
    if shape in LEARNER_CASES:
        return LEARNER_CASES[shape]
    from deepcomp_amd import learner as lm
    from deepcomp_amd.actor import FcnetActor
    kind, E, U, B, H = shape
    base = actor_case(torch, shape)
    obs, rows = base['obs'], base['rows']
    w = base['actor'].weights
    vw = FcnetActor.random_value_weights(kind, U, B, H, seed=7, bias_std=0.1)
    rng = np.random.default_rng(77)
    pert = lambda d, s: {n: (a + rng.normal(size=a.shape).astype(np.float32) * np.float32(s * (a.std() + 0.02))) for n, a in d.items()}      # noqa: E731
    old = FcnetActor(kind, U, B, pert(w, 0.25), activation='tanh')
    logits = torch.zeros((rows, old.num_logits), device='cuda')
    act = old.actions(obs, sample=True, seed=3, step=1, logits=logits)
    x = obs.cpu().numpy().reshape(rows, -1)
    olp, ovf, adv, vt = old_policy_inputs(w, vw, x, act.cpu().numpy().reshape(rows, -1), B)
    logp, vf = cuda(torch, olp), cuda(torch, ovf)
    actor = FcnetActor(kind, U, B, w, activation='tanh', value_weights=vw)
    learner = lm.PPOLearner(actor, max_rows=rows, **HYPER)
    dev = dict(obs=obs.reshape(rows, -1).contiguous(), actions=act.reshape(rows, -1).contiguous(), old_logp=logp, old_logits=logits,
               advantages=cuda(torch, adv), value_targets=cuda(torch, vt), old_vf=vf)
    stats = learner.grads(**dev)
    c = dict(actor=actor, learner=learner, dev=dev, rows=rows, w=w, vw=vw, stats=stats.cpu().numpy(), grads=learner.read('grads'))
    c['host'] = {k: t.cpu().numpy() for k, t in dev.items()}
    c['ref64'] = lm.ppo_loss_reference(w, vw, c['host'], HYPER, 'tanh', 'float64')
    c['chain'] = lm.ppo_loss_reference(w, vw, c['host'], HYPER, 'tanh', 'bf16')
    LEARNER_CASES[shape] = c
    return c


def errors(lm, got_stats, got_grads, ref64, chain):
    """(name, kernel error, chain error) for the five statistics and the twelve arrays: max abs against the float64 model."""
    out = []
    for i, n in enumerate(lm.STATS):
        out.append((n, abs(float(got_stats[i]) - ref64[0][n]), abs(chain[0][n] - ref64[0][n])))
    for n in lm.ARRAYS:
        out.append((n, float(np.abs(got_grads[n].astype(np.float64) - ref64[1][n]).max()), float(np.abs(chain[1][n].astype(np.float64) - ref64[1][n]).max())))
    return out


def collect_like(c, torch):
    d = c['dev']
    return {'obs': d['obs'], 'actions': d['actions'], 'action_logp': d['old_logp'], 'action_dist_inputs': d['old_logits'],
            'advantages': d['advantages'], 'value_targets': d['value_targets'], 'vf_preds': d['old_vf']}


def check_backward_integer_data_exact(torch, shape):
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.learner import PPOLearner, ARRAYS
    kind, E, U, B, H = shape
    for seed in (1, 2):
        w, v, x, dl, dv, ref = fc.learner_int_case(kind, E, U, B, H, seed)
        actor = FcnetActor(kind, U, B, w, activation='relu', value_weights=v)
        learner = PPOLearner(actor, max_rows=len(x))
        stats = learner.grads(cuda(torch, x), dlogits=cuda(torch, dl), dvalue=cuda(torch, dv))
        got = learner.read('grads')
        assert np.array_equal(stats.cpu().numpy(), np.zeros(5, dtype=np.float32))
        for n in ARRAYS:
            bad = np.argwhere(got[n] != ref[n].astype(np.float32))
            assert bad.size == 0, f'seed {seed} {n}: {len(bad)} of {got[n].size} entries differ, first at {bad[0]}: {got[n][tuple(bad[0])]} != {ref[n][tuple(bad[0])]}'
        assert any(np.abs(ref[n]).max() > 0 for n in ('w1', 'vw1'))


def check_loss_and_gradient_numerics(torch, shape):
    """The kernel's statistics and gradients against the float64 model: allowed 2 x the max abs error the CPU bf16 chain has on the
    same inputs, per statistic and per array (the factor covers the accumulation order and a device tanh that flips single bf16
    roundings).  The old policy is a perturbed weight set: ratios fall on both sides of the clip and both branches of the value
    loss occur (asserted on the model)."""
    from deepcomp_amd import learner as lm
    c = learner_case(torch, shape)
    rows64 = c['ref64'][2]
    n = c['rows']
    assert 0 < float(rows64['clipped'].sum()) < n and 0 < float(rows64['vf_clipped'].sum()) < n
    assert float(rows64['ratio'].min()) < 0.7 and float(rows64['ratio'].max()) > 1.3
    assert np.isfinite(c['stats']).all()
    worst = []
    for name, ek, ec in errors(lm, c['stats'], c['grads'], c['ref64'], c['chain']):
        print(f'learner numerics {shape} {name}: CPU chain max abs err {ec:.3e}  kernel {ek:.3e}  ratio {ek / ec if ec else float("nan"):.2f}')
        if not ek <= 2 * ec:
            worst.append((name, ek, ec))
    assert not worst, worst


def check_repacked_weights_are_what_create_packs(torch, shape):
    """After updates, the actor's handle (rewritten on the device, in both orientations) against a fresh FcnetActor built on the
    host from the learner's master weights: logits, logp, vf and actions bit-identical; and the learner's next gradients are those
    of a fresh learner on that fresh actor (the backward fragments, padding included)."""
    from deepcomp_amd import learner as lm
    from deepcomp_amd.actor import FcnetActor
    c = learner_case(torch, shape)
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


# ================================================================================================ indexed minibatches
COLLECTED = {}


def collected(torch, kind, E, U, B, H, activation, T, compact):
    """One collect(..., dist_inputs=True) batch per configuration, computed once and left unchanged: (weights, value weights, batch)."""
    key = (kind, E, U, B, H, activation, T, compact)
    if key not in COLLECTED:
        from deepcomp_amd.actor import FcnetActor
        from deepcomp_amd.sampler import collect
        w = FcnetActor.random_weights(kind, U, B, H, seed=1, bias_std=0.1)
        vw = FcnetActor.random_value_weights(kind, U, B, H, seed=1, bias_std=0.1)
        actor = FcnetActor(kind, U, B, w, activation=activation, value_weights=vw)
        batch = collect(env(kind, E, U, B), actor, T, gamma=0.99, lam=0.95, compact=compact, dist_inputs=True)
        COLLECTED[key] = (w, vw, batch)
    return COLLECTED[key]


def perturbed(w, vw, seed=5):
    rng = np.random.default_rng(seed)
    pert = lambda d: {n: (a + rng.normal(size=a.shape).astype(np.float32) * np.float32(0.25 * (a.std() + 0.02))) for n, a in d.items()}      # noqa: E731
    return pert(w), pert(vw)


def ppo_learner(kind, U, B, w, vw, activation, max_rows, perturb=True, **kw):
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.learner import PPOLearner
    if perturb:
        w, vw = perturbed(w, vw)
    return PPOLearner(FcnetActor(kind, U, B, w, activation=activation, value_weights=vw), max_rows=max_rows, **dict(HYPER, **kw))


def source(batch, actor, own_advantages=False):
    """The flattened sample-batch tensors of a collect() batch under grads' argument names.  own_advantages: a copy of the
    advantages, for a caller that writes to them."""
    adv = batch['advantages'].reshape(-1)
    s = {'actions': batch['actions'].reshape(-1, actor.heads), 'old_logp': batch['action_logp'].reshape(-1, actor.heads),
         'old_logits': batch['action_dist_inputs'].reshape(-1, actor.num_logits), 'advantages': adv.clone() if own_advantages else adv,
         'value_targets': batch['value_targets'].reshape(-1), 'old_vf': batch['vf_preds'].reshape(-1)}
    if 'obs' in batch:
        s['obs'] = batch['obs'].reshape(-1, actor.num_in)
    else:
        s['obs_compact'] = batch['obs_compact'].reshape(-1, batch['obs_compact'].shape[-1])
    return s


def rows_batch(batch, U, B):
    """A batch (or a flattened source) with observation rows: the compact record unpacked, everything else as it is."""
    from deepcomp_amd.fragment import FragmentCodec
    rows = {k: t for k, t in batch.items() if k != 'obs_compact'}
    rows['obs'] = FragmentCodec(U, B).unpack(batch['obs_compact'])
    return rows


def as_rows(src, actor):
    """The same source with observation rows: a compact source unpacked record by record."""
    if 'obs' in src:
        return src
    rows = rows_batch(src, actor.U, actor.B)
    rows['obs'] = rows['obs'].reshape(-1, actor.num_in)
    return rows


def outputs(torch, rows, heads, pad=0):
    return {k: torch.full((rows + pad, heads) if k == 'logp' else (rows + pad,), float('nan'), device='cuda') for k in OUTS}


def check_against_gathered(torch, learner, src, index, num_active=None):
    """grads_indexed / evaluate_indexed against grads / evaluate on the gathered rows; returns the indexed call's outputs."""
    from deepcomp_amd.learner import ARRAYS
    a = learner.actor
    rows_src = as_rows(src, a)
    n_src = rows_src['obs'].shape[0]
    pick = index.long() if index is not None else torch.arange(n_src, device='cuda')
    n = int(pick.numel())
    gathered = {k: t.index_select(0, pick).contiguous() for k, t in rows_src.items()}
    want_out, got_out = outputs(torch, n, a.heads), outputs(torch, n, a.heads)
    want_stats = learner.grads(**gathered, num_active=num_active, **want_out).clone()
    want = learner.read('grads')
    got_stats = learner.grads_indexed(src, index, num_active=num_active, **got_out)
    got = learner.read('grads')
    assert torch.equal(tbits(torch, got_stats), tbits(torch, want_stats)), (got_stats, want_stats)
    for name in ARRAYS:
        assert np.array_equal(got[name], want[name]), name
        assert np.isfinite(got[name]).all(), name
    assert any(np.abs(want[name]).max() > 0 for name in ('w1', 'vw1'))
    for k in OUTS:
        assert torch.equal(tbits(torch, got_out[k]), tbits(torch, want_out[k])), k
    if 'actions' in gathered:
        e_want = learner.evaluate(gathered['obs'], gathered['actions'], num_active=num_active)
        e_got = learner.evaluate_indexed(src, index, num_active=num_active)
        for x, y in zip(e_got, e_want):
            assert torch.equal(tbits(torch, x), tbits(torch, y))
    return got_stats, got, got_out


def shuffled(torch, n_src, n, seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return torch.randperm(n_src, generator=g, device='cuda')[:n].to(torch.int32).contiguous()


def same_state(s1, s2, stepped=False):
    """Two learner states equal bit for bit; stepped: and they have taken a step (a comparison of two untouched learners says nothing)."""
    from deepcomp_amd.learner import ARRAYS
    assert s1['step'] == s2['step'] and s1['kl_coeff'] == s2['kl_coeff'] and (not stepped or s1['step'] > 0)
    for k in ('weights', 'm', 'v'):
        for n in ARRAYS:
            assert np.array_equal(s1[k][n], s2[k][n]), (k, n)


def gathered_update(torch, learner, batch, num_sgd_iter, minibatch_rows, seed, num_active=None):
    """The SGD phase written out on rows: standardise, seeded randperm, index_select of all seven tensors per minibatch, grads, apply."""
    a = learner.actor
    src = source(batch, a)
    N = src['obs'].shape[0]
    kernel_active = None
    if num_active is not None and num_active < a.U:
        if a.heads == 1:
            keep = torch.nonzero(torch.arange(N, device='cuda') % a.U < num_active).reshape(-1)
            src = {k: t.index_select(0, keep) for k, t in src.items()}
            N = int(keep.numel())
        else:
            kernel_active = num_active
    adv = src['advantages']
    src['advantages'] = (adv - adv.mean()) / adv.std(unbiased=False).clamp_min(1e-4)
    mb = min(minibatch_rows, N)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed)
    for _ in range(num_sgd_iter):
        perm = torch.randperm(N, generator=gen, device='cuda')
        for s in range(0, N, mb):
            idx = perm[s:s + mb]
            learner.grads(**{k: t.index_select(0, idx) for k, t in src.items()}, num_active=kernel_active)
            learner.apply()


# ================================================================================================ policy set
def set_member(name, seed, value=True, **over):
    from deepcomp_amd.actor import FcnetActor
    U, B, H, act, _ = fc.SET_SHAPES[name]
    U, B, H, act = over.get('U', U), over.get('B', B), over.get('H', H), over.get('activation', act)
    w = FcnetActor.random_weights('multi', U, B, H, seed=seed, bias_std=0.1)
    vw = FcnetActor.random_value_weights('multi', U, B, H, seed=seed, bias_std=0.1, shared=over.get('shared', False)) if value else None
    return FcnetActor('multi', U, B, w, activation=act, value_weights=vw)


def set_distinct(name, value=True):
    from deepcomp_amd.policy_set import PerUEActor
    sp = fc.SET_SLOTS[name]
    return PerUEActor([set_member(name, 10 + p, value) for p in range(max(sp) + 1)], sp)


def set_run(torch, actor, obs, compact, mode, guard=0, **kw):
    """One launch into fresh buffers: mode 'a' = actions, 'av' = actions with the value, 'v' = the value alone.  Floats start as NaN
    (an unwritten element then equals nothing); guard > 0 puts that many pattern elements behind every output."""
    E = obs.shape[0]
    rows = E * actor.U
    full = {}

    def buf(key, n, dtype, fill):
        t = torch.full((n + guard,), fill, dtype=dtype, device='cuda')
        t[n:] = 0x5A if dtype == torch.uint8 else -12345.0
        full[key] = (t, n)
        return t[:n]
    out = {}
    if mode == 'v':
        out['vf'] = buf('vf', rows, torch.float32, float('nan'))
        actor.value(obs, compact=compact, out=out['vf'])
    else:
        out['act'] = buf('act', rows, torch.uint8, 0xEE).view(E, actor.U)
        out['logits'] = buf('logits', rows * actor.num_logits, torch.float32, float('nan')).view(rows, actor.num_logits)
        out['logp'] = buf('logp', rows * actor.heads, torch.float32, float('nan')).view(rows, actor.heads)
        if mode == 'av':
            out['vf'] = buf('vf', rows, torch.float32, float('nan'))
        actor.actions(obs, compact=compact, out=out['act'], logits=out['logits'], logp=out['logp'], vf=out.get('vf'), **kw)
    torch.cuda.synchronize()
    for key, (t, n) in full.items():
        tail = t[n:]
        assert bool((tail == (0x5A if t.dtype == torch.uint8 else -12345.0)).all()), f'{key}: written past its end'
    return out


def set_nrows(out):
    return out['vf'].numel() if 'vf' in out else out['act'].numel()


def set_same(torch, got, want, rows=None):
    """Every output of two launches equal, bit for bit (NaN, the initial fill, equals nothing); rows: at these decision rows only."""
    assert got.keys() == want.keys()
    for k in got:
        a, b = got[k].reshape(set_nrows(got), -1), want[k].reshape(set_nrows(want), -1)
        if rows is not None:
            a, b = a[rows], b[rows]
        assert torch.equal(a, b), k


SET_BATCH = {}


def set_batch(torch, compact):
    """One collect() batch of (a)'s shape at T = 5 driven by the distinct set, computed once: (batch, the same with observation rows)."""
    if compact not in SET_BATCH:
        from deepcomp_amd.sampler import collect
        U, B, _, _, E = fc.SET_SHAPES['a']
        batch = collect(env('multi', E, U, B), set_distinct('a'), fc.SET_T, gamma=0.99, lam=0.95, compact=compact, dist_inputs=True)
        SET_BATCH[compact] = (batch, rows_batch(batch, U, B) if compact else batch)
    return SET_BATCH[compact]


# ================================================================================================ grouped learner
def policy_set(U, B, H, act, slots, seed=10):
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.policy_set import PerUEActor
    members = [FcnetActor('multi', U, B, FcnetActor.random_weights('multi', U, B, H, seed=seed + p, bias_std=0.1), activation=act,
                          value_weights=FcnetActor.random_value_weights('multi', U, B, H, seed=seed + p, bias_std=0.1))
               for p in range(max(slots) + 1)]
    return PerUEActor(members, slots)


def per_ue_learner(pset, max_rows=64):
    from deepcomp_amd.policy_set import PerUELearner
    return PerUELearner(pset, max_rows=max_rows, **dict(HYPER, lr=1e-3))


GROUP_BATCH = {}


def group_collected(key, U, B, H, act, E, T, slots, compact):
    """One collect() batch of the shape, driven by a set of distinct members; computed once per key."""
    if key not in GROUP_BATCH:
        from deepcomp_amd.sampler import collect
        GROUP_BATCH[key] = collect(env('multi', E, U, B), policy_set(U, B, H, act, slots), T, gamma=0.99, lam=0.95, compact=compact, dist_inputs=True)
    return GROUP_BATCH[key]


def same_run(got, want, learner_g, learner_s):
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        assert g == w, p
        if g is not None:
            assert all(np.isfinite(v) for v in g.values())
            same_state(learner_g.learners[p].state_dict(), learner_s.learners[p].state_dict(), stepped=True)


def twins(name, max_rows=64):
    U, B, H, act, E, T, slots, compact = group_cases.GROUP_CASES[name]
    batch = group_collected(name, U, B, H, act, E, T, slots, compact)
    return batch, per_ue_learner(policy_set(U, B, H, act, slots), max_rows), per_ue_learner(policy_set(U, B, H, act, slots), max_rows)


def c_group(learners):
    """dcomp_learner_group_create over the learners' handles: (return code, handle, the library's message)."""
    from deepcomp_amd import _lib
    L = _lib.load()
    arr = (ctypes.c_void_p * len(learners))(*[ln._h.value for ln in learners])
    cfg = _lib.DcompLearnerGroupCfg(ctypes.sizeof(_lib.DcompLearnerGroupCfg), len(learners), arr)
    h = ctypes.c_void_p()
    rc = L.dcomp_learner_group_create(ctypes.byref(cfg), ctypes.byref(h))
    return rc, h, L.dcomp_last_error().decode()


def c_group_batch(src, index, rows, compact, source_rows=None):
    from deepcomp_amd import _lib
    obs = src['obs_compact' if compact else 'obs']
    n = src['actions'].shape[0] if source_rows is None else source_rows
    arr = (ctypes.c_int64 * len(rows))(*rows)
    b = _lib.DcompGroupBatch(ctypes.sizeof(_lib.DcompGroupBatch), _lib.ACTOR_COMPACT if compact else _lib.ACTOR_ROWS, n, obs.data_ptr(),
                             src['actions'].data_ptr(), src['old_logp'].data_ptr(), src['old_logits'].data_ptr(), src['advantages'].data_ptr(),
                             src['value_targets'].data_ptr(), src['old_vf'].data_ptr(), index.data_ptr(), index.shape[1], arr)
    b._keep = arr
    return b


def c_hypers(learners):
    from deepcomp_amd import _lib
    return (_lib.DcompPpoHyper * len(learners))(*[ln._hyper_struct() for ln in learners])


# ================================================================================================ accumulated gradients
def shard(batch, r, R, E, U, T):
    """Rank r's envs of a batch: every per-row tensor is [T, E, U, ...] flattened; the compact record is [T, E, words]."""
    lo, hi = r * E // R, (r + 1) * E // R
    keys = ('actions', 'action_logp', 'action_dist_inputs', 'advantages', 'value_targets', 'vf_preds')
    keys = ('obs',) + keys if 'obs' in batch else keys
    out = {k: batch[k].reshape(T, E, U, -1)[:, lo:hi].reshape(T, (hi - lo) * U, -1).contiguous() for k in keys}
    if 'obs' not in batch:
        out['obs_compact'] = batch['obs_compact'][:, lo:hi].contiguous()
    return out


def flat(grads):
    from deepcomp_amd.learner import ARRAYS
    return np.concatenate([grads[n].reshape(-1) for n in ARRAYS])


WHOLE = {}


def whole(torch, shape, compact=False):
    """Per shape and source format, computed once and left unchanged: the collect() batch, a shuffled index of fc.ACCUM_ROWS positions,
    the rows it picks (gathered), and grads() on all of them by a learner with max_rows = fc.ACCUM_ROWS: statistics and gradients."""
    key = (shape, compact)
    if key not in WHOLE:
        kind, E, U, B, H, T = shape
        w, vw, batch = collected(torch, kind, E, U, B, H, 'tanh', T, compact)
        learner = ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=fc.ACCUM_ROWS)
        src = source(batch, learner.actor)
        n_src = src['actions'].shape[0]
        assert n_src == 6464
        index = shuffled(torch, n_src, fc.ACCUM_ROWS, 7)
        gathered = {k: t.index_select(0, index.long()).contiguous() for k, t in as_rows(src, learner.actor).items()}
        stats = learner.grads(**gathered).cpu().numpy()
        WHOLE[key] = dict(w=w, vw=vw, learner=learner, src=src, index=index, gathered=gathered, stats=stats, grads=learner.read('grads'))
    return WHOLE[key]


def now(c):
    """The weights the case's learner runs (perturbed against the ones the batch was collected with), as the references take them."""
    if 'w_now' not in c:
        from deepcomp_amd import learner as lm
        c['w_now'], c['vw_now'] = lm.split_weights(c['learner'].read('weights'))
    return c


TERMS = {}


def row_terms(c, shape):
    """mean |per-row term| of the five statistics, from the float64 model on the gathered rows (computed once per shape)."""
    if shape not in TERMS:
        from deepcomp_amd import learner as lm
        host = {k: t.cpu().numpy() for k, t in c['gathered'].items()}
        ref64 = lm.ppo_loss_reference(c['w_now'], c['vw_now'], host, HYPER, 'tanh', 'float64')
        r = {k: ref64[2][k].numpy() for k in ('surr', 'kl', 'entropy', 'vf_loss')}
        hy = HYPER
        total = -r['surr'] + hy['kl_coeff'] * r['kl'] + hy['vf_loss_coeff'] * r['vf_loss'] - hy['entropy_coeff'] * r['entropy']
        TERMS[shape] = (ref64, {'total_loss': np.abs(total).mean(), 'policy_loss': np.abs(r['surr']).mean(), 'vf_loss': np.abs(r['vf_loss']).mean(),
                                'kl': np.abs(r['kl']).mean(), 'entropy': np.abs(r['entropy']).mean()})
    return TERMS[shape]
