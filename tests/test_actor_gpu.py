"""GPU tests of the fcnet actor kernel (dcomp_actor_create / dcomp_actor_actions, deepcomp_amd/actor.py).

Bars: (1) on integer data every logit equals the integer reference EXACTLY (any fragment-map, k-permutation or padding error
shows); (2) with tanh and random-init weights the kernel's logits are within 2 x the error the CPU bf16 / f32 chain itself has
against the float64 model, measured on the same inputs; (3-5) the action is the first maximum of the kernel's own logits (+ the
Gumbel noise recomputed on the host through the oracle's Philox), logp its log-softmax; (6) draws are keyed by (seed, step,
global row); (7) sampled actions follow softmax(logits); (8) the compact record gives bit-identical results; (9) the actor drives
env.step.  Measured kernel errors: profiles/r07_actor_numerics.txt."""
import numpy as np
import pytest

from tests import fcnet_cases as fc
from tests import fcnet_support as fs
from tests.fcnet_support import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SHAPES, LOOP_SHAPE, IDS = fc.BASE_SHAPES, fc.BASE_LOOP_SHAPE, fc.BASE_IDS


@pytest.mark.parametrize('shape', SHAPES + [LOOP_SHAPE], ids=IDS + ['loop2200x32x10h32'])
def test_integer_data_exact(torch_cuda, shape):
    """relu, inputs in {0, 1}, <= 8 entries of +-1 per column of W1 / W2, <= 4 per column of W3, integer biases in [-2, 2]: every
    intermediate is an integer of magnitude <= 82 (exact in bf16), every logit <= 330 (exact in f32)."""
    torch = torch_cuda
    from deepcomp_amd.actor import FcnetActor
    kind, E, U, B, H = shape
    rows = fc.rows_of(kind, E, U)
    for seed in (1, 2, 3):
        w = fc.int_weights(kind, U, B, H, seed)
        x = np.random.default_rng(100 + seed).integers(0, 2, size=fc.obs_shape(kind, E, U, B)).astype(np.float32)
        x2 = x.reshape(rows, -1).astype(np.float64)
        h = np.maximum(x2 @ w['w1'] + w['b1'], 0)
        h = np.maximum(h @ w['w2'] + w['b2'], 0)
        assert np.abs(h).max() <= 82
        ref = h @ w['w3'] + w['b3']
        assert np.abs(ref).max() <= 330
        actor = FcnetActor(kind, U, B, w, activation='relu')
        act, logits, _ = fs.actor_run(torch, actor, torch.from_numpy(x).cuda(), rows, sample=False)
        bad = np.argwhere(logits != ref.astype(np.float32))
        assert bad.size == 0, f'seed {seed}: {len(bad)} of {ref.size} logits differ, first at (row, logit) {bad[0]}: {logits[tuple(bad[0])]} != {ref[tuple(bad[0])]}'
        first = ref.reshape(rows, actor.heads, B + 1).argmax(axis=-1)            # np.argmax: the first maximum
        assert np.array_equal(act.reshape(rows, actor.heads), first)


# ---------------------------------------------------------------------------------------------------------------- real observations
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_tanh_numerics(torch_cuda, shape):
    fs.check_tanh_numerics(torch_cuda, shape)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_greedy_is_first_maximum_of_own_logits(torch_cuda, shape):
    fs.check_greedy_is_first_maximum_of_own_logits(torch_cuda, shape)


@pytest.mark.parametrize('kind', ['multi', 'central'])
def test_unlisted_slots_get_action_zero(torch_cuda, kind):
    """An env with UE arrival: slots (multi-agent) / heads (central) >= the number of listed UEs get action 0, the listed ones the
    first maximum of their logits."""
    torch = torch_cuda
    from deepcomp_amd.actor import FcnetActor
    E, U0, B = 6, 4, 5
    env = fs.env(kind, E, U0, B, ue_arrival={2: 2, 4: -1})
    U = env.U
    actor = FcnetActor.random(kind, U, B, hidden=64, seed=3, bias_std=0.1)
    env.reset()
    seen = set()
    for t in range(6):
        n = env.num_ue
        seen.add(n)
        rows = fc.rows_of(kind, E, U)
        logits = torch.empty((rows, actor.num_logits), device='cuda')
        for sample in (False, True):
            act = actor.act(env, sample=sample)
            a = act.cpu().numpy()
            assert (a[:, n:] == 0).all(), (t, n)
        actor.actions(env.obs, sample=False, num_active=n, logits=logits)
        own = logits.cpu().numpy().reshape(rows, actor.heads, B + 1).argmax(axis=-1).reshape(E, U)
        assert np.array_equal(actor.act(env, sample=False).cpu().numpy()[:, :n], own[:, :n])
        env.step(actor.act(env, sample=True))
    env.check()
    assert len(seen) > 1 and min(seen) < U


def _sub(shape):
    """At most 2 048 decision rows of a case (the first envs of the large one)."""
    kind, E, U, B, H = shape
    return min(E, 2048 // U) if kind == 'multi' else min(E, 2048)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_sampled_action_matches_host_gumbel(torch_cuda, shape):
    """action == first argmax of the kernel's logits + Gumbel noise recomputed in float64 from oracle.philox4x32_10.  Decisions whose
    top-two gap of that sum is below 1e-3 are left out (device logf vs float64 log), at most 1 % of them."""
    torch = torch_cuda
    from deepcomp_amd.actor import gumbel_noise
    from oracle import oracle as orc
    kind, E, U, B, H = shape
    c = fs.actor_case(torch, shape)
    actor, Es = c['actor'], _sub(shape)
    rows = fc.rows_of(kind, Es, U)
    seed, step, row_base = 0x1234ABCD5678, 77, 1000
    act, logits, _ = fs.actor_run(torch, actor, c['obs'][:Es].contiguous(), rows, sample=True, seed=seed, step=step, row_base=row_base)
    assert np.array_equal(logits, c['logits'][:rows])
    g = gumbel_noise(orc.philox4x32_10, seed, step, row_base + np.arange(rows), actor.heads, B + 1)
    y = logits.astype(np.float64).reshape(rows, actor.heads, B + 1) + g
    top = np.sort(y, axis=-1)
    clear = (top[..., -1] - top[..., -2]) >= 1e-3
    left_out = int((~clear).sum())
    print(f'sampled {shape}: {left_out} of {clear.size} decisions within 1e-3 of a tie')
    assert left_out <= 0.01 * clear.size
    got = act.reshape(rows, actor.heads)
    assert np.array_equal(got[clear], y.argmax(axis=-1)[clear])


@pytest.mark.parametrize('shape', SHAPES[:6], ids=IDS[:6])
def test_logp_is_log_softmax_of_chosen_action(torch_cuda, shape):
    """|logit| <= 10 (the head's weights scaled): logp within 1e-4 of log_softmax(kernel logits)[action] in float64 -- the bound is
    (N + a few) 2^-24 x 10 for N <= 65 summands plus logf."""
    torch = torch_cuda
    from deepcomp_amd.actor import FcnetActor
    kind, E, U, B, H = shape
    c = fs.actor_case(torch, shape)
    s = 9.9 / float(np.abs(c['logits']).max())
    w = dict(c['actor'].weights)
    w['w3'], w['b3'] = w['w3'] * np.float32(s), w['b3'] * np.float32(s)
    actor = FcnetActor(kind, U, B, w, activation='tanh')
    for sample in (True, False):
        act, logits, logp = fs.actor_run(torch, actor, c['obs'], c['rows'], sample=sample, seed=9, step=3)
        assert np.abs(logits).max() <= 10.0
        lg = logits.astype(np.float64).reshape(c['rows'], actor.heads, B + 1)
        ls = lg - (np.log(np.exp(lg - lg.max(-1, keepdims=True)).sum(-1, keepdims=True)) + lg.max(-1, keepdims=True))
        want = np.take_along_axis(ls, act.reshape(c['rows'], actor.heads, 1).astype(np.int64), axis=-1)[..., 0]
        err = np.abs(logp.astype(np.float64) - want).max()
        print(f'logp {shape} sample={sample}: max abs err {err:.3e}')
        assert err <= 1e-4


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[4]], ids=[IDS[1], IDS[4]])
def test_keying(torch_cuda, shape):
    torch = torch_cuda
    kind, E, U, B, H = shape
    c = fs.actor_case(torch, shape)
    actor, obs = c['actor'], c['obs']
    a0 = actor.actions(obs, seed=11, step=5).cpu().numpy()
    assert np.array_equal(a0, actor.actions(obs, seed=11, step=5).cpu().numpy())
    assert not np.array_equal(a0, actor.actions(obs, seed=11, step=6).cpu().numpy())
    assert not np.array_equal(a0, actor.actions(obs, seed=12, step=5).cpu().numpy())
    # the batch as two calls with row_base set == the slices of the one-call result, byte for byte (and with a base of its own)
    cut = 2 if kind == 'multi' else 4
    rpe = U if kind == 'multi' else 1
    whole = actor.actions(obs, seed=11, step=5, row_base=7 * rpe).cpu().numpy()
    lo = actor.actions(obs[:cut].contiguous(), seed=11, step=5, row_base=7 * rpe).cpu().numpy()
    hi = actor.actions(obs[cut:].contiguous(), seed=11, step=5, row_base=(7 + cut) * rpe).cpu().numpy()
    assert np.array_equal(whole, np.concatenate([lo, hi]))
    assert not np.array_equal(whole, a0)
    with pytest.raises(ValueError):
        actor.actions(obs, seed=1, step=1, row_base=2 ** 32 - 1)


def test_sampled_actions_follow_softmax(torch_cuda):
    """One observation row 65 536 times at 11 actions: chi-square of the counts against softmax(kernel logits) below the 1e-6 upper
    quantile, at fixed seeds."""
    torch = torch_cuda
    from scipy import stats
    shape = SHAPES[1]
    c = fs.actor_case(torch, shape)
    actor = c['actor']
    U, B = shape[2], shape[3]
    E = 65536 // U
    obs = c['obs'][2:3, 5:6].expand(E, U, 4 * B + 1).contiguous()
    lg = c['logits'][2 * U + 5].astype(np.float64)
    p = np.exp(lg - lg.max())
    p /= p.sum()
    limit = stats.chi2.ppf(1 - 1e-6, B)
    for seed, step in ((1, 0), (2, 9), (987654321987, 4000)):
        a = actor.actions(obs, seed=seed, step=step).cpu().numpy().ravel()
        counts = np.bincount(a, minlength=B + 1)
        assert counts.sum() == 65536 and len(counts) == B + 1
        chi = float(((counts - 65536 * p) ** 2 / (65536 * p)).sum())
        print(f'distribution seed {seed} step {step}: chi-square {chi:.2f} (limit {limit:.2f}, {B} degrees of freedom)')
        assert chi < limit


@pytest.mark.parametrize('E,U,B,H', [(300, 32, 10, 256), (9, 5, 32, 64)])
def test_compact_record_from_the_step(torch_cuda, E, U, B, H):
    """(a) the rows one env writes with step_into and the record its twin writes with step_compact from equal state: logits and
    actions bit-identical."""
    torch = torch_cuda
    from deepcomp_amd.actor import FcnetActor
    rows_env, comp_env = fs.env('multi', E, U, B), fs.env('multi', E, U, B)
    actor = FcnetActor.random('multi', U, B, hidden=H, seed=4, bias_std=0.1)
    packed = torch.zeros((E, comp_env.compact_words), dtype=torch.int32, device='cuda')
    obs, rew, rew2 = torch.zeros_like(rows_env.obs), torch.zeros_like(rows_env.reward), torch.zeros_like(rows_env.reward)
    rows_env.reset()
    comp_env.reset_compact(packed)
    a = actor.act(rows_env)
    for t in range(4):
        rows_env.step_into(a, obs, rew)
        comp_env.step_compact(a, packed, rew2)
        ra, rl, rp = fs.actor_run(torch, actor, obs, E * U, sample=True, seed=5, step=t)
        ca, cl, cp = fs.actor_run(torch, actor, packed, E * U, compact=True, sample=True, seed=5, step=t)
        assert np.array_equal(fs.bits(rl), fs.bits(cl)) and np.array_equal(ra, ca) and np.array_equal(fs.bits(rp), fs.bits(cp)), t
        a = torch.from_numpy(ra).cuda()
    rows_env.check(); comp_env.check()


@pytest.mark.parametrize('B', [10, 64])
def test_compact_record_from_pack_fragment(torch_cuda, B):
    """(b) dcomp_pack_fragment of synthetic valid rows, including unlisted (all-zero) slots of a dynamic env."""
    torch = torch_cuda
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.fragment import FragmentCodec
    E, U, listed = 37, 6, 4
    rng = np.random.default_rng(B)
    x = np.zeros((E, U, 4 * B + 1), dtype=np.float32)
    x[:, :listed, :B] = rng.integers(0, 2, size=(E, listed, B))
    dr = rng.random((E, listed, B)).astype(np.float32)
    dr[np.arange(E)[:, None], np.arange(listed)[None, :], rng.integers(0, B, size=(E, listed))] = 1.0      # a listed UE's best station has dr == 1
    x[:, :listed, B:2 * B] = dr
    x[:, :listed, 2 * B:4 * B] = rng.random((E, 1, 2 * B)).astype(np.float32)                               # per-env columns, replicated
    x[:, :listed, 4 * B] = rng.uniform(-1, 1, size=(E, listed))
    obs = torch.from_numpy(x).cuda()
    codec = FragmentCodec(U, B)
    packed = codec.pack(obs)
    codec.check()
    assert torch.equal(codec.unpack(packed).view(torch.int32), obs.view(torch.int32))
    actor = FcnetActor.random('multi', U, B, hidden=64, seed=B, bias_std=0.1)
    for sample in (False, True):
        ra, rl, rp = fs.actor_run(torch, actor, obs, E * U, sample=sample, seed=8, step=2, num_active=listed)
        ca, cl, cp = fs.actor_run(torch, actor, packed, E * U, compact=True, sample=sample, seed=8, step=2, num_active=listed)
        assert np.array_equal(fs.bits(rl), fs.bits(cl)) and np.array_equal(ra, ca) and np.array_equal(fs.bits(rp), fs.bits(cp))
        assert (ra[:, listed:] == 0).all()


@pytest.mark.parametrize('kind,E,U,B', [('multi', 64, 32, 10), ('central', 64, 10, 5)])
def test_actor_drives_the_env(torch_cuda, kind, E, U, B):
    """FcnetActor.act(env) -> env.step for 20 steps; greedy: the same trajectory (connection masks, every env, every step) as the
    one driven by the greedy actions of reference_logits (float64 form).  Decisions whose float64 top-two logit gap is below 4 x the
    kernel's error against the float64 model (measured on that step's rows, as in test_tanh_numerics) are excluded -- there the
    reference env takes the kernel's action, so that both stay on one trajectory -- and at most 2 % of the decisions may be.
    The head's biases are N(0, 4): a head with marked preferences, as a trained policy has.  The share of decisions inside the
    exclusion band is a property of the model, not of what computes it: 4 x err x the density of the top-two gap at zero, and that
    density falls as 1 / (spread of the logits) while err (the bf16 roundings of h1 and h2) does not grow with the biases.  A
    random-init head with N(0, 0.1) biases has 11 nearly equal logits: 5 - 7 % of its decisions are within 4 x the CPU bf16 chain's
    own error of a tie (2 048 synthetic rows), and with N(0, 1) biases 4.6 % of the env's real rows were (1 872 of 40 960; the kernel
    decided 51 of those the other way, every clear decision and every connection mask equal) -- both above the cap whatever
    computes the logits.  With N(0, 4) the band holds about a quarter of that."""
    torch = torch_cuda
    from deepcomp_amd.actor import FcnetActor
    dev_env, ref_env, sampled = fs.env(kind, E, U, B), fs.env(kind, E, U, B), fs.env(kind, E, U, B)
    w = FcnetActor.random_weights(kind, U, B, 256, seed=21, bias_std=0.1)
    w['b3'] = np.random.default_rng(21).normal(0.0, 4.0, size=w['b3'].shape).astype(np.float32)
    actor = FcnetActor(kind, U, B, w)
    dev_env.reset(); ref_env.reset(); sampled.reset()
    rows = fc.rows_of(kind, E, U)
    close = changed = 0
    for t in range(20):
        sampled.step(actor.act(sampled, sample=True))
        assert torch.equal(dev_env.conn, ref_env.conn), f'connection masks differ before step {t}'
        assert torch.equal(dev_env.obs.view(torch.int32), ref_env.obs.view(torch.int32))
        x = ref_env.obs.cpu().numpy().reshape(rows, -1)
        ref64 = actor.reference_logits(x, form='float64').numpy()
        logits = torch.empty((rows, actor.num_logits), device='cuda')
        actor.actions(dev_env.obs, sample=False, logits=logits)
        err = float(np.abs(logits.cpu().numpy() - ref64).max())
        lg = ref64.reshape(rows, actor.heads, B + 1)
        top = np.sort(lg, axis=-1)
        near = ((top[..., -1] - top[..., -2]) < 4 * err).reshape(E, U)
        a_ref = lg.argmax(axis=-1).reshape(E, U).astype(np.uint8)
        a_dev = actor.act(dev_env, sample=False)
        a_host = a_dev.cpu().numpy()
        assert np.array_equal(a_host[~near], a_ref[~near]), f'step {t}: a clear decision differs'
        close += int(near.sum())
        changed += int((a_host != a_ref).sum())
        dev_env.step(a_dev)
        ref_env.step(torch.from_numpy(np.where(near, a_host, a_ref)).cuda())
    assert torch.equal(dev_env.conn, ref_env.conn)
    dev_env.check(); ref_env.check(); sampled.check()
    print(f'end to end {kind}: {close} of {20 * E * U} decisions within 4 x err of a tie, {changed} of them decided the other way')
    assert close <= 0.02 * 20 * E * U
