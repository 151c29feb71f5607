"""GPU tests of the value function in the actor kernel (dcomp_actor_set_value / dcomp_actor_actions_v, deepcomp_amd/actor.py), in both
forms RLlib's fcnet has: a value trunk of its own ('own') and value_out on the actor's second hidden layer ('shared').

Bars: (1) on integer data every vf equals the integer reference EXACTLY; (2) with tanh, random-init weights and real observations
the kernel's vf is within 2 x the error the CPU bf16 / f32 chain itself has against the float64 model on the same inputs (the bar
test_actor_gpu.py holds the logits to, for the same reason); (3) actions, logits and logp of a call with vf are bit-identical to
those of the call without; (4) the value-only call and (5) the compact record give bit-identical vf; (6) nothing is stored beyond
the batch's rows; (7) the refusals that need a live handle.  Shapes and constructions are those of tests/test_actor_gpu.py.
Measured kernel errors: profiles/r08_critic_numerics.txt."""
import ctypes

import numpy as np
import pytest

from tests import fcnet_cases as fc
from tests import fcnet_support as fs
from tests.fcnet_support import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SHAPES, IDS, FORMS = fc.BASE_SHAPES, fc.BASE_IDS, fc.FORMS


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES + [fc.BASE_LOOP_SHAPE], ids=IDS + ['loop2200x32x10h32'])
def test_value_integer_data_exact(torch_cuda, shape, form):
    """relu, inputs in {0, 1}, <= 8 entries of +-1 per column of each trunk matrix, wv with <= 4 entries of +-1, integer biases in
    [-2, 2]: every intermediate is an integer of magnitude <= 82 (exact in bf16), every value <= 4 * 82 + 2 (exact in f32)."""
    torch = torch_cuda
    from deepcomp_amd.actor import FcnetActor
    kind, E, U, B, H = shape
    rows = fc.rows_of(kind, E, U)
    for seed in (1, 2, 3):
        w = fc.int_weights(kind, U, B, H, seed)
        v = fc.int_value_weights(kind, U, B, H, seed, form)
        x = np.random.default_rng(100 + seed).integers(0, 2, size=fc.obs_shape(kind, E, U, B)).astype(np.float32)
        x2 = x.reshape(rows, -1).astype(np.float64)
        t = v if form == 'own' else w
        h = np.maximum(x2 @ t['w1'] + t['b1'], 0)
        h = np.maximum(h @ t['w2'] + t['b2'], 0)
        assert np.abs(h).max() <= 82
        ref = h @ v['wv'].astype(np.float64) + float(v['bv'][0])
        assert np.count_nonzero(v['wv']) <= 4 and np.abs(ref).max() <= 330
        actor = FcnetActor(kind, U, B, w, activation='relu', value_weights=v)
        assert actor.value_shared == (form == 'shared')
        vf = torch.full((rows,), float('nan'), device='cuda')
        actor.actions(torch.from_numpy(x).cuda(), sample=False, vf=vf)
        got = vf.cpu().numpy()
        bad = np.argwhere(got != ref.astype(np.float32))
        assert bad.size == 0, f'seed {seed}: {len(bad)} of {rows} values differ, first at row {bad[0]}: {got[tuple(bad[0])]} != {ref[tuple(bad[0])]}'


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_value_tanh_numerics(torch_cuda, shape, form):
    fs.check_value_tanh_numerics(torch_cuda, shape, form)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_policy_outputs_are_bit_identical_with_vf(torch_cuda, shape, form):
    fs.check_policy_outputs_are_bit_identical_with_vf(torch_cuda, shape, form)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_value_only_call_is_bit_identical(torch_cuda, shape, form):
    fs.check_value_only_call_is_bit_identical(torch_cuda, shape, form)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('E,U,B,H', [(300, 32, 10, 256), (9, 5, 32, 64)])
def test_compact_record_gives_bit_identical_vf(torch_cuda, E, U, B, H, form):
    """The rows one env writes with step_into and the record its twin writes with step_compact from equal state."""
    torch = torch_cuda
    from deepcomp_amd.actor import FcnetActor
    rows_env, comp_env = fs.env('multi', E, U, B), fs.env('multi', E, U, B)
    v = FcnetActor.random_value_weights('multi', U, B, H, seed=4, bias_std=0.1, shared=form == 'shared')
    actor = FcnetActor('multi', U, B, FcnetActor.random_weights('multi', U, B, H, seed=4, bias_std=0.1), value_weights=v)
    packed = torch.zeros((E, comp_env.compact_words), dtype=torch.int32, device='cuda')
    obs, rew, rew2 = torch.zeros_like(rows_env.obs), torch.zeros_like(rows_env.reward), torch.zeros_like(rows_env.reward)
    rows_env.reset()
    comp_env.reset_compact(packed)
    a = actor.act(rows_env)
    for t in range(3):
        rows_env.step_into(a, obs, rew)
        comp_env.step_compact(a, packed, rew2)
        rv, cv = torch.full((E * U,), float('nan'), device='cuda'), torch.full((E * U,), float('nan'), device='cuda')
        ra, rl, rp = fs.actor_run(torch, actor, obs, E * U, sample=True, seed=5, step=t, vf=rv)
        ca, cl, cp = fs.actor_run(torch, actor, packed, E * U, compact=True, sample=True, seed=5, step=t, vf=cv)
        assert torch.isfinite(rv).all()
        assert torch.equal(rv.view(torch.int32), cv.view(torch.int32)), t
        assert np.array_equal(ra, ca) and np.array_equal(fs.bits(rl), fs.bits(cl)) and np.array_equal(fs.bits(rp), fs.bits(cp)), t
        assert torch.equal(actor.value(packed, compact=True).view(torch.int32), rv.view(torch.int32)), t
        a = torch.from_numpy(ra).cuda()
    rows_env.check(); comp_env.check()


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[4]], ids=[IDS[0], IDS[4]])
def test_rows_beyond_the_batch_are_never_stored(torch_cuda, shape, form):
    """The last tile is partial at both shapes (21 and 9 rows): a vf buffer of rows + 64 floats filled with NaN keeps its last 64."""
    torch = torch_cuda
    c = fs.value_case(torch, shape, form)
    rows = c['rows']
    for only in (False, True):
        buf = torch.full((rows + 64,), float('nan'), device='cuda')
        if only:
            c['actor'].value(c['obs'], out=buf[:rows])
        else:
            c['actor'].actions(c['obs'], sample=False, vf=buf[:rows])
        got = buf.cpu().numpy()
        assert np.isnan(got[rows:]).all(), only
        assert np.array_equal(fs.bits(got[:rows]), fs.bits(c['only'])), only


def test_refusals_that_need_a_handle(torch_cuda):
    """A handle without a value function, a second set_value, and the Python checks of vf."""
    torch = torch_cuda
    from deepcomp_amd import _lib
    from deepcomp_amd.actor import FcnetActor
    kind, U, B, H = 'multi', 4, 5, 32
    actor = FcnetActor.random(kind, U, B, hidden=H, seed=1)
    obs = torch.zeros((2, U, 4 * B + 1), device='cuda')
    act, vf = torch.zeros((2, U), dtype=torch.uint8, device='cuda'), torch.zeros(2 * U, device='cuda')
    run = _lib.DcompActorRun(ctypes.sizeof(_lib.DcompActorRun), 0, 2, U, 0, 0, 0, 0, None, None)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    assert actor._L.dcomp_actor_actions_v(actor._h, ctypes.byref(run), p(obs), p(act), p(vf), None) == _lib.EINVAL
    assert b'no value function' in actor._L.dcomp_last_error()
    with pytest.raises(ValueError):
        actor.actions(obs, vf=vf)
    with pytest.raises(ValueError):
        actor.value(obs)
    actor.set_value(FcnetActor.random_value_weights(kind, U, B, H, seed=2, shared=True), shared=True)
    with pytest.raises(ValueError, match='already'):
        actor.set_value(FcnetActor.random_value_weights(kind, U, B, H, seed=3, shared=True), shared=True)
    with pytest.raises(ValueError, match='already'):
        actor.set_value(FcnetActor.random_value_weights(kind, U, B, H, seed=3), shared=False)
    actor.actions(obs, vf=vf)
    for bad in (torch.zeros(2 * U + 1, device='cuda'), torch.zeros(2 * U, dtype=torch.float64, device='cuda'), torch.zeros(2 * U)):
        with pytest.raises(ValueError):
            actor.actions(obs, vf=bad)
    torch.cuda.synchronize()
