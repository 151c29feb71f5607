"""GPU tests of the collector on envs with UE arrival and departure (deepcomp_amd/sampler.py: collect(by_ue=True), live_rows): what it
records is, bit for bit, what a plain loop of actor.act + env.step with a reset at the horizon sees on a twin env -- uid / uid_next
being the twin's env.uid before and after each step (after the step, before the reset) -- and advantages, value_targets and live are
gae_uid_reference's and the cut-out trajectories' (tests/gae_uid_cases.py) of the recorded columns.  episode_length = 6 with the
schedule of tests/gae_uid_cases.py: a batch of T = 9 crosses one boundary and ends inside an episode, the batch that follows it
without a gap ends on one, and so does one of T = 6.  Then the learner: update(rows=live_rows(batch)) never reads a row that does not
count."""
import numpy as np
import pytest

from tests import fcnet_support as fs
from tests import gae_uid_cases as gc
from tests.fcnet_support import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

B = 5
# initial UEs, envs, draws
CASES = [(5, 16, 'philox'), (66, 4, 'philox'), (5, 2, 'reference')]
IDS = ['u5-philox', 'u66-philox', 'u5-reference']


def _env(kind, E, U0, rng='philox', ue_arrival=gc.UE_ARRIVAL):
    from deepcomp_amd import scenarios
    from deepcomp_amd.entities import build_from_scenario
    from deepcomp_amd.env import BatchedMobileEnv
    m, bs, ues = build_from_scenario(scenarios.grid_map(B, 'mixed').with_ues(num_slow=U0))
    return BatchedMobileEnv(m, bs, ues, kind, num_envs=E, seed=42, episode_length=gc.HORIZON, rng=rng, rand_episodes=True, ue_arrival=ue_arrival)


def _actor(kind, U):
    from deepcomp_amd.actor import FcnetActor
    w = FcnetActor.random_weights(kind, U, B, 64, seed=11, bias_std=0.1)
    return FcnetActor(kind, U, B, w, value_weights=FcnetActor.random_value_weights(kind, U, B, 64, seed=11, bias_std=0.1))


def _twin_loop(torch, env, actor, T, started):
    """The plain loop; per step host-side copies of what the collector must have recorded."""
    if not started:
        env.reset()
    rec = []
    for t in range(T):
        obs, uid = env.obs.clone(), env.uid.clone()
        vf = torch.full((env.E * env.U,), float('nan'), device='cuda')
        a = actor.act(env, sample=True, vf=vf).clone()
        env.step(a)
        rew, uid_next = env.reward.clone(), env.uid.clone()
        done = env.time >= env.episode_length
        if done:
            env.reset()
        rec.append((obs, uid, a, vf, rew, uid_next, done))
    return rec, env.obs.clone()


def _check_batch(torch, env, twin, actor, b, T, compact, started):
    from deepcomp_amd.fragment import FragmentCodec
    from deepcomp_amd.sampler import gae_uid_reference
    E, U = env.E, env.U
    assert b['uid'].shape == b['uid_next'].shape == (T, E, U) and b['uid'].dtype == b['uid_next'].dtype == torch.int16
    assert b['live'].shape == (T, E * U) and b['live'].dtype == torch.uint8
    rec, last_obs = _twin_loop(torch, twin, actor, T, started)
    codec = FragmentCodec(U, B) if compact else None
    rows_of = (lambda p: codec.unpack(p.contiguous())) if compact else (lambda o: o)
    dones = b['dones'].cpu().numpy()
    for t, (obs, uid, a, vf, rew, uid_next, done) in enumerate(rec):
        assert torch.equal(fs.tbits(torch, rows_of(b['obs_compact'][t] if compact else b['obs'][t])), fs.tbits(torch, obs)), f'obs differ at t = {t}'
        assert torch.equal(b['actions'][t], a), f'actions differ at t = {t}'
        assert torch.equal(fs.tbits(torch, b['rewards'][t]), fs.tbits(torch, rew.reshape(-1))), f'rewards differ at t = {t}'
        assert torch.equal(fs.tbits(torch, b['vf_preds'][t]), fs.tbits(torch, vf)), f'vf_preds differ at t = {t}'
        assert torch.equal(b['uid'][t].reshape(-1), uid.reshape(-1)), f'uid differs at t = {t}'
        assert torch.equal(b['uid_next'][t].reshape(-1), uid_next.reshape(-1)), f'uid_next differs at t = {t}'
        assert int(dones[t]) == int(done), t
    assert torch.equal(fs.tbits(torch, rows_of(b['new_obs_last'])), fs.tbits(torch, last_obs)), 'new_obs_last differs'
    last_vf = None if dones[T - 1] else actor.value(b['new_obs_last'], compact=compact).cpu().numpy()
    cols = [b[k].cpu().numpy() for k in ('rewards', 'vf_preds', 'uid', 'uid_next')]
    got = [b[k].cpu().numpy().reshape(T, E, U) for k in ('advantages', 'value_targets', 'live')]
    for fn in (gae_uid_reference, gc.by_trajectory):
        want = fn(*cols, last_vf, dones, gc.GAMMA, gc.LAM)
        for g, w, name in zip(got, want, ('advantages', 'value_targets', 'live')):
            assert np.array_equal(gc.bits(g), gc.bits(w)), f'{name} differ from {fn.__name__}'
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    uid = cols[2].astype(np.uint16)
    assert (np.sort(uid != 0, axis=2)[:, :, ::-1] == (uid != 0)).all()                  # live slots are a prefix
    return dones, got[2]


@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
@pytest.mark.parametrize('U0,E,rng', CASES, ids=IDS)
def test_collect_by_ue_matches_the_plain_loop(torch_cuda, U0, E, rng, compact):
    """T = 9 over a horizon of 6: dones = 0 0 0 0 0 1 0 0 0.  The second collect into the same buffers continues at time 3 and ends on
    the boundary after next: dones = 0 0 1 0 0 0 0 0 1, no bootstrap."""
    torch = torch_cuda
    from deepcomp_amd.sampler import collect
    env, twin = _env('multi', E, U0, rng), _env('multi', E, U0, rng)
    assert env.dynamic and env.U == U0 + 2 and max(r for r, _ in env.schedule) == 2 and env.schedule == gc.SCHEDULE
    actor = _actor('multi', env.U)
    T = 9
    b = collect(env, actor, T, gamma=gc.GAMMA, lam=gc.LAM, compact=compact, by_ue=True)
    dones, live = _check_batch(torch, env, twin, actor, b, T, compact, started=False)
    assert dones.tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0]
    listed = {5: 48, 66: 597}[U0]                                # UEs listed over the nine steps, per env (5 5 7 6 4 4 | 5 5 7); four rows are departures
    assert int((b['uid'] != 0).sum()) == listed * E and int(live.sum()) == (listed - 4) * E
    env.check(); twin.check()
    assert env.time == twin.time == 3 and env.episode == twin.episode and env.num_ue == twin.num_ue

    b2 = collect(env, actor, T, gamma=gc.GAMMA, lam=gc.LAM, compact=compact, by_ue=True, out=b)
    assert b2 is b
    dones, _ = _check_batch(torch, env, twin, actor, b, T, compact, started=True)
    assert dones.tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 1]
    env.check(); twin.check()
    assert env.time == twin.time == 0


@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_collect_by_ue_ending_on_the_boundary(torch_cuda, compact):
    """T = 6 = the horizon: no bootstrap, every trajectory ends with next value 0."""
    torch = torch_cuda
    from deepcomp_amd.sampler import collect
    env, twin = _env('multi', 16, 5), _env('multi', 16, 5)
    actor = _actor('multi', env.U)
    b = collect(env, actor, 6, gamma=gc.GAMMA, lam=gc.LAM, compact=compact, by_ue=True)
    dones, live = _check_batch(torch, env, twin, actor, b, 6, compact, started=False)
    assert dones.tolist() == [0, 0, 0, 0, 0, 1] and int(live.sum()) == (31 - 3) * 16
    env.check(); twin.check()


@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_static_env_by_ue_is_the_plain_collector(torch_cuda, compact):
    torch = torch_cuda
    from deepcomp_amd.sampler import collect
    E, U, T = 16, 5, 9
    env, twin = _env('multi', E, U, ue_arrival=None), _env('multi', E, U, ue_arrival=None)
    assert not env.dynamic and env.uid is None
    actor = _actor('multi', U)
    got = collect(env, actor, T, gamma=gc.GAMMA, lam=gc.LAM, compact=compact, dist_inputs=True, by_ue=True)
    want = collect(twin, actor, T, gamma=gc.GAMMA, lam=gc.LAM, compact=compact, dist_inputs=True)
    assert sorted(set(got) - set(want)) == ['live', 'uid', 'uid_next']
    for k, t in want.items():
        assert torch.equal(got[k].view(torch.uint8), t.view(torch.uint8)), k
    assert bool(got['live'].all()) and bool((got['uid'] == torch.arange(1, U + 1, device='cuda')).all()) and torch.equal(got['uid'], got['uid_next'])
    assert want['dones'].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0]
    env.check(); twin.check()


def test_refusals(torch_cuda):
    from deepcomp_amd.sampler import collect
    dyn = _env('multi', 4, 5)
    actor = _actor('multi', dyn.U)
    with pytest.raises(NotImplementedError, match='by_ue=True'):
        collect(dyn, actor, 3)                                                            # still: a column is not one UE's trajectory
    central = _env('central', 4, 5)
    with pytest.raises(NotImplementedError, match='central'):
        collect(central, _actor('central', central.U), 3, by_ue=True)
    with pytest.raises(NotImplementedError, match='per-UE policy set'):
        collect(dyn, fs.policy_set(dyn.U, B, 32, 'tanh', [s % 2 for s in range(dyn.U)]), 3, by_ue=True)
    b = collect(dyn, actor, 3, by_ue=True)
    plain = {k: t for k, t in b.items() if k not in ('uid', 'uid_next', 'live')}
    with pytest.raises(ValueError):
        collect(dyn, actor, 3, by_ue=True, out=plain)                                     # buffers of a plain batch
    dyn.check()


@pytest.mark.parametrize('compact', [False, True], ids=['rows', 'compact'])
def test_training_on_the_live_rows_reads_no_other_row(torch_cuda, compact):
    """Two learners from the same weights: one trains on the batch, the other on a copy whose rows that do not count are NaN in every
    per-row field and in their observation rows.  Weights, Adam state and statistics are equal bit for bit, and finite."""
    torch = torch_cuda
    from deepcomp_amd import learner as lm
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.sampler import collect, live_rows
    E, T, H = 16, 9, 64
    env = _env('multi', E, 5)
    U = env.U
    w = FcnetActor.random_weights('multi', U, B, H, seed=1, bias_std=0.1)
    vw = FcnetActor.random_value_weights('multi', U, B, H, seed=1, bias_std=0.1)
    batch = collect(env, FcnetActor('multi', U, B, w, value_weights=vw), T, gamma=gc.GAMMA, lam=gc.LAM, compact=compact, dist_inputs=True, by_ue=True)
    rows = live_rows(batch)
    flat = batch['live'].reshape(-1)
    assert rows.dtype == torch.int64 and rows.device == flat.device and torch.equal(rows, torch.nonzero(flat).reshape(-1))
    assert rows.numel() == 44 * E

    dead = flat == 0
    poisoned = {k: t.clone() for k, t in batch.items()}
    for k in ('action_logp', 'action_dist_inputs', 'vf_preds', 'advantages', 'value_targets', 'rewards'):
        poisoned[k].view(T * E * U, -1)[dead] = float('nan')
    poisoned['actions'].view(-1)[dead] = 0xEE
    if compact:                                                    # a record holds a whole env: the per-UE words (dr[B] | utility | mask each) come first
        words = poisoned['obs_compact'].view(T * E, -1)
        assert words.shape[1] == U * (B + 2) + 2 * B
        nan_bits = torch.full((int(dead.sum()), B + 2), float('nan'), device='cuda').view(torch.int32)
        ue_words = words[:, :U * (B + 2)].reshape(T * E * U, B + 2)
        ue_words[dead] = nan_bits
        words[:, :U * (B + 2)] = ue_words.view(T * E, -1)
        assert not torch.equal(words, batch['obs_compact'].view(T * E, -1))
    else:
        poisoned['obs'].view(T * E * U, -1)[dead] = float('nan')

    learners = [fs.ppo_learner('multi', U, B, w, vw, 'tanh', max_rows=512, perturb=False, lr=1e-3) for _ in range(2)]
    out = [ln.update(bt, num_sgd_iter=2, minibatch_rows=256, seed=3, rows=rows) for ln, bt in zip(learners, (batch, poisoned))]
    assert out[0] == out[1] and all(np.isfinite(out[0][n]) for n in lm.STATS)
    s0, s1 = learners[0].state_dict(), learners[1].state_dict()
    fs.same_state(s0, s1, stepped=True)
    assert all(np.isfinite(s0['weights'][n]).all() for n in lm.ARRAYS) and np.abs(s0['weights']['w2'] - w['w2']).max() > 1e-5
