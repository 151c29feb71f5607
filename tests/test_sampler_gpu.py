"""GPU tests of the sample-batch collector (deepcomp_amd/sampler.py: collect): what it records is, bit for bit, what a plain Python
loop of actor.act + env.step with a reset at the horizon sees on a twin env; vf_preds and action_logp are the kernel's own of
separate calls; advantages and value_targets are gae_reference of the collected columns.  episode_length = 4: a batch of T = 6
crosses one boundary and ends inside an episode (bootstrap from new_obs_last), one of T = 4 ends on the boundary (no bootstrap)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [('multi', 64, 32, 10, False), ('multi', 64, 32, 10, True), ('central', 64, 10, 5, False)]
IDS = ['multi-rows', 'multi-compact', 'central-rows']
HORIZON, GAMMA, LAM = 4, 0.99, 0.95


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _env(kind, E, U, B, **kw):
    from deepcomp_amd import scenarios
    from deepcomp_amd.entities import build_from_scenario
    from deepcomp_amd.env import BatchedMobileEnv
    m, bs, ues = build_from_scenario(scenarios.grid_map(B, 'mixed').with_ues(num_slow=U))
    return BatchedMobileEnv(m, bs, ues, kind, num_envs=E, seed=42, episode_length=HORIZON, rng='philox', rand_episodes=True, **kw)


def _actor(kind, U, B):
    from deepcomp_amd.actor import FcnetActor
    w = FcnetActor.random_weights(kind, U, B, 64, seed=11, bias_std=0.1)
    return FcnetActor(kind, U, B, w, value_weights=FcnetActor.random_value_weights(kind, U, B, 64, seed=11, bias_std=0.1))


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _twin_loop(torch, env, actor, T, started):
    """The plain loop: per step the observation, actor.act, env.step, a reset at the horizon.  Returns per-step host copies."""
    if not started:
        env.reset()
    rec = []
    for t in range(T):
        obs = env.obs.clone()
        step_key = env.time + max(env.episode, 0) * env.episode_length
        a = actor.act(env, sample=True).clone()
        env.step(a)
        rew = env.reward.clone()
        done = env.time >= env.episode_length
        if done:
            env.reset()
        rec.append((obs, a, rew, done, step_key))
    return rec, env.obs.clone()


def _check_batch(torch, env, twin, actor, b, T, compact, started):
    from deepcomp_amd.fragment import FragmentCodec
    from deepcomp_amd.sampler import gae_reference
    kind_rows = b['vf_preds'].shape[1]
    rec, last_obs = _twin_loop(torch, twin, actor, T, started)
    codec = FragmentCodec(env.U, env.B) if compact else None
    rows_of = (lambda p: codec.unpack(p.contiguous())) if compact else (lambda o: o)
    dones = b['dones'].cpu().numpy()
    for t, (obs, a, rew, done, step_key) in enumerate(rec):
        got_obs = rows_of(b['obs_compact'][t] if compact else b['obs'][t])
        assert np.array_equal(_bits(got_obs), _bits(obs)), f'obs differ at t = {t}'
        assert torch.equal(b['actions'][t], a), f'actions differ at t = {t}'
        assert np.array_equal(_bits(b['rewards'][t]), _bits(rew.reshape(-1))), f'rewards differ at t = {t}'
        assert int(dones[t]) == int(done), t
        # the kernel's own value and logp of separate calls on the recorded observation
        src = b['obs_compact'][t] if compact else b['obs'][t]
        assert np.array_equal(_bits(actor.value(src, compact=compact)), _bits(b['vf_preds'][t])), f'vf_preds differ at t = {t}'
        logp = torch.full((kind_rows, actor.heads), float('nan'), device='cuda')
        rpe = env.U if actor.heads == 1 else 1
        again = actor.actions(src, compact=compact, sample=True, seed=env.seed_value, step=step_key, row_base=env.env_id_base * rpe,
                              num_active=env.num_ue, logp=logp)
        assert torch.equal(again, b['actions'][t])
        assert np.array_equal(_bits(logp), _bits(b['action_logp'][t])), f'action_logp differ at t = {t}'
        assert torch.isfinite(b['action_logp'][t]).all() and (b['action_logp'][t] <= 0).all()
    got_last = rows_of(b['new_obs_last'])
    assert np.array_equal(_bits(got_last), _bits(last_obs)), 'new_obs_last differs'
    last_vf = None if dones[T - 1] else actor.value(b['new_obs_last'], compact=compact).cpu().numpy()
    want_a, want_t = gae_reference(b['rewards'].cpu().numpy(), b['vf_preds'].cpu().numpy(), last_vf, dones, GAMMA, LAM)
    assert np.array_equal(_bits(b['advantages']), want_a.view(np.int32))
    assert np.array_equal(_bits(b['value_targets']), want_t.view(np.int32))
    assert np.isfinite(want_a).all()
    return dones


@pytest.mark.parametrize('kind,E,U,B,compact', CASES, ids=IDS)
def test_collect_matches_the_plain_loop(torch_cuda, kind, E, U, B, compact):
    """T = 6 over a horizon of 4: dones = 0 0 0 1 0 0, the batch ends inside the second episode.  Then a second collect into the
    same buffers continues it: its obs[0] is the first batch's new_obs_last, its dones = 0 1 0 0 0 1 (ending ON a boundary)."""
    torch = torch_cuda
    from deepcomp_amd.sampler import collect
    env, twin, actor = _env(kind, E, U, B), _env(kind, E, U, B), _actor(kind, U, B)
    T = 6
    b = collect(env, actor, T, gamma=GAMMA, lam=LAM, compact=compact)
    rows = E * U if kind == 'multi' else E
    assert b['actions'].shape == (T, E, U) and b['actions'].dtype == torch.uint8
    assert b['action_logp'].shape == (T, rows, actor.heads) and b['vf_preds'].shape == (T, rows)
    assert b['rewards'].shape == b['advantages'].shape == b['value_targets'].shape == (T, rows) and b['dones'].shape == (T,)
    assert ('obs_compact' in b) == compact and ('obs' in b) != compact
    dones = _check_batch(torch, env, twin, actor, b, T, compact, started=False)
    assert dones.tolist() == [0, 0, 0, 1, 0, 0]
    env.check(); twin.check()
    assert env.time == twin.time == 2 and env.episode == twin.episode

    first_last = b['new_obs_last'].clone()
    b2 = collect(env, actor, T, gamma=GAMMA, lam=LAM, compact=compact, out=b)
    assert b2 is b
    key = 'obs_compact' if compact else 'obs'
    assert torch.equal(b[key][0].view(torch.int32), first_last.view(torch.int32))
    dones = _check_batch(torch, env, twin, actor, b, T, compact, started=True)
    assert dones.tolist() == [0, 1, 0, 0, 0, 1]
    env.check(); twin.check()
    assert env.time == twin.time == 0


@pytest.mark.parametrize('kind,E,U,B,compact', CASES, ids=IDS)
def test_consecutive_collects_without_out(torch_cuda, kind, E, U, B, compact):
    """collect(env, actor, T) three times with fresh buffers each, a step of the caller's own between the second and the third:
    every batch starts from the env's CURRENT observation (collect leaves new_obs_last in env.obs), so the three batches and the
    step are one trajectory -- the twin's plain loop.  T = 3 over a horizon of 4: the batches start at time 0, 3 and 3."""
    torch = torch_cuda
    from deepcomp_amd.sampler import collect
    env, twin, actor = _env(kind, E, U, B), _env(kind, E, U, B), _actor(kind, U, B)
    T = 3
    b1 = collect(env, actor, T, gamma=GAMMA, lam=LAM, compact=compact)
    assert _check_batch(torch, env, twin, actor, b1, T, compact, started=False).tolist() == [0, 0, 0]
    assert np.array_equal(_bits(env.obs), _bits(twin.obs))
    b2 = collect(env, actor, T, gamma=GAMMA, lam=LAM, compact=compact)
    assert b2 is not b1 and b2['actions'].data_ptr() != b1['actions'].data_ptr()
    assert _check_batch(torch, env, twin, actor, b2, T, compact, started=True).tolist() == [1, 0, 0]
    assert np.array_equal(_bits(env.obs), _bits(twin.obs)) and env.time == twin.time == 2
    a = actor.act(env, sample=True)                    # the caller's own step, on the observation collect left in env.obs
    assert torch.equal(a, actor.act(twin, sample=True))
    env.step(a)
    twin.step(a)
    assert np.array_equal(_bits(env.obs), _bits(twin.obs))
    b3 = collect(env, actor, T, gamma=GAMMA, lam=LAM, compact=compact)
    assert _check_batch(torch, env, twin, actor, b3, T, compact, started=True).tolist() == [1, 0, 0]
    assert np.array_equal(_bits(env.obs), _bits(twin.obs))
    env.check(); twin.check()


@pytest.mark.parametrize('kind,E,U,B,compact', CASES, ids=IDS)
def test_collect_ending_on_the_boundary(torch_cuda, kind, E, U, B, compact):
    """T = 4 = the horizon: dones = 0 0 0 1, no bootstrap (new_obs_last is the next episode's first observation, and its value does
    not enter the advantages: gae_reference gets last_vf = None)."""
    torch = torch_cuda
    from deepcomp_amd.sampler import collect
    env, twin, actor = _env(kind, E, U, B), _env(kind, E, U, B), _actor(kind, U, B)
    started = not compact
    if started:                                        # rows: from a reset the caller made
        env.reset()
        twin.reset()
    b = collect(env, actor, 4, gamma=GAMMA, lam=LAM, compact=compact)
    dones = _check_batch(torch, env, twin, actor, b, 4, compact, started=started)
    assert dones.tolist() == [0, 0, 0, 1]
    env.check(); twin.check()


def test_collect_refuses_what_it_cannot_do(torch_cuda):
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.sampler import collect
    env = _env('multi', 4, 4, 5)
    with pytest.raises(ValueError):
        collect(env, FcnetActor.random('multi', 4, 5, hidden=32), 3)                     # no value function
    actor = FcnetActor('multi', 4, 5, FcnetActor.random_weights('multi', 4, 5, 32), value_weights=FcnetActor.random_value_weights('multi', 4, 5, 32))
    with pytest.raises(ValueError):
        collect(env, actor, 0)
    b = collect(env, actor, 3)
    with pytest.raises(ValueError):
        collect(env, actor, 2, out=b)                                                    # buffers of another length
    with pytest.raises(ValueError):
        collect(env, actor, 3, compact=True, out=b)                                      # buffers of the other format
    dyn = _env('multi', 4, 4, 5, ue_arrival={2: 1})
    dactor = FcnetActor('multi', dyn.U, 5, FcnetActor.random_weights('multi', dyn.U, 5, 32),
                        value_weights=FcnetActor.random_value_weights('multi', dyn.U, 5, 32))
    with pytest.raises(NotImplementedError):
        collect(dyn, dactor, 3)
    env.check()
