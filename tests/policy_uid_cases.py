"""What the tests of the policy set keyed by UE id share (tests/test_policy_uid_cpu.py, tests/test_policy_uid_gpu.py;
include/dcomp_policy_set_uid.h, deepcomp_amd.policy_set.PerIdActor / PerIdLearner / policy_rows_by_id): the shapes, the hand-written
traces of the row split with its device-free checks, and the builders and comparisons the GPU tests run more than once.  A support
module, not a test: nothing at import time touches a GPU, and it imports no test module."""
import numpy as np

from tests import gae_uid_cases as gc

B = 5
HORIZON, UE_ARRIVAL, SCHEDULE = gc.HORIZON, gc.UE_ARRIVAL, gc.SCHEDULE      # 5 5 7 6 4 4 UEs listed over an episode; ids up to U0 + 3
STEPS = 9                                                                    # one horizon and three steps of the next episode
# (initial UEs, envs, hidden, activation, compact): one full env group and a partial one at MT 1 and 2; an env wider than a wavefront,
# uid rows longer than one pass of the lanes; the widest instantiation once
DYN_CASES = [(5, 40, 32, 'tanh', False), (5, 40, 64, 'relu', True), (66, 4, 32, 'relu', True), (66, 4, 64, 'tanh', False), (5, 4, 256, 'tanh', False)]
DYN_IDS = ['u5-e40-h32-rows', 'u5-e40-h64-compact', 'u66-e4-h32-compact', 'u66-e4-h64-rows', 'u5-e4-h256-rows']
NAN_BITS = 0x7FC00000


# ------------------------------------------------------------------------------------------------ the row split: hand-written traces
def trace_a():
    """T = 6, E = 2, U = 7, five initial UEs, gae_uid_cases.SCHEDULE with every departure chosen by hand.
    env 0: [1 2 3 4 5] -> +6' 7' -> 7' leaves -> 6' and 5 leave (two departures in one step) -> [1 2 3 4] -> 5' arrives: an arrival
    whose id equals a departed UE's.  env 1: 1 leaves, then 3 and 4: [2 5 6' 7'] -> 8' arrives.  Slots behind the list are dead
    throughout; the rows of the steps in which a UE departs do not count."""
    pops = {(2, 0, 0): 6, (3, 0, 0): 5, (3, 0, 1): 4, (2, 1, 0): 0, (3, 1, 0): 1, (3, 1, 1): 1}
    uid, uid_next, end = gc.make_trace(6, 2, 7, 5, SCHEDULE, 6, seed=0, force=lambda t, e, k, n: pops[(t, e, k)])
    Bn = gc.BORN
    assert uid[5].tolist() == [[1, 2, 3, 4, 0, 0, 0], [2, 5, 6 | Bn, 7 | Bn, 0, 0, 0]]
    assert uid_next[5].tolist() == [[1, 2, 3, 4, 5 | Bn, 0, 0], [2, 5, 6 | Bn, 7 | Bn, 8 | Bn, 0, 0]]
    assert uid[3, 0].tolist() == [1, 2, 3, 4, 5, 6 | Bn, 0] and uid_next[3, 0].tolist() == [1, 2, 3, 4, 0, 0, 0]
    return uid, uid_next, end


def trace_b():
    """T = 9 over the horizon of 6, E = 3, random departures: the list is reset inside the batch, and the batch ends inside an episode."""
    return gc.make_trace(9, 3, 7, 5, SCHEDULE, 6, seed=4)


TRACES = {'a': (trace_a, 9), 'b': (trace_b, 8)}          # name -> (trace, policies): (a) has a policy that never appears, id 9


def trajectory_rows(uid, uid_next, end, num_policies):
    """The rows gae_uid_cases.by_trajectory's trajectories give to each id: with a UE's id as its value, no reward and gamma = 0 a
    counted row's advantage is -id and every other row's 0.  Returns (per policy the ascending source rows, the live rows)."""
    ids = (uid & 0x7FFF).astype(np.float32)
    adv, _, live = gc.by_trajectory(np.zeros_like(ids), ids, uid, uid_next, None, end, 0.0, 1.0)
    assert np.array_equal(adv != 0, live != 0)
    flat = adv.reshape(-1)
    return [np.nonzero(flat == -float(p + 1))[0].astype(np.int64) for p in range(num_policies)], np.nonzero(live.reshape(-1))[0].astype(np.int64)


def check_split(rows, uid, uid_next, end, num_policies):
    """The three checks of a row split: disjoint and ascending; together the live rows; per policy the trajectories' rows."""
    rows = [np.asarray(r) for r in rows]
    want, live = trajectory_rows(uid, uid_next, end, num_policies)
    assert len(rows) == num_policies
    for r in rows:
        assert r.dtype == np.int64 and (np.diff(r) > 0).all()
    every = np.concatenate(rows)
    assert np.unique(every).size == every.size and np.array_equal(np.sort(every), live)
    for p in range(num_policies):
        assert np.array_equal(rows[p], want[p]), p
    return want


# ------------------------------------------------------------------------------------------------ GPU builders
def dyn_env(E, U0, ue_arrival=UE_ARRIVAL, rng='philox'):
    from deepcomp_amd import scenarios
    from deepcomp_amd.entities import build_from_scenario
    from deepcomp_amd.env import BatchedMobileEnv
    m, bs, ues = build_from_scenario(scenarios.grid_map(B, 'mixed').with_ues(num_slow=U0))
    return BatchedMobileEnv(m, bs, ues, 'multi', num_envs=E, seed=42, episode_length=HORIZON, rng=rng, rand_episodes=True, ue_arrival=ue_arrival)


def member(U, H, act, seed, value=True, shared=False, kind='multi'):
    from deepcomp_amd.actor import FcnetActor
    w = FcnetActor.random_weights(kind, U, B, H, seed=seed, bias_std=0.1)
    vw = FcnetActor.random_value_weights(kind, U, B, H, seed=seed, bias_std=0.1, shared=shared) if value else None
    return FcnetActor(kind, U, B, w, activation=act, value_weights=vw)


def members(U, H, act, P, seed=10, same=False):
    return [member(U, H, act, seed if same else seed + p) for p in range(P)]


def fresh(torch, E, actor, mode, carve=None):
    """The output tensors of one launch, floats NaN and actions 0xEE (carve(numel, dtype): from guarded storage instead, in its fill)."""
    rows = E * actor.U
    def buf(n, dtype):
        if carve is not None:
            return carve(n, dtype)
        return torch.full((n,), 0xEE if dtype == torch.uint8 else float('nan'), dtype=dtype, device='cuda')
    out = {}
    if mode != 'v':
        out['act'], out['logits'], out['logp'] = buf(rows, torch.uint8), buf(rows * actor.num_logits, torch.float32), buf(rows * actor.heads, torch.float32)
    if mode != 'a':
        out['vf'] = buf(rows, torch.float32)
    return out


def launch(torch, actor, obs, compact, mode, uid=None, out=None, **kw):
    """One launch into `out` (fresh() by default): mode 'a' = actions, 'av' = with the value, 'v' = the value alone.  uid: the words of
    an id-keyed set's launch."""
    E = obs.shape[0]
    out = fresh(torch, E, actor, mode) if out is None else out
    by_id = {} if uid is None else {'uid': uid}
    if mode == 'v':
        actor.value(obs, compact=compact, out=out['vf'], **by_id)
    else:
        actor.actions(obs, compact=compact, out=out['act'].view(E, actor.U), logits=out['logits'], logp=out['logp'], vf=out.get('vf'), **by_id, **kw)
    torch.cuda.synchronize()
    return out


def same(torch, got, want, rows=None):
    """Every output of two launches equal bit for bit (rows: at these decision rows); NaN, the initial fill, equals nothing."""
    assert got.keys() == want.keys()
    n = (got.get('vf') if 'vf' in got else got['act']).numel()
    for k in got:
        a, b = got[k].reshape(n, -1), want[k].reshape(n, -1)
        if rows is not None:
            a, b = a[rows], b[rows]
        assert torch.equal(a, b), k


def all_zero(torch, out, rows):
    n = (out.get('vf') if 'vf' in out else out['act']).numel()
    for k, t in out.items():
        assert not bool(t.reshape(n, -1)[rows].view(torch.uint8).any()), f'{k}: a row without a policy is not zero'


def ids_of(torch, uid):
    return (uid.reshape(-1).to(torch.int32) & 0x7FFF)


def poison_dead(torch, obs, uid, compact, U):
    """A copy of the observations with NaN in every row (compact: every per-UE record) of a slot whose word is 0."""
    dead = uid.reshape(-1) == 0
    bad = obs.clone()
    if compact:
        words = bad.view(bad.shape[0], -1)
        ue = words[:, :U * (B + 2)].reshape(-1, B + 2)
        ue[dead] = NAN_BITS
        words[:, :U * (B + 2)] = ue.view(bad.shape[0], -1)
    else:
        bad.view(dead.numel(), -1)[dead] = float('nan')
    assert int(dead.sum()) == 0 or not torch.equal(bad.view(torch.uint8), obs.view(torch.uint8))
    return bad


# ------------------------------------------------------------------------------------------------ the collector's twin
def twin_loop(torch, env, actor, T, started):
    """The plain act + step loop with a reset at the horizon; per step what the collector must have recorded."""
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


def check_batch(torch, env, twin, actor, b, T, compact, started):
    """collect(by_ue=True)'s batch against the twin's loop, and its advantages against gae_uid_reference and the cut-out trajectories of
    the recorded columns (the structure of tests/test_sampler_dyn_gpu.py's check, for an actor whose value call takes uid words)."""
    from deepcomp_amd.fragment import FragmentCodec
    from deepcomp_amd.sampler import gae_uid_reference
    E, U = env.E, env.U
    bits = lambda t: t.contiguous().view(torch.int32)      # noqa: E731
    rec, last_obs = twin_loop(torch, twin, actor, T, started)
    codec = FragmentCodec(U, B) if compact else None
    rows_of = (lambda p: codec.unpack(p.contiguous())) if compact else (lambda o: o)
    dones = b['dones'].cpu().numpy()
    for t, (obs, uid, a, vf, rew, uid_next, done) in enumerate(rec):
        assert torch.equal(bits(rows_of(b['obs_compact'][t] if compact else b['obs'][t])), bits(obs)), f'obs differ at t = {t}'
        assert torch.equal(b['actions'][t], a), f'actions differ at t = {t}'
        assert torch.equal(bits(b['rewards'][t]), bits(rew.reshape(-1))), f'rewards differ at t = {t}'
        assert torch.equal(bits(b['vf_preds'][t]), bits(vf)), f'vf_preds differ at t = {t}'
        assert torch.equal(b['uid'][t].reshape(-1), uid.reshape(-1)) and torch.equal(b['uid_next'][t].reshape(-1), uid_next.reshape(-1)), t
        assert int(dones[t]) == int(done), t
    assert torch.equal(bits(rows_of(b['new_obs_last'])), bits(last_obs)), 'new_obs_last differs'
    last_vf = None if dones[T - 1] else actor.value(b['new_obs_last'], uid=actor.uid_of(twin), compact=compact).cpu().numpy()
    cols = [b[k].cpu().numpy() for k in ('rewards', 'vf_preds', 'uid', 'uid_next')]
    got = [b[k].cpu().numpy().reshape(T, E, U) for k in ('advantages', 'value_targets', 'live')]
    for fn in (gae_uid_reference, gc.by_trajectory):
        want = fn(*cols, last_vf, dones, gc.GAMMA, gc.LAM)
        for g, w, name in zip(got, want, ('advantages', 'value_targets', 'live')):
            assert np.array_equal(gc.bits(g), gc.bits(w)), f'{name} differ from {fn.__name__}'
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    return dones, got[2]
