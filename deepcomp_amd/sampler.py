"""PPO sample batches collected on the device (include/dcomp.h: dcomp_actor_actions_v, dcomp_gae).

What an RLlib rollout worker does per env and step -- compute_action, env.step, append to a SampleBatch, then
``compute_advantages(use_gae=True)`` over the finished fragment -- for a whole env batch with everything in HBM:

    actor = FcnetActor.from_rllib_weights('multi', U, B, policy.get_weights(), with_value=True)
    batch = collect(env, actor, num_steps=50, gamma=0.99, lam=0.95)
    # batch['obs'] [T, E, U, 4B+1], 'actions' [T, E, U], 'action_logp', 'vf_preds', 'rewards', 'advantages', 'value_targets' [T, rows]

Per step two launches (the actor with its value function, the env step writing straight into the next slot of the buffers), after
the loop one value-only launch for the bootstrap and one for the advantages.  With Philox draws nothing synchronises and nothing is
allocated per step.  The PPO loss and the optimiser read the batch where it lies: deepcomp_amd.learner.PPOLearner.update (which needs
``dist_inputs=True``: the logits the actions were drawn from, for the KL term).

Envs with UE arrival / departure (include/dcomp_gae_uid.h: dcomp_gae_uid): there a column of the batch is a slot, and slots shift when a
UE leaves.  ``collect(..., by_ue=True)`` records env.uid before and after every step (two small copies per step) and the advantages
follow each UE through the slots by its uid word; ``live`` marks the rows that count and the learner trains on exactly those:

    batch = collect(env, actor, num_steps=50, gamma=0.99, lam=0.95, dist_inputs=True, by_ue=True)
    stats = learner.update(batch, rows=live_rows(batch))

gae_reference / gae_uid_reference are the two estimators' specifications in numpy; on a static layout they agree bit for bit.
"""
import ctypes

import numpy as np
import torch

from . import _lib


def gae_reference(reward, vf, last_vf=None, end=None, gamma=0.99, lam=1.0):
    """The specification of dcomp_gae: RLlib's compute_advantages(use_gae=True) as float32 operations, each rounded on its own,
    in this order.  reward, vf: [T, R]; last_vf: [R] or None (= 0); end: [T] (1 = step t was the last of its episode) or None.
    Returns (advantages, value_targets), float32 [T, R]."""
    reward, vf = np.asarray(reward, dtype=np.float32), np.asarray(vf, dtype=np.float32)
    T = reward.shape[0]
    reward, vf = reward.reshape(T, -1), vf.reshape(T, -1)
    g = np.float32(gamma)
    gl = np.float32(g * np.float32(lam))
    nv = np.zeros(reward.shape[1], dtype=np.float32) if last_vf is None else np.asarray(last_vf, dtype=np.float32).reshape(-1).copy()
    A = np.zeros_like(nv)
    adv, target = np.empty_like(reward), np.empty_like(reward)
    with np.errstate(invalid='ignore'):
        for t in range(T - 1, -1, -1):
            if end is not None and end[t]:
                nv, A = np.zeros_like(nv), np.zeros_like(A)
            d = (reward[t] + g * nv) - vf[t]               # float32 arrays: every operation rounds to float32
            A = d + gl * A
            adv[t], target[t] = A, A + vf[t]
            nv = vf[t]
    return adv, target


def _require(t, dtype, numel, what, device):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != device or not t.is_contiguous() or t.numel() != numel:
        raise ValueError(f"{what} must be a contiguous {dtype} tensor with {numel} elements on {device}")


def gae(reward, vf, last_vf=None, end=None, gamma=0.99, lam=1.0, out=None):
    """dcomp_gae on torch tensors: reward, vf float32 [T, ...] on one GPU, last_vf [...] or None, end uint8 [T] or None.
    Returns (advantages, value_targets) of reward's shape; out: a pair of such tensors to write into.  The outputs must not
    overlap the inputs."""
    if not isinstance(reward, torch.Tensor) or reward.dim() < 1 or reward.numel() == 0 or reward.device.type != 'cuda':
        raise ValueError("reward must be a non-empty float32 tensor [T, ...] on the GPU")
    dev, T = reward.device, reward.shape[0]
    R = reward.numel() // T
    _require(reward, torch.float32, T * R, 'reward', dev)
    _require(vf, torch.float32, T * R, 'vf', dev)
    if last_vf is not None:
        _require(last_vf, torch.float32, R, 'last_vf', dev)
    if end is not None:
        _require(end, torch.uint8, T, 'end', dev)
    adv, target = out if out is not None else (torch.empty_like(reward), torch.empty_like(reward))
    _require(adv, torch.float32, T * R, 'advantages', dev)
    _require(target, torch.float32, T * R, 'value_targets', dev)
    L = _lib.load()
    args = _lib.DcompGaeArgs(ctypes.sizeof(_lib.DcompGaeArgs), T, R, float(gamma), float(lam), reward.data_ptr(), vf.data_ptr(),
                             last_vf.data_ptr() if last_vf is not None else None, end.data_ptr() if end is not None else None,
                             adv.data_ptr(), target.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(L.dcomp_gae(ctypes.byref(args), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return adv, target


def gae_uid_reference(reward, vf, uid, uid_next, last_vf=None, end=None, gamma=0.99, lam=1.0):
    """The specification of dcomp_gae_uid (include/dcomp_gae_uid.h): gae_reference per UE, the UE followed through the slots by its
    uid word.  uid, uid_next: [T, E, U] 16-bit words before / after step t (0 = dead slot); reward [T, E, U] in uid_next[t]'s layout,
    vf [T, E, U] in uid[t]'s; last_vf [E, U] in uid_next[T-1]'s, or None (= 0); end [T] or None.  Walks t backwards with the carry
    (nv, A) held per slot of the layout after step t.  Row (t, e, s) counts iff its word is not 0 and stands in uid_next[t, e] at
    some slot s': it takes reward[t, e, s'] and the carry of s', and leaves (vf, A) as its own slot's carry; a row that does not count
    writes zeros and leaves (0, 0).  Every f32 operation is rounded on its own, in gae_reference's order; values of rows that do not
    count are selected away, never multiplied.  Returns (advantages, value_targets, live): float32, float32, uint8 [T, E, U]."""
    uid, uid_next = np.asarray(uid), np.asarray(uid_next)
    T, E, U = uid.shape
    uid, uid_next = uid.astype(np.uint16), uid_next.astype(np.uint16).reshape(T, E, U)      # (int16 words: the same bits)
    reward, vf = np.asarray(reward, dtype=np.float32).reshape(T, E, U), np.asarray(vf, dtype=np.float32).reshape(T, E, U)
    g = np.float32(gamma)
    gl = np.float32(g * np.float32(lam))
    zero = np.zeros((E, U), dtype=np.float32)
    nv = zero.copy() if last_vf is None else np.asarray(last_vf, dtype=np.float32).reshape(E, U).copy()
    A = zero.copy()
    adv, target, live = np.empty_like(reward), np.empty_like(reward), np.empty((T, E, U), dtype=np.uint8)
    with np.errstate(invalid='ignore'):
        for t in range(T - 1, -1, -1):
            if end is not None and end[t]:
                nv, A = zero, zero
            same = (uid[t][:, :, None] == uid_next[t][:, None, :]) & (uid[t][:, :, None] != 0)       # [E, s, s']
            found, sp = same.any(axis=2), same.argmax(axis=2)
            r, nv, A = (np.take_along_axis(x, sp, axis=1) for x in (reward[t], nv, A))
            d = (r + g * nv) - vf[t]                       # float32 arrays: every operation rounds to float32
            a = d + gl * A
            adv[t], target[t], live[t] = np.where(found, a, zero), np.where(found, a + vf[t], zero), found
            nv, A = np.where(found, vf[t], zero), adv[t]
    return adv, target, live


def gae_uid(reward, vf, uid, uid_next, last_vf=None, end=None, gamma=0.99, lam=1.0, max_shift=None, out=None):
    """dcomp_gae_uid on torch tensors: uid, uid_next int16 [T, E, U] on one GPU, reward, vf float32 with T E U elements, last_vf
    float32 with E U elements or None, end uint8 [T] or None.  max_shift: the largest number of departures in one step (None:
    unknown, every search runs over the whole prefix).  Returns (advantages, value_targets, live): float32 of reward's shape twice
    and uint8 of reward's shape; out: a triple of such tensors to write into.  The outputs must not overlap the inputs."""
    if not isinstance(uid, torch.Tensor) or uid.dim() != 3 or uid.numel() == 0 or uid.device.type != 'cuda':
        raise ValueError("uid must be a non-empty int16 tensor [T, E, U] on the GPU")
    dev, (T, E, U) = uid.device, uid.shape
    n = T * E * U
    _require(uid, torch.int16, n, 'uid', dev)
    _require(uid_next, torch.int16, n, 'uid_next', dev)
    _require(reward, torch.float32, n, 'reward', dev)
    _require(vf, torch.float32, n, 'vf', dev)
    if last_vf is not None:
        _require(last_vf, torch.float32, E * U, 'last_vf', dev)
    if end is not None:
        _require(end, torch.uint8, T, 'end', dev)
    adv, target, live = out if out is not None else (torch.empty_like(reward), torch.empty_like(reward), torch.empty_like(reward, dtype=torch.uint8))
    _require(adv, torch.float32, n, 'advantages', dev)
    _require(target, torch.float32, n, 'value_targets', dev)
    _require(live, torch.uint8, n, 'live', dev)
    L = _lib.load()
    args = _lib.DcompGaeUidArgs(ctypes.sizeof(_lib.DcompGaeUidArgs), T, E, U, -1 if max_shift is None else int(max_shift), float(gamma), float(lam),
                                reward.data_ptr(), vf.data_ptr(), uid.data_ptr(), uid_next.data_ptr(),
                                last_vf.data_ptr() if last_vf is not None else None, end.data_ptr() if end is not None else None,
                                adv.data_ptr(), target.data_ptr(), live.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(L.dcomp_gae_uid(ctypes.byref(args), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return adv, target, live


def live_rows(batch):
    """The rows of a collect(..., by_ue=True) batch that count, as PPOLearner.update(batch, rows=live_rows(batch)) takes them: the int64
    device tensor of the source rows t E U + e U + s with live = 1, ascending.  One synchronisation (the count of the rows is read)."""
    return torch.nonzero(batch['live'].reshape(-1)).reshape(-1)


_CODECS = {}


def _codec(env):
    """The compact record's codec for this env's shape and device (its flag word is allocated once)."""
    from .fragment import FragmentCodec
    key = (env.U, env.B, env.device)
    if key not in _CODECS:
        _CODECS[key] = FragmentCodec(env.U, env.B, env.device)
    return _CODECS[key]


def buffers(env, actor, num_steps, compact=False, dist_inputs=False, by_ue=False):
    """The device buffers of a num_steps batch, allocated once.  by_ue=True adds uid and uid_next (int16 [T, E, U]) and live (uint8
    [T, rows])."""
    T, E, U, dev = int(num_steps), env.E, env.U, env.device
    rows = E * U if env.kind == _lib.MULTI else E
    b = {}
    if compact:
        b['obs_compact'] = torch.zeros((T, E, env.compact_words), dtype=torch.int32, device=dev)
        b['new_obs_last'] = torch.zeros((E, env.compact_words), dtype=torch.int32, device=dev)
    else:
        b['obs'] = torch.zeros((T,) + tuple(env.obs.shape), dtype=torch.float32, device=dev)
        b['new_obs_last'] = torch.zeros_like(env.obs)
    b['actions'] = torch.zeros((T, E, U), dtype=torch.uint8, device=dev)
    b['action_logp'] = torch.zeros((T, rows, actor.heads), dtype=torch.float32, device=dev)
    if dist_inputs:
        b['action_dist_inputs'] = torch.zeros((T, rows, actor.num_logits), dtype=torch.float32, device=dev)
    for name in ('vf_preds', 'rewards', 'advantages', 'value_targets'):
        b[name] = torch.zeros((T, rows), dtype=torch.float32, device=dev)
    b['dones'] = torch.zeros(T, dtype=torch.uint8, device=dev)
    b['last_vf'] = torch.zeros(rows, dtype=torch.float32, device=dev)
    if by_ue:
        b['uid'] = torch.zeros((T, E, U), dtype=torch.int16, device=dev)
        b['uid_next'] = torch.zeros((T, E, U), dtype=torch.int16, device=dev)
        b['live'] = torch.zeros((T, rows), dtype=torch.uint8, device=dev)
    return b


def collect(env, actor, num_steps, gamma=0.99, lam=1.0, sample=True, compact=False, out=None, dist_inputs=False, by_ue=False):
    """num_steps steps of `env` driven by `actor` (which needs a value function) as one PPO train batch: a dict of device tensors
    under RLlib's SampleBatch names -- obs [T, ...] (compact=True: obs_compact [T, E, words], the record of env.step_compact),
    actions [T, E, U] uint8, action_logp [T, rows, heads], vf_preds / rewards / advantages / value_targets [T, rows], dones [T]
    uint8 (the env batch runs in lock-step) and new_obs_last, the observation after step T-1 (last_vf [rows] holds its value, the
    bootstrap, where the batch ended inside an episode).  dist_inputs=True adds action_dist_inputs [T, rows, logits], the logits the
    actions were drawn from (what PPO's KL term needs).

    The batch starts from env.obs -- the observation of the caller's reset() / step(), or of the previous collect() -- and from a
    reset of its own where the env has never been reset; it leaves new_obs_last in env.obs, so batches follow each other (and the
    caller's own steps) without a gap, with or without `out`.  When env.time reaches env.episode_length, dones[t] = 1 and the env
    is reset into the next slot, as RLlib does at its horizon (env_setup.py:281).  A batch that ends inside an episode bootstraps
    from the value of new_obs_last.  Draws are keyed as in FcnetActor.act.  out: the dict of an earlier call with the same
    num_steps and format, to reuse its buffers.  compact=True packs env.obs into the first slot and unpacks new_obs_last into
    env.obs (one launch each per batch; pack(rows) is the record the step writes, word for word).

    by_ue=True (multi-agent envs) is the collector for envs with UE arrival / departure, where slots shift when a UE leaves and a
    column is not one UE's trajectory.  The batch gets three more keys: uid and uid_next (int16 [T, E, U]), env.uid before step t and
    after it (before a reset at the horizon) -- obs[t], actions[t], vf_preds[t], action_logp[t] stand in uid[t]'s layout, rewards[t]
    and the next observation in uid_next[t]'s -- and live (uint8 [T, rows]).  advantages and value_targets then follow each UE
    through the slots by its uid word (gae_uid, include/dcomp_gae_uid.h): row (t, e, s) counts, live = 1, iff its UE acted in step
    t and was still listed after it, at slot s'; it takes rewards[t, e, s'] and continues in row (t + 1, e, s').  A UE's trajectory
    ends, with next value 0, at the horizon and where it departs in the next step; at the batch end inside an episode it bootstraps
    from last_vf[e, s'].  The row of the step in which a UE departs does not count, and neither does the reward an arriving UE gets
    before its first action; rows that do not count hold advantages = value_targets = 0.  Train on the counted rows:
    PPOLearner.update(batch, rows=live_rows(batch)).  On a static env uid and uid_next hold 1 ... U and the batch is the plain
    collector's, bit for bit, with live all ones.  Not with central envs (a row is an env there, and the learner's num_active is one
    number per batch) and not with per-UE policy sets keyed by slot (their learner picks rows by slot, and a slot is not one UE here).  A
    set keyed by UE id (deepcomp_amd.policy_set.PerIdActor, which needs by_ue=True and one member per id up to env.max_id) is the
    per-UE set of such envs: every row goes through the policy of the id in its uid word, the bootstrap too, with the words after the
    last step; PerIdLearner.update trains each policy on its UE's counted rows."""
    T = int(num_steps)
    if T < 1:
        raise ValueError("num_steps must be >= 1")
    if env.dynamic and not by_ue:
        raise NotImplementedError("envs with UE arrival / departure: slots shift on departure, a column is not one UE's trajectory; "
                                  "by_ue=True follows each UE through the slots (multi-agent envs)")
    from .policy_set import PerIdActor, PerUEActor
    by_id = isinstance(actor, PerIdActor)
    if by_ue:
        if env.kind != _lib.MULTI:
            raise NotImplementedError("by_ue=True with a central env: its rows are envs, not UEs, and the learner takes one num_active per batch "
                                      "while the number of listed UEs changes from step to step")
        if isinstance(actor, PerUEActor):
            raise NotImplementedError("by_ue=True with a per-UE policy set: its policies belong to slots, and a slot is not one UE where the list shifts")
    if env.kind != actor.kind or env.U != actor.U or env.B != actor.B:
        raise ValueError("the env's kind / UE slots / stations differ from the actor's")
    if by_id:
        if not by_ue:
            raise ValueError("a policy set keyed by UE id needs by_ue=True: its learner picks every policy's rows by the recorded uid words")
        actor.check_env(env)
    if actor.value_weights is None:
        raise ValueError("the actor has no value function (set_value)")
    if compact and env.kind != _lib.MULTI:
        raise NotImplementedError("compact observation records exist for multi-agent observations only")
    key = 'obs_compact' if compact else 'obs'
    b = out if out is not None else buffers(env, actor, T, compact, dist_inputs, by_ue)
    if not isinstance(b, dict) or key not in b or b[key].shape[0] != T or b['actions'].shape != (T, env.E, env.U) or \
            (dist_inputs and 'action_dist_inputs' not in b) or (by_ue and 'live' not in b):
        raise ValueError(f"out must be the dict of a collect() call with the same env shape, num_steps, compact={compact}, dist_inputs and by_ue")
    obs, last = b[key], b['new_obs_last']
    reset_into = env.reset_compact if compact else env.reset_into

    if env.episode < 0:
        env.reset()
    if compact:
        _codec(env).pack(env.obs, out=obs[0])
    else:
        obs[0].copy_(env.obs)

    words = env.uid.view(env.E, env.U) if by_ue and env.uid is not None else None
    if by_ue and words is None:                        # a static env: slot s is UE s + 1 throughout
        b['uid'].copy_(torch.arange(1, env.U + 1, dtype=torch.int16, device=env.device).expand(T, env.E, env.U))
        b['uid_next'].copy_(b['uid'])
    b['dones'].zero_()
    done = False
    for t in range(T):
        if words is not None:
            b['uid'][t].copy_(words)
        actor.act(env, sample=sample, obs=obs[t], compact=compact, out=b['actions'][t], logp=b['action_logp'][t], vf=b['vf_preds'][t],
                  logits=b['action_dist_inputs'][t] if dist_inputs else None)
        nxt = obs[t + 1] if t + 1 < T else last
        if compact:
            env.step_compact(b['actions'][t], nxt, b['rewards'][t])
        else:
            env.step_into(b['actions'][t], nxt, b['rewards'][t])
        if words is not None:                          # after the step's events, before a reset changes the layout once more
            b['uid_next'][t].copy_(words)
        done = env.time >= env.episode_length
        if done:                                     # the horizon: what the step wrote is discarded, the new episode's first observation takes its place
            b['dones'][t].fill_(1)
            reset_into(nxt)
    if not done and by_id:                             # the words after the last step: the layout `last` stands in
        actor.value(last, uid=actor.uid_of(env), compact=compact, out=b['last_vf'])
    elif not done:
        actor.value(last, compact=compact, out=b['last_vf'])
    if by_ue:
        gae_uid(b['rewards'], b['vf_preds'], b['uid'], b['uid_next'], None if done else b['last_vf'], b['dones'], gamma, lam,
                max_shift=max(r for r, _ in env.schedule) if env.dynamic else 0, out=(b['advantages'], b['value_targets'], b['live']))
    else:
        gae(b['rewards'], b['vf_preds'], None if done else b['last_vf'], b['dones'], gamma, lam, out=(b['advantages'], b['value_targets']))
    if compact:                                        # env.obs is the current observation again: the next batch, or the caller, goes on from it
        _codec(env).unpack(last, out=env.obs)
    else:
        env.obs.copy_(last)
    return b
