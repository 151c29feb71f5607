#!/usr/bin/env python3
"""Policy-in-the-loop sampling rate on one GPU: the batched env feeding a shared-parameter actor (RLlib's default fcnet,
2 x 256 tanh, parameter sharing across UEs as in DD-CoMP, env_setup.py:266-283) that turns the observation tensor into the
next action tensor -- everything stays in HBM, no per-env Python.  The policy is random-init and NOT part of the product;
this only shows where the time goes once the env runs at ~10^8-10^9 env-steps/s.

    python tools/closed_loop.py [--envs 65536] [--steps 200] [--dtype bf16] [--kind multi] [--actor hip [--compact]]
    python tools/closed_loop.py --collect 50 [--envs 65536] [--kind multi] [--compact] [--shared-value]
    python tools/closed_loop.py --train 3 [--train-steps 5] [--sgd-iters 2] [--minibatch ROWS] [--envs 65536] [--kind multi] [--compact]
                                [--micro-rows ROWS] [--grad-clip NORM]
    python tools/closed_loop.py --collect 50 | --train 3  --ue-arrival 10:4,30:-2,60:-3 [--envs 8192 --ues 12] [--compact]
    python tools/closed_loop.py --per-ue [--actor hip | --collect 50 | --train 3 [--grouped]] [--hidden 64] [--compact] [--envs 4096 --ues 128 --bs 32]

--actor torch (default): the actor as torch ops (bf16 matmuls, Gumbel-max through torch.rand).  --actor hip: the same weights in
deepcomp_amd.actor.FcnetActor -- one HIP kernel from observation tensor to action tensor -- and BOTH loops are timed in this
process, one after the other on the same env.  --compact (multi-agent, hip): the env writes only the compact record
(env.step_compact) and the actor reads it.

--collect T: PPO sample batches of T steps instead -- deepcomp_amd.sampler.collect (actor + value function in one launch per step,
the bootstrap value, dcomp_gae) against the same loop with the HIP actor but the value network as torch ops (bf16 matmuls) and GAE
as a torch loop over t: what a user had before the value function moved into the kernel.  Both are timed in this process,
interleaved, --steps / T batches each.

--train ITERS: the whole PPO loop in this process -- sampler.collect(dist_inputs=True) then deepcomp_amd.learner.PPOLearner.update --
printing the mean reward and the five loss statistics per iteration; then the time of grads + apply per minibatch (HIP events over
back-to-back launches) next to the same network and loss under torch autograd with bf16 autocast and torch.optim.Adam, interleaved;
and the time of one SGD iteration of update on the rows batch (minibatches gathered with index_select, then grads) next to the same
iteration with the minibatches picked through a row index instead (grads_indexed: nothing is copied, rows are read scattered).
--compact (multi-agent): collect returns the compact record and update trains on it through the row index -- no observation row is
written anywhere in the loop; the unpack a rows-only learner would need first is timed on its own.
--grad-clip NORM: update(grad_clip=NORM), RLlib's global-norm clip.  --micro-rows ROWS (a multiple of 2 048): the learner's handle is
sized by ROWS instead of the minibatch and update(micro_rows=ROWS) accumulates a minibatch's gradient micro-batch by micro-batch; the
time of one SGD iteration that way is printed and the comparisons that need a whole-minibatch handle are left out.

--ue-arrival STEP:N,... (multi-agent, with --collect or --train): the env gets the reference's ue_arrival schedule -- N UEs arrive
(N > 0) or depart (N < 0) in step STEP of every episode -- and has max_ues slots; collect runs with by_ue=True (advantages follow each UE
through the slots by its uid word, include/dcomp_gae_uid.h) and update trains on rows=live_rows(batch).  --collect then times
collect(by_ue=True) per step against the bare act + step_into loop on the same env (the torch GAE loop knows no shifting slots);
--train prints the loop's statistics and the share of rows that count, and stops there.

--per-ue --ue-arrival STEP:N,...: the per-UE set of an env with arrival and departure is keyed by UE ID (deepcomp_amd.policy_set.PerIdActor,
one random-init member per id the schedule ever lists): --train N (default 3) iterations of collect(by_ue=True) -> PerIdLearner.update
(--grouped: in grouped launch rounds), with the rows that count, the policies that had rows and the two phases' wall times.

--per-ue (multi-agent): one policy network per UE (D3-CoMP) -- deepcomp_amd.policy_set.PerUEActor over U random-init members and, with
--train, PerUELearner -- timed next to the shared-policy actor / learner on the same env, interleaved: the loop env step + actor
(--actor hip), sampler.collect (--collect T), or collect + update with the time of one SGD iteration (--train ITERS; --minibatch is
per policy there; --grouped adds PerUELearner.update(grouped=True), all policies in one launch round per minibatch round, as a third
interleaved variant and prints medians and ranges).
"""
import argparse
import sys
import time

sys.path.insert(0, '.')
import torch

from deepcomp_amd import scenarios
from deepcomp_amd.entities import build_from_scenario
from deepcomp_amd.actor import FcnetActor
from deepcomp_amd.env import BatchedMobileEnv

ap = argparse.ArgumentParser()
ap.add_argument('--envs', type=int, default=65536)
ap.add_argument('--ues', type=int, default=32)
ap.add_argument('--bs', type=int, default=10)
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
ap.add_argument('--kind', default='multi', choices=['multi', 'central'])
ap.add_argument('--actor', default='torch', choices=['torch', 'hip'])
ap.add_argument('--compact', action='store_true', help='hip actor, multi-agent: the env writes only the compact record and the actor reads it')
ap.add_argument('--collect', type=int, default=0, metavar='T', help='time sampler.collect of T-step batches against the torch-value + torch-GAE loop')
ap.add_argument('--shared-value', action='store_true', help='--collect: value_out on the actor\'s second hidden layer (vf_share_layers)')
ap.add_argument('--train', type=int, default=0, metavar='ITERS', help='collect -> PPOLearner.update, ITERS times, then time grads + apply against torch autograd')
ap.add_argument('--train-steps', type=int, default=5, help='--train: steps per collected batch')
ap.add_argument('--sgd-iters', type=int, default=2, help='--train: SGD iterations per batch')
ap.add_argument('--minibatch', type=int, default=0, help='--train: rows per minibatch (default: one step\'s rows)')
ap.add_argument('--micro-rows', type=int, default=0, help='--train: rows per micro-batch (a multiple of 2048): the handle is sized by it, a minibatch is accumulated')
ap.add_argument('--grad-clip', type=float, default=0.0, help='--train: global-norm gradient clip (RLlib grad_clip); 0: none')
ap.add_argument('--hidden', type=int, default=256, help='hidden width of the fcnet (two layers)')
ap.add_argument('--grouped', action='store_true', help='--per-ue --train: also time PerUELearner.update(grouped=True), interleaved with the sequential update and the shared learner')
ap.add_argument('--ue-arrival', default='', metavar='STEP:N,...', help='--collect / --train, multi-agent: UEs arrive (N > 0) / depart (N < 0) in step STEP of every episode; collect(by_ue=True), update(rows=live_rows(batch))')
ap.add_argument('--per-ue', action='store_true', help='one policy per UE (PerUEActor / PerUELearner) next to the shared policy; multi-agent')
a = ap.parse_args()
if a.per_ue and a.kind != 'multi':
    ap.error('--per-ue needs --kind multi')
if a.collect or a.train or a.per_ue:
    a.actor = 'hip'
arrival = {int(k): int(v) for k, v in (kv.split(':') for kv in a.ue_arrival.split(','))} if a.ue_arrival else None
if arrival and (a.kind != 'multi' or not (a.collect or a.train or a.per_ue)):
    ap.error('--ue-arrival needs --kind multi and --collect, --train or --per-ue')
if a.compact and (a.actor != 'hip' or a.kind != 'multi'):
    ap.error('--compact needs --actor hip and --kind multi')

dev = torch.device('cuda', 0)
E, U, B = a.envs, a.ues, a.bs
scn = scenarios.grid_map(B, 'mixed').with_ues(num_slow=U)
m, bs, ues = build_from_scenario(scn)
multi = a.kind == 'multi'
env = BatchedMobileEnv(m, bs, ues, a.kind, num_envs=E, seed=42, episode_length=100, rng='philox', rand_episodes=True, device=dev, ue_arrival=arrival)
U = env.U                                          # (UE slots: max_ues with --ue-arrival)
dt = torch.bfloat16 if a.dtype == 'bf16' else torch.float32
D = 4 * B + 1 if multi else U * (2 * B + 1)
heads = 1 if multi else U
host_w = FcnetActor.random_weights(a.kind, U, B, a.hidden, seed=0)           # N(0, 1 / fan_in) kernels, zero biases
W1, W2, W3 = (torch.from_numpy(host_w[n]).to(dev).to(dt) for n in ('w1', 'w2', 'w3'))


def policy(obs):                                   # obs [E, U, 4B+1] / [E, U(2B+1)] f32 in HBM -> uint8 actions [E, U]
    x = obs.view(-1, D).to(dt)
    h = torch.tanh(torch.tanh(x @ W1) @ W2)
    logits = (h @ W3).float().view(-1, heads, B + 1)
    gumbel = -torch.log(-torch.log(torch.rand_like(logits).clamp_(1e-20, 1.0)))
    return (logits + gumbel).argmax(dim=-1).to(torch.uint8).view(E, U)


hip = FcnetActor(a.kind, U, B, host_w, device=dev) if a.actor == 'hip' else None


def collect_mode(T):
    from deepcomp_amd.sampler import collect
    gamma, lam = 0.99, 0.95
    host_v = FcnetActor.random_value_weights(a.kind, U, B, a.hidden, seed=0, shared=a.shared_value)
    hip.set_value(host_v, shared=a.shared_value)
    if arrival:
        return collect_dynamic(T, gamma, lam)
    trunk = host_v if not a.shared_value else host_w
    V1, V2 = (torch.from_numpy(trunk[n]).to(dev).to(dt) for n in ('w1', 'w2'))
    Vo = torch.from_numpy(host_v['wv']).to(dev).to(dt).view(-1, 1)
    rows = E * U if multi else E
    obs_t = torch.zeros((T + 1,) + tuple(env.obs.shape), device=dev)
    act_t = torch.zeros((T, E, U), dtype=torch.uint8, device=dev)
    logp_t = torch.zeros((T, rows, heads), device=dev)
    vf_t, rew_t = torch.zeros((T + 1, rows), device=dev), torch.zeros((T, rows), device=dev)
    adv_t, tgt_t = torch.zeros((T, rows), device=dev), torch.zeros((T, rows), device=dev)

    def value(o):
        return (torch.tanh(torch.tanh(o.view(-1, D).to(dt) @ V1) @ V2) @ Vo).float().view(-1)

    def torch_batch():
        """The same batch with the HIP actor (actions + logp), the value network and GAE as torch ops; rows only."""
        obs_t[0].copy_(env.obs)
        ends = []
        for t in range(T):
            hip.act(env, obs=obs_t[t], out=act_t[t], logp=logp_t[t])
            vf_t[t] = value(obs_t[t])
            env.step_into(act_t[t], obs_t[t + 1], rew_t[t])
            ends.append(env.time >= env.episode_length)
            if ends[-1]:
                env.reset_into(obs_t[t + 1])
        vf_t[T] = value(obs_t[T])
        nv, A = (torch.zeros_like(vf_t[T]) if ends[-1] else vf_t[T]), torch.zeros_like(vf_t[T])
        for t in range(T - 1, -1, -1):
            if ends[t]:
                nv, A = torch.zeros_like(nv), torch.zeros_like(A)
            A = rew_t[t] + gamma * nv - vf_t[t] + gamma * lam * A
            adv_t[t], tgt_t[t] = A, A + vf_t[t]
            nv = vf_t[t]
        env.obs.copy_(obs_t[T])

    state = {'buf': None}

    def hip_batch():
        state['buf'] = collect(env, hip, T, gamma, lam, compact=a.compact, out=state['buf'])

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (n * T)

    n = max(1, a.steps // T)
    env.reset()
    torch_batch()
    hip_batch()
    res = {'torch': [], 'hip': []}
    for _ in range(3):                                  # interleaved: drift of the clocks shows as spread, not as a difference
        env.reset()
        res['torch'].append(timed(torch_batch, n))
        env.reset()
        res['hip'].append(timed(hip_batch, n))
    form = 'shared value_out' if a.shared_value else 'value trunk of its own'
    print(f'{E} envs x {U} UE x {B} BS ({a.kind}), actor 2x{a.hidden} tanh + {form}, batches of T = {T}, {n} batches per timing')
    for k, name in (('torch', f'hip actor + torch value ({a.dtype}) + torch GAE'), ('hip', 'sampler.collect' + (' (compact record)' if a.compact else ''))):
        ts = res[k]
        print(f'{name:<46}: ' + ' / '.join(f'{t * 1e3:.3f}' for t in ts) + f' ms/step  (best {E / min(ts):.3e} env-steps/s)')
    print(f'collect vs torch value + torch GAE: {min(res["torch"]) / min(res["hip"]):.2f} x')
    env.check()


def collect_dynamic(T, gamma, lam):
    """--collect T --ue-arrival: collect(by_ue=True) per step against the bare act + step_into loop (rows) on the same env."""
    from deepcomp_amd.sampler import buffers, collect
    state = {'buf': None}
    bare = buffers(env, hip, T, False)

    def hip_batch():
        state['buf'] = collect(env, hip, T, gamma, lam, compact=a.compact, out=state['buf'], by_ue=True)

    def bare_loop():
        obs, last = bare['obs'], bare['new_obs_last']
        obs[0].copy_(env.obs)
        for t in range(T):
            hip.act(env, obs=obs[t], out=bare['actions'][t], logp=bare['action_logp'][t], vf=bare['vf_preds'][t])
            nxt = obs[t + 1] if t + 1 < T else last
            env.step_into(bare['actions'][t], nxt, bare['rewards'][t])
            if env.time >= env.episode_length:
                env.reset_into(nxt)
        env.obs.copy_(last)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (n * T)

    n = max(1, a.steps // T)
    env.reset()
    bare_loop()
    hip_batch()
    res = {'bare': [], 'hip': []}
    for _ in range(3):
        env.reset()
        res['bare'].append(timed(bare_loop, n))
        env.reset()
        res['hip'].append(timed(hip_batch, n))
    live = float(state['buf']['live'].float().mean())
    print(f'{E} envs x {U} UE slots ({env.U0} initial, ue_arrival {arrival}) x {B} BS, actor 2x{a.hidden} tanh + value trunk, batches of T = {T}, {n} batches per timing')
    for k, name in (('bare', 'act + step_into loop (rows, no advantages)'), ('hip', 'sampler.collect(by_ue=True)' + (' (compact record)' if a.compact else ''))):
        ts = res[k]
        print(f'{name:<46}: ' + ' / '.join(f'{t * 1e3:.3f}' for t in ts) + f' ms/step  (best {E / min(ts):.3e} env-steps/s)')
    print(f'collect(by_ue=True) vs the bare loop: {min(res["hip"]) / min(res["bare"]):.2f} x the time; {live:.3f} of the rows of the last batch count')
    env.check()


def train_mode(iters):
    from deepcomp_amd.learner import PPOLearner, STATS
    from deepcomp_amd.sampler import collect, live_rows
    T = a.train_steps
    host_v = FcnetActor.random_value_weights(a.kind, U, B, a.hidden, seed=0)
    hip.set_value(host_v)
    rows = E * U if multi else E
    mb = a.minibatch or rows
    extra = dict(micro_rows=a.micro_rows or None, grad_clip=a.grad_clip or None)
    learner = PPOLearner(hip, lr=5e-5, max_rows=a.micro_rows or mb)
    env.reset()
    buf = None
    print(f'{E} envs x {U} UE x {B} BS ({a.kind}), 2x{a.hidden} tanh + value trunk, batches of T = {T} ({T * rows} rows), {a.sgd_iters} SGD iterations, minibatches of {mb}'
          + (', compact record' if a.compact else ''))
    for it in range(iters):
        buf = collect(env, hip, T, 0.99, 0.95, out=buf, dist_inputs=True, compact=a.compact, by_ue=bool(arrival))
        picked = live_rows(buf) if arrival else None
        st = learner.update(buf, num_sgd_iter=a.sgd_iters, minibatch_rows=mb, seed=it, rows=picked, check_rows=False, **extra)
        print(f'iter {it}: mean reward {float(buf["rewards"].mean()):+.4f}  ' + '  '.join(f'{n} {st[n]:+.5f}' for n in STATS) + f'  kl_coeff {st["kl_coeff"]:.3f}'
              + (f'  rows that count {picked.numel()} of {T * rows}' if arrival else ''))
    if arrival:                                                          # (the comparisons below take contiguous minibatches of a static env's batch)
        env.check()
        return
    if a.micro_rows:
        ts = []
        for _ in range(4):                                               # (the first: warm-up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            learner.update(buf, num_sgd_iter=1, minibatch_rows=mb, seed=0, **extra)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        print(f'one SGD iteration over {T * rows} rows, minibatches of {mb} accumulated in micro-batches of {a.micro_rows} (handle of {a.micro_rows} rows): '
              + ' / '.join(f'{t:.0f}' for t in ts[1:]) + ' us')
        env.check()
        return

    # ---- grads + apply on one minibatch against torch autograd (bf16 autocast) + torch.optim.Adam on the same network and loss
    rows_buf = buf
    if a.compact:                                                        # the contiguous-minibatch calls below take rows
        from deepcomp_amd.fragment import FragmentCodec
        codec = FragmentCodec(U, B, dev)
        rows_buf = {k: t for k, t in buf.items() if k != 'obs_compact'}
        rows_buf['obs'] = codec.unpack(buf['obs_compact'])
    f = lambda k, w: rows_buf[k].reshape(-1, w)[:mb].contiguous()        # noqa: E731
    obs, act = f('obs', D), f('actions', heads)
    olp, ologits = f('action_logp', heads), f('action_dist_inputs', heads * (B + 1))
    adv, vt, ovf = (buf[k].reshape(-1)[:mb].contiguous() for k in ('advantages', 'value_targets', 'vf_preds'))
    stats = torch.zeros(5, device=dev)

    def hip_step():
        learner.grads(obs, act, olp, ologits, adv, vt, ovf, stats=stats)
        learner.apply()

    names = ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')
    P = {n: torch.from_numpy(host_w[n]).to(dev).requires_grad_() for n in names}
    V = {n: torch.from_numpy(host_v[n]).to(dev).requires_grad_() for n in ('w1', 'b1', 'w2', 'b2', 'wv', 'bv')}
    opt = torch.optim.Adam(list(P.values()) + list(V.values()), lr=5e-5)
    act_l = act.long().unsqueeze(-1)
    hy = learner.hyper

    def torch_step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            h = torch.tanh(torch.addmm(P['b2'], torch.tanh(torch.addmm(P['b1'], obs, P['w1'])), P['w2']))
            logits = torch.addmm(P['b3'], h, P['w3'])
            g = torch.tanh(torch.addmm(V['b2'], torch.tanh(torch.addmm(V['b1'], obs, V['w1'])), V['w2']))
            v = (g @ V['wv'].unsqueeze(-1)).squeeze(-1)
        v = v.float() + V['bv']
        lsm = torch.log_softmax(logits.float().view(mb, heads, B + 1), -1)
        lso = torch.log_softmax(ologits.view(mb, heads, B + 1), -1)
        ratio = (lsm.gather(-1, act_l).squeeze(-1).sum(1) - olp.sum(1)).exp()
        surr = torch.minimum(adv * ratio, adv * ratio.clamp(1 - hy['clip_param'], 1 + hy['clip_param']))
        kl = (lso.exp() * (lso - lsm)).sum((1, 2))
        ent = -(lsm.exp() * lsm).sum((1, 2))
        vc = ovf + (v - ovf).clamp(-hy['vf_clip_param'], hy['vf_clip_param'])
        vfl = torch.maximum((v - vt) ** 2, (vc - vt) ** 2)
        (-surr + hy['kl_coeff'] * kl + hy['vf_loss_coeff'] * vfl - hy['entropy_coeff'] * ent).mean().backward()
        opt.step()

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    n = max(3, min(50, a.steps))
    for fn in (hip_step, torch_step):
        timed(fn, 2)
    res = {'hip': [], 'torch': []}
    for _ in range(3):                                  # interleaved: drift of the clocks shows as spread, not as a difference
        res['hip'].append(timed(hip_step, n))
        res['torch'].append(timed(torch_step, n))
    print(f'one minibatch of {mb} rows, {n} back-to-back steps per timing, HIP events')
    print('PPOLearner grads + apply                      : ' + ' / '.join(f'{t:.0f}' for t in res['hip']) + ' us')
    print('torch autograd (bf16 autocast) + Adam         : ' + ' / '.join(f'{t:.0f}' for t in res['torch']) + ' us')
    print(f'torch / PPOLearner: {min(res["torch"]) / min(res["hip"]):.2f} x')

    # ---- one SGD iteration of update: gathered minibatches (rows), a row index into the rows where they lie, a row index into the record
    N = T * rows
    flat = {'obs': rows_buf['obs'].reshape(-1, D), 'actions': rows_buf['actions'].reshape(-1, heads), 'old_logp': rows_buf['action_logp'].reshape(-1, heads),
            'old_logits': rows_buf['action_dist_inputs'].reshape(-1, heads * (B + 1)), 'advantages': rows_buf['advantages'].reshape(-1),
            'value_targets': rows_buf['value_targets'].reshape(-1), 'old_vf': rows_buf['vf_preds'].reshape(-1)}
    gen = torch.Generator(device=dev)

    def indexed_iteration():
        """update's iteration on the rows batch with grads_indexed in place of the gather"""
        src = dict(flat)
        adv_ = src['advantages']
        src['advantages'] = (adv_ - adv_.mean()) / adv_.std(unbiased=False).clamp_min(1e-4)
        starts = list(range(0, N, mb))
        st = torch.zeros((len(starts), 5), device=dev)
        gen.manual_seed(0)
        index = torch.randperm(N, generator=gen, device=dev).to(torch.int32)
        for i, s0 in enumerate(starts):
            learner.grads_indexed(src, index[s0:s0 + mb], stats=st[i])
            learner.apply()
        return st.mean(0).cpu()

    def wall(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / k

    k = max(2, min(20, a.steps))
    variants = [('update, rows batch (gathered minibatches)', lambda: learner.update(rows_buf, num_sgd_iter=1, minibatch_rows=mb, seed=0)),
                ('the same through a row index (grads_indexed)', indexed_iteration)]
    if a.compact:
        variants.append(('update, compact batch (row index)', lambda: learner.update(buf, num_sgd_iter=1, minibatch_rows=mb, seed=0)))
        variants.append(('unpack of the compact batch to rows', lambda: codec.unpack(buf['obs_compact'], out=rows_buf['obs'])))
    for _, fn in variants:
        wall(fn, 1)
    times = {name: [] for name, _ in variants}
    for _ in range(3):
        for name, fn in variants:
            times[name].append(wall(fn, k))
    print(f'one SGD iteration over {N} rows in minibatches of {mb}, {k} iterations per timing, wall clock with the final read of the statistics')
    for name, _ in variants:
        print(f'{name:<46}: ' + ' / '.join(f'{t:.0f}' for t in times[name]) + ' us')
    env.check()


def per_ue_mode():
    """The shared policy and a set of U distinct members on the same env, interleaved."""
    from deepcomp_amd.learner import PPOLearner
    from deepcomp_amd.policy_set import PerUEActor, PerUELearner
    from deepcomp_amd.sampler import collect
    hip.set_value(FcnetActor.random_value_weights(a.kind, U, B, a.hidden, seed=0))
    pset = PerUEActor.random(U, B, hidden=a.hidden, seed=0, device=dev)                # member p from seed p: member 0 is the shared policy's twin
    actors = {'shared policy': hip, f'per-UE set, {U} policies': pset}
    rows = E * U
    form = ', compact record' if a.compact else ''
    print(f'{E} envs x {U} UE x {B} BS (multi), 2x{a.hidden} tanh + value trunk{form}')

    def wall(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    def report(what, fns, n, per=1):
        for fn in fns.values():
            fn()
        res = {k: [] for k in fns}
        for _ in range(3):
            for k, fn in fns.items():
                res[k].append(wall(fn, n) / per)
        for k, ts in res.items():
            print(f'{what}, {k:<28}: ' + ' / '.join(f'{t:.3f}' for t in ts) + ' ms')
        best = [min(ts) for ts in res.values()]
        print(f'{what}: set / shared = {best[1] / best[0]:.2f} x')
        return res

    env.reset()
    if a.train:
        T = a.train_steps
        mb = a.minibatch or rows // U
        learners = {k: (PPOLearner(x, lr=5e-5, max_rows=mb * (U if x is hip else 1)) if x is hip else PerUELearner(x, lr=5e-5, max_rows=mb))
                    for k, x in actors.items()}
        bufs = {k: None for k in actors}
        print(f'batches of T = {T} ({T * rows} rows), minibatches of {mb} rows per policy ({mb * U} for the shared policy)')
        for it in range(a.train):
            for k, x in actors.items():
                bufs[k] = collect(env, x, T, 0.99, 0.95, out=bufs[k], dist_inputs=True, compact=a.compact)
                st = learners[k].update(bufs[k], num_sgd_iter=a.sgd_iters, minibatch_rows=mb * (U if x is hip else 1), seed=it)
                st = st if isinstance(st, dict) else {n: sum(s[n] for s in st) / len(st) for n in st[0]}
                print(f'iter {it}, {k}: mean reward {float(bufs[k]["rewards"].mean()):+.4f}  total_loss {st["total_loss"]:+.5f}  kl {st["kl"]:+.5f} (mean over policies)')
        fns = {k: (lambda k=k, x=x: learners[k].update(bufs[k], num_sgd_iter=1, minibatch_rows=mb * (U if x is hip else 1), seed=0))
               for k, x in actors.items()}
        if a.grouped:
            ks = list(actors)[1]
            fns['per-UE set, grouped launches'] = lambda: learners[ks].update(bufs[ks], num_sgd_iter=1, minibatch_rows=mb, seed=0, grouped=True)
        res = report('one SGD iteration of update', fns, max(2, min(10, a.steps)))
        if a.grouped:
            seq, grp = sorted(res[list(actors)[1]]), sorted(res['per-UE set, grouped launches'])
            print(f'grouped / sequential (medians) = {grp[1] / seq[1]:.3f} x; sequential {seq[0]:.3f} ... {seq[2]:.3f} ms, grouped {grp[0]:.3f} ... {grp[2]:.3f} ms, '
                  f'shared learner (the floor) median {sorted(res[list(actors)[0]])[1]:.3f} ms')
    elif a.collect:
        T = a.collect
        bufs = {k: None for k in actors}

        def batch(k):
            bufs[k] = collect(env, actors[k], T, 0.99, 0.95, compact=a.compact, out=bufs[k])
        report(f'collect, T = {T}, per step', {k: (lambda k=k: batch(k)) for k in actors}, max(1, a.steps // T), per=T)
    else:
        pk = torch.zeros((E, env.compact_words), dtype=torch.int32, device=dev) if a.compact else None
        out = torch.zeros((E, U), dtype=torch.uint8, device=dev)

        def loop(x):
            if env.time >= env.episode_length:
                env.reset_compact(pk) if a.compact else env.reset()
            x.act(env, obs=pk if a.compact else None, compact=a.compact, out=out)
            if a.compact:
                env.step_compact(out, pk, env.reward)
            else:
                env.step(out)
        if a.compact:
            env.reset_compact(pk)
        report('env step + actor, per step', {k: (lambda x=x: loop(x)) for k, x in actors.items()}, a.steps)
    env.check()


def per_id_mode(iters):
    """--per-ue --ue-arrival: a set keyed by UE id, one member per id the schedule ever lists: collect(by_ue=True) -> PerIdLearner.update."""
    from deepcomp_amd.policy_set import PerIdActor, PerIdLearner
    from deepcomp_amd.sampler import collect
    T = a.train_steps
    P = env.max_id
    pset = PerIdActor.random(U, B, P, hidden=a.hidden, seed=0, device=dev)
    mb = a.minibatch or E * T
    extra = dict(micro_rows=a.micro_rows or None, grad_clip=a.grad_clip or None)
    learner = PerIdLearner(pset, lr=5e-5, max_rows=a.micro_rows or mb)
    print(f'{E} envs x {U} UE slots ({env.U0} initial, ue_arrival {arrival}, ids up to {P}) x {B} BS, {P} policies 2x{a.hidden} tanh + value trunk, '
          f'batches of T = {T} ({T * E * U} rows), {a.sgd_iters} SGD iterations, minibatches of {mb} per policy' + (', grouped' if a.grouped else '')
          + (', compact record' if a.compact else ''))
    env.reset()
    buf = None
    for it in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        buf = collect(env, pset, T, 0.99, 0.95, out=buf, dist_inputs=True, compact=a.compact, by_ue=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        stats = learner.update(buf, num_sgd_iter=a.sgd_iters, minibatch_rows=mb, seed=it, grouped=a.grouped, **extra)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        trained = [s for s in stats if s is not None]
        print(f'iter {it}: mean reward {float(buf["rewards"].mean()):+.4f}  rows that count {int(buf["live"].sum())} of {T * E * U}  policies trained {len(trained)} of {P}  '
              f'total_loss {sum(s["total_loss"] for s in trained) / len(trained):+.5f}  kl {sum(s["kl"] for s in trained) / len(trained):+.5f} (mean over policies)  '
              f'collect {(t1 - t0) * 1e3:.1f} ms  update {(t2 - t1) * 1e3:.1f} ms')
    env.check()


if a.per_ue and arrival:
    per_id_mode(a.train or 3)
    sys.exit(0)
if a.per_ue:
    per_ue_mode()
    sys.exit(0)
if a.collect:
    collect_mode(a.collect)
    sys.exit(0)
if a.train:
    train_mode(a.train)
    sys.exit(0)
packed = torch.zeros((E, env.compact_words), dtype=torch.int32, device=dev) if a.compact else None
act_buf = torch.zeros((E, U), dtype=torch.uint8, device=dev)


def run(n, actor):
    """n steps of the loop; actor: None (a fixed action tensor), 'torch' or 'hip'."""
    compact = actor == 'hip' and a.compact
    obs = env.reset_compact(packed) if compact else env.reset()
    act = torch.zeros((E, U), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(n):
        if t and t % 100 == 0:
            obs = env.reset_compact(packed) if compact else env.reset()
        if actor == 'torch':
            act = policy(obs)
        elif actor == 'hip':
            act = hip.act(env, obs=packed if compact else None, compact=compact, out=act_buf)
        if compact:
            env.step_compact(act, packed, env.reward)
        else:
            obs = env.step(act)[0]
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def report(name, t):
    print(f'{name:<34}: {t * 1e3:8.3f} ms/step  {E / t:.3e} env-steps/s  ({E * U / t:.3e} agent-steps/s)  env share {100 * t_env / t:.1f} %')


run(20, 'torch')
if hip is not None:
    run(20, 'hip')
t_env = run(a.steps, None)
print(f'{E} envs x {U} UE x {B} BS ({a.kind}), actor 2x{a.hidden} tanh, sampled actions')
print(f'{"env only":<34}: {t_env * 1e3:8.3f} ms/step  {E / t_env:.3e} env-steps/s')
t_torch = run(a.steps, 'torch')
report(f'env + torch actor ({a.dtype})', t_torch)
if hip is not None:
    t_hip = run(a.steps, 'hip')
    report('env + hip actor' + (' (compact record)' if a.compact else ''), t_hip)
    t_torch2 = run(a.steps, 'torch')               # the torch loop again: drift of the clocks between the two measurements
    report(f'env + torch actor ({a.dtype}), again', t_torch2)
    print(f'hip actor loop vs torch actor loop: {min(t_torch, t_torch2) / t_hip:.2f} x')
env.check()
