#!/usr/bin/env python3
"""One SGD iteration of a per-UE policy set with micro-batches and grad_clip (include/dcomp_learner_group_accum.h), grouped against
the per-member calls it replaces, on one GPU:

    python tools/group_accum_bench.py [--shapes 4096x128x32x64,4096x128x32x256] [--steps 5] [--minibatch 4096] [--micro-rows 2048]
                                      [--grad-clip 0.5] [--repeats 3] [--out FILE]

Per shape E x U x B x hidden (multi-agent, tanh, P = U distinct random-init members with value trunks, a compact batch of --steps
steps collected by the set, --minibatch rows PER POLICY), three variants of one SGD iteration, interleaved --repeats times after a
warm call each, synchronised wall clock over the whole update:
  (a) PerUELearner.update(grouped=True, micro_rows=M, grad_clip=c) on learners with max_rows = M
  (b) the P member calls PPOLearner.update(rows=, micro_rows=M, grad_clip=c) on the same learners: what (a) replaces
  (c) PerUELearner.update(grouped=True) without accumulation, on learners whose max_rows holds the minibatch
and the device memory the two sets of learners took when they were created (free memory before and after: the workspaces are the
library's own allocations), max_rows = M against max_rows = minibatch.  profiles/r20_group_accum.txt section 2 is this output."""
import argparse
import sys
import time

sys.path.insert(0, '.')
import torch

from deepcomp_amd import scenarios
from deepcomp_amd.entities import build_from_scenario
from deepcomp_amd.env import BatchedMobileEnv
from deepcomp_amd.policy_set import PerUEActor, PerUELearner
from deepcomp_amd.sampler import collect

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', default='4096x128x32x64,4096x128x32x256', help='comma-separated E x U x B x hidden')
ap.add_argument('--steps', type=int, default=5)
ap.add_argument('--minibatch', type=int, default=4096, help='rows of a minibatch PER POLICY')
ap.add_argument('--micro-rows', type=int, default=2048)
ap.add_argument('--grad-clip', type=float, default=0.5)
ap.add_argument('--repeats', type=int, default=3)
ap.add_argument('--out', default='', help='also write the lines to this file')
a = ap.parse_args()
dev = torch.device('cuda', 0)
log = open(a.out, 'w') if a.out else None


def say(line):
    print(line, flush=True)
    if log:
        log.write(line + '\n')
        log.flush()


def learners(U, B, H, max_rows):
    """(set of learners, bytes of device memory their creation took)."""
    torch.cuda.synchronize(dev)
    before = torch.cuda.mem_get_info(dev)[0]
    ln = PerUELearner(PerUEActor.random(U, B, hidden=H, seed=0, bias_std=0.1, device=dev), lr=1e-4, max_rows=max_rows)
    torch.cuda.synchronize(dev)
    return ln, before - torch.cuda.mem_get_info(dev)[0]


def timed(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


for shape in a.shapes.split(','):
    E, U, B, H = (int(x) for x in shape.split('x'))
    m, bs, ues = build_from_scenario(scenarios.grid_map(B, 'mixed').with_ues(num_slow=U))
    env = BatchedMobileEnv(m, bs, ues, 'multi', num_envs=E, seed=42, episode_length=100, rng='philox', rand_episodes=True, device=dev)
    small, small_bytes = learners(U, B, H, a.micro_rows)
    whole, whole_bytes = learners(U, B, H, a.minibatch)
    batch = collect(env, small.actor, a.steps, 0.99, 0.95, dist_inputs=True, compact=True)
    rows = small.rows_of(int(batch['actions'].numel()))
    kw = dict(num_sgd_iter=1, minibatch_rows=a.minibatch)
    acc = dict(kw, micro_rows=a.micro_rows, grad_clip=a.grad_clip)
    fns = {'(a) grouped, micro_rows + grad_clip': lambda: small.update(batch, seed=0, grouped=True, **acc),
           '(b) member calls, micro_rows + grad_clip': lambda: [ln.update(batch, seed=p, rows=rows[p], check_rows=False, **acc) for p, ln in enumerate(small.learners)],
           '(c) grouped, unaccumulated': lambda: whole.update(batch, seed=0, grouped=True, **kw)}
    for fn in fns.values():
        fn()                                                 # warm: the group handle, the gather buffers, the allocator
    res = {k: [] for k in fns}
    for _ in range(a.repeats):                               # interleaved: drift of the clocks shows as spread, not as a difference
        for k, fn in fns.items():
            res[k].append(timed(fn))
    say(f'{E} envs x {U} UE x {B} BS, 2x{H} tanh + value trunk, P = {U} policies, compact batch of T = {a.steps} ({E * a.steps} rows per policy), '
        f'minibatches of {a.minibatch} rows per policy, micro_rows {a.micro_rows}, grad_clip {a.grad_clip}')
    for k, v in res.items():
        say(f'   one SGD iteration, {k:42s}: ' + ' / '.join(f'{x:.3f}' for x in v) + ' ms')
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    ka, kb, kc = list(fns)
    say(f'   medians: (a) / (b) = {med[ka] / med[kb]:.3f} x, (a) / (c) = {med[ka] / med[kc]:.3f} x')
    say(f'   device memory of the {U} learners: max_rows = {a.micro_rows}: {small_bytes / 2 ** 20:.1f} MiB, max_rows = {a.minibatch}: {whole_bytes / 2 ** 20:.1f} MiB '
        f'({small_bytes / max(whole_bytes, 1):.3f} x)')
    del small, whole, batch, env
