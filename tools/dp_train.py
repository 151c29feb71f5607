#!/usr/bin/env python3
"""One data-parallel PPO step end to end: env shards, collect, DataParallelLearner.update, check_sync.

    python tools/dp_train.py --world 2 [--backend nccl|gloo] [--same-device] [--envs 64 --ues 4 --bs 5 --steps 8 --hidden 32]
                             [--sgd-iters 1] [--minibatch GLOBAL_ROWS] [--micro-rows ROWS] [--grad-clip NORM] [--compact] [--per-ue]
    python tools/dp_train.py --lockstep 2 [...]

--world N: this command starts N ranks as fresh child processes (RANK / WORLD_SIZE / MASTER_* in their environment), each with a
time limit; a child that fails or runs out of time ends the run, the others are stopped and nothing more is started.  Every rank
builds its shard of the env axis (deepcomp_amd.sharded.make_sharded_env: --envs per rank), the same random-init actor, collects
--steps steps and runs one DataParallelLearner.update on its shard, then check_sync.  Rank 0 prints one JSON line: every rank's
sha256 of its master weights (equal, or check_sync has raised), the statistics and the seconds per phase.  --same-device: every rank
uses cuda:0 (a dry run on one GPU; with --backend gloo the reductions are staged through the host).

--lockstep R: the same R ranks in ONE process on one GPU through deepcomp_amd.dp_learner.run_lockstep, the reductions staged through
the host: the same phases, the same bits (a sum of two f32 terms does not depend on the order), no process group.

--per-ue: one policy per UE slot (deepcomp_amd.policy_set: a PerUEActor collects, a DataParallelPerUELearner trains the set's policies
together); --minibatch is then the GLOBAL minibatch PER POLICY, the statistics are a list with one entry per policy, and a rank's
sha256 is taken over its policies' sha256 in order."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--world', type=int, default=0, help='ranks, each a fresh child process')
    ap.add_argument('--lockstep', type=int, default=0, metavar='R', help='R ranks in this process through run_lockstep')
    ap.add_argument('--backend', default='nccl', choices=['nccl', 'gloo'])
    ap.add_argument('--same-device', action='store_true', help='dry run: every rank uses cuda:0')
    ap.add_argument('--envs', type=int, default=64, help='envs PER RANK')
    ap.add_argument('--ues', type=int, default=4)
    ap.add_argument('--bs', type=int, default=5)
    ap.add_argument('--steps', type=int, default=8, help='steps of the collected batch')
    ap.add_argument('--hidden', type=int, default=32)
    ap.add_argument('--sgd-iters', type=int, default=1)
    ap.add_argument('--minibatch', type=int, default=0, help='rows of the GLOBAL minibatch (default: the whole batch)')
    ap.add_argument('--micro-rows', type=int, default=0, help='rows per micro-batch of a rank (a multiple of 2048)')
    ap.add_argument('--grad-clip', type=float, default=0.0)
    ap.add_argument('--compact', action='store_true', help='collect the compact record and train on it through the row index')
    ap.add_argument('--per-ue', action='store_true', help='one policy per UE slot, trained as a data-parallel per-UE set')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--timeout', type=float, default=300.0, help='seconds a child may take')
    a = ap.parse_args()
    if (a.world > 0) == (a.lockstep > 0):
        ap.error('give --world N or --lockstep R')
    return a


def free_port():
    """Below the kernel's ephemeral range: a bind(0) port can be handed to any outgoing connection before rank 0 binds it."""
    import random
    import socket
    for _ in range(64):
        port = random.randrange(20000, 32000)
        s = socket.socket()
        try:
            s.bind(('127.0.0.1', port))
            return port
        except OSError:
            continue
        finally:
            s.close()
    sys.exit('dp_train.py: no free rendezvous port between 20000 and 32000')


def spawn(a):
    """The ranks as fresh children of this process, which has not touched the GPU.  Rank 0 owns stdout."""
    port = free_port()
    procs = []
    for r in range(a.world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'), DCOMP_DP_TRAIN_CHILD='1')
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, stdout=None if r == 0 else sys.stderr))
    deadline = time.monotonic() + a.timeout
    status = 0
    while status == 0 and any(p.poll() is None for p in procs):
        for r, p in enumerate(procs):
            if p.poll() not in (None, 0):
                status = p.returncode
                print(f'dp_train.py: rank {r} ended with status {status}', file=sys.stderr)
        if status == 0 and time.monotonic() > deadline:
            status = 124
            print(f'dp_train.py: the ranks did not finish within {a.timeout:g} s', file=sys.stderr)
        if status == 0:
            time.sleep(0.05)
    for p in procs:                                          # after a failure: stop what still runs, start nothing more
        if p.poll() is None:
            p.kill()
        p.wait()
    for r, p in enumerate(procs):
        if status == 0 and p.returncode != 0:
            status = p.returncode
    sys.exit(status if 0 <= status < 256 else 1)


def make_rank(a, rank, world, dev):
    """(env, learner) of one rank: its shard of the env axis and the actor every rank builds from the same seeds."""
    from deepcomp_amd import build as hip_build
    from deepcomp_amd import scenarios
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.learner import PPOLearner
    from deepcomp_amd.sharded import make_sharded_env
    if not hip_build.up_to_date():
        raise SystemExit('dp_train.py: build the HIP extension first (python -m deepcomp_amd.build)')
    scn = scenarios.grid_map(a.bs, 'mixed').with_ues(num_slow=a.ues)
    env = make_sharded_env(scn, 'multi', a.envs * world, rank, world, device=dev, seed=42, episode_length=100, rng='philox', rand_episodes=True)
    local_rows = a.envs * a.steps * (1 if a.per_ue else a.ues)       # (per policy: every UE slot has its own)
    share = min(a.minibatch // world, local_rows) if a.minibatch else local_rows
    if a.per_ue:
        from deepcomp_amd.policy_set import PerUEActor, PerUELearner
        return env, PerUELearner(PerUEActor.random(a.ues, a.bs, a.hidden, 'tanh', seed=1, bias_std=0.1, device=dev), lr=a.lr, max_rows=a.micro_rows or share)
    w = FcnetActor.random_weights('multi', a.ues, a.bs, a.hidden, seed=1, bias_std=0.1)
    vw = FcnetActor.random_value_weights('multi', a.ues, a.bs, a.hidden, seed=1, bias_std=0.1)
    actor = FcnetActor('multi', a.ues, a.bs, w, activation='tanh', device=dev, value_weights=vw)
    return env, PPOLearner(actor, lr=a.lr, max_rows=a.micro_rows or share)


def update_args(a):
    return dict(num_sgd_iter=a.sgd_iters, minibatch_rows=a.minibatch or None, micro_rows=a.micro_rows or None, seed=a.seed,
                grad_clip=a.grad_clip or None)


def dp_of(a, learner, **kw):
    from deepcomp_amd.dp_learner import DataParallelLearner, DataParallelPerUELearner
    return (DataParallelPerUELearner if a.per_ue else DataParallelLearner)(learner, **kw)


def one_sha(sha):
    """check_sync's result as one sha256: a set's is taken over its policies' in order."""
    import hashlib
    return sha if isinstance(sha, str) else hashlib.sha256(''.join(sha).encode()).hexdigest()


def report(a, mode, world, shas, stats, seconds, t_collect, t_update):
    print(json.dumps({'tool': 'dp_train', 'mode': mode, 'world': world, 'backend': a.backend if mode == 'ranks' else None,
                      'rows_per_rank': a.envs * a.ues * a.steps, 'sha256': shas, 'in_sync': len(set(shas)) == 1, 'stats': stats,
                      'seconds': dict(seconds, collect=t_collect, update=t_update)}), flush=True)


def child(a):
    import torch
    import torch.distributed as dist
    from deepcomp_amd.sampler import collect
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    if not a.same_device and torch.cuda.device_count() < world:
        sys.exit(f'dp_train.py: --world {world} but only {torch.cuda.device_count()} GPU(s) are visible (--same-device --backend gloo: dry run on one)')
    dev = torch.device('cuda', 0 if a.same_device else rank)
    torch.cuda.set_device(dev)
    if a.backend == 'nccl':
        dist.init_process_group('nccl', device_id=dev)
    else:
        dist.init_process_group(a.backend)
    try:
        env, learner = make_rank(a, rank, world, dev)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        batch = collect(env, learner.actor, a.steps, 0.99, 0.95, dist_inputs=True, compact=a.compact)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        dp = dp_of(a, learner, group=dist.group.WORLD)
        dp.profile = True
        stats = dp.update(batch, **update_args(a))
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        sha = one_sha(dp.check_sync())
        # every rank's sha256 on rank 0: one SUM of a [world, 32] table in which a rank fills its own row
        table = torch.zeros((world, 32), dtype=torch.int64, device=dev)
        table[rank] = torch.tensor(list(bytes.fromhex(sha)), dtype=torch.int64, device=dev)
        dp._reduce(table, 'sum')
        if rank == 0:
            shas = [bytes(row).hex() for row in table.cpu().tolist()]
            report(a, 'ranks', world, shas, stats, dp.seconds, t1 - t0, t2 - t1)
    finally:
        dist.destroy_process_group()


def lockstep(a):
    import torch
    from deepcomp_amd.dp_learner import run_lockstep
    from deepcomp_amd.sampler import collect
    R = a.lockstep
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    ranks = [make_rank(a, r, R, dev) for r in range(R)]
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    batches = [collect(env, learner.actor, a.steps, 0.99, 0.95, dist_inputs=True, compact=a.compact) for env, learner in ranks]
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    dps = [dp_of(a, learner, rank=r, world=R) for r, (_, learner) in enumerate(ranks)]
    for d in dps:
        d.profile = True
    reduce_s = {}
    stats = run_lockstep(dps, batches, host_staged=True, seconds=reduce_s, **update_args(a))
    torch.cuda.synchronize(dev)
    t2 = time.perf_counter()
    shas = [one_sha(s) for s in run_lockstep(dps, phases='check_sync', host_staged=True)]
    # per rank: the local phases; the reductions: the driver's clock (a rank's own also sees the other ranks' phases)
    seconds = {k: sum(d.seconds[k] for d in dps) / R for k in ('accumulate', 'finish', 'apply')}
    seconds['reduce'] = reduce_s.get('reduce', 0.0)
    report(a, 'lockstep', R, shas, stats[0], seconds, (t1 - t0) / R, t2 - t1)


if __name__ == '__main__':
    args = parse()
    if args.lockstep:
        lockstep(args)
    elif os.environ.get('DCOMP_DP_TRAIN_CHILD') == '1':
        child(args)
    else:
        spawn(args)
