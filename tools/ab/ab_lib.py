#!/usr/bin/env python3
"""A/B of library builds on ONE GPU box (boxes differ by +-3 %, so only same-box comparisons count).

  python tools/ab/ab_lib.py build <tag> [--ref GITREF | --src TREE] [--b 5,10,32] [--flags "-DX=1 ..."]     (build container)
        -> deepcomp_amd/csrc/variants/libdcomp_hip_<tag>.so from the working tree, from the sources at GITREF
           (csrc/ + include/ exported to a scratch directory) or from an edited copy of the tree (a variant: the product headers
           carry no build switches); only the listed base-station counts (seconds, not minutes)
  python tools/ab/ab_lib.py run <tag> <tag> ... [--rounds 2] [--only c3,c2roll,...]              (GPU box, via gpurun)
        -> every workload timed with every library, interleaved `rounds` times, one child process per (library, round);
           prints kernel ms per step (HIP events, steady state) and the ratio to the first tag
  python tools/ab/ab_lib.py measure [--only ...]     (child: the library is whatever DCOMP_LIB names)

Workloads: BASELINE config 3 (65 536 x 32 x 10 multi, one launch per step), config 2 through the fused rollout (4 096 x 10 x 5
central, 100 steps per launch, every step's outputs), one GPU's share of config 5 (4 096 x 128 x 32) and of config 4
(32 768 x 32 x 10), 65 536 x 10 x 5 central, 65 536 x 32 x 10 central, the closed policy loop at config 2; learner_c3 / learner_c2:
PPOLearner grads + apply on one minibatch of 65 536 x 32 multi rows / 4 096 central rows (libraries from round 9 on); actor_c3 / actor_c2:
dcomp_actor_actions_v (actions, logp and the value of a trunk of its own, sampled) at 65 536 x 32 x 10 multi / 4 096 x 10 x 5 central
(libraries from round 8 on); update_c2 / update_c3s / update_per_ue: the host side of the learners' update() at launch-bound shapes
(profiles/r18_sgd_phase.txt) -- wall-clock ms per call, not kernel time; step_philox / step_reference / step_philox_dyn and the compat_*
loops: the host side of BatchedMobileEnv.step() and of the single-env classes (profiles/r19_env_tape.txt), wall clock as well.  For the
wall-clock workloads `run` also prints the median over the rounds and their spread (max - min).  A tag `py:TREE` times the working tree's library under the
Python package of another checkout (TREE/deepcomp_amd, e.g. `git archive <ref> deepcomp_amd | tar -x -C TREE`): a host-side A/B."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # tools/ab/ -> the repo
CSRC = os.path.join(REPO, 'deepcomp_amd', 'csrc')
VAR = os.path.join(CSRC, 'variants')
BASE = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=fast-honor-pragmas']


def build(a):
    os.makedirs(VAR, exist_ok=True)
    src = a.src or REPO
    tmp = None
    if a.ref:
        tmp = tempfile.mkdtemp(prefix='dcomp_ref_')
        subprocess.check_call(f'git -C {REPO} archive {a.ref} deepcomp_amd/csrc include | tar -x -C {tmp}', shell=True)
        src = tmp
    bl = [int(x) for x in a.b.split(',')]
    flags = BASE + [f for f in a.flags.split() if f] + ['-DDCOMP_B_LIST(X)=' + ' '.join(f'X({b})' for b in bl),
                                                         '-DDCOMP_B_LIST_STR="' + ','.join(map(str, bl)) + ' (A/B build)"']
    csrc = os.path.join(src, 'deepcomp_amd', 'csrc')
    objdir = tempfile.mkdtemp(prefix='dcomp_obj_')
    procs = []
    for b in bl:
        o = os.path.join(objdir, f'b{b}.o')
        procs.append((o, subprocess.Popen(['hipcc'] + flags + [f'-DDCOMP_B={b}', '-c', os.path.join(csrc, 'dcomp_inst.hip'), '-o', o],
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    # the ABI + dispatch, the generic kernel dcomp_api.hip links against (round 5 on), the fcnet actor and the PPO learner (rounds 7, 9 on)
    for name in ('api', 'big', 'actor', 'learner'):
        if not os.path.exists(os.path.join(csrc, f'dcomp_{name}.hip')):
            continue
        o = os.path.join(objdir, f'{name}.o')
        procs.append((o, subprocess.Popen(['hipcc'] + flags + ['-c', os.path.join(csrc, f'dcomp_{name}.hip'), '-o', o], stdout=subprocess.PIPE,
                                          stderr=subprocess.STDOUT, text=True)))
    for o, p in procs:
        out, _ = p.communicate()
        if p.returncode:
            sys.exit(out[-4000:])
    so = os.path.join(VAR, f'libdcomp_hip_{a.tag}.so')
    subprocess.check_call(['hipcc', '--offload-arch=gfx950', '-shared', '-fPIC', '-o', so] + [o for o, _ in procs] + ['-lpthread'])
    shutil.rmtree(objdir)
    if tmp:
        shutil.rmtree(tmp)
    print(so, os.path.getsize(so) >> 20, 'MiB')


WORKLOADS = ['big64', 'big40c', 'c3', 'c2roll', 'c5', 'c5mid', 'c5big', 'c4share', 'c4big', 'central10x5', 'central10x5roll', 'central10x5f', 'central32x10', 'c2policy', 'c3rf', 'c3roll',
             'learner_c3', 'learner_c2', 'actor_c3', 'actor_c2']
UPDATES = ['update_c2', 'update_c3s', 'update_per_ue']        # run on request only (--only): wall clock, and a collect() batch each
ENV_STEPS = {'step_philox': dict(rng='philox'), 'step_reference': dict(rng='reference'), 'step_philox_dyn': dict(rng='philox', new_ue_interval=25)}
COMPAT = {'compat_multi32x10': 'multi 32x10', 'compat_central10x5': 'central 10x5', 'compat_central3x3': 'central 3x3'}     # tools/compat_rate.py's loops
WALL = UPDATES + list(ENV_STEPS) + list(COMPAT)               # all of them on request only


def measure_actor(torch, dev, kind, E, U, B, n):
    """FcnetActor.actions with logp and vf (2 x 256 tanh, a value trunk of its own, sampled; synthetic observations: the time does not
    depend on the values), ms per launch over n back-to-back launches."""
    from deepcomp_amd.actor import FcnetActor
    actor = FcnetActor(kind, U, B, FcnetActor.random_weights(kind, U, B, 256, seed=0), device=dev,
                       value_weights=FcnetActor.random_value_weights(kind, U, B, 256, seed=0))
    rows = E * U if kind == 'multi' else E
    g = torch.Generator(device=dev).manual_seed(3)
    obs = torch.rand((E, U, actor.num_in) if kind == 'multi' else (E, actor.num_in), generator=g, device=dev)
    out = torch.zeros((E, U), dtype=torch.uint8, device=dev)
    logp, vf = torch.zeros((rows, actor.heads), device=dev), torch.zeros(rows, device=dev)

    def step(i):
        actor.actions(obs, sample=True, seed=1, step=i, out=out, logp=logp, vf=vf)
    for i in range(3):
        step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        step(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def measure_learner(torch, dev, kind, E, U, B, n):
    """PPOLearner grads + apply on one minibatch of E envs' rows (2 x 256 tanh, a value trunk of its own; synthetic inputs: the time
    does not depend on the values), ms per step over n back-to-back steps, through dcomp_learner_grads -- the entry point every
    library since round 9 has."""
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.learner import PPOLearner
    actor = FcnetActor(kind, U, B, FcnetActor.random_weights(kind, U, B, 256, seed=0), device=dev,
                       value_weights=FcnetActor.random_value_weights(kind, U, B, 256, seed=0))
    rows = E * U if kind == 'multi' else E
    learner = PPOLearner(actor, lr=5e-5, max_rows=rows)
    g = torch.Generator(device=dev).manual_seed(3)
    r = lambda *shape: torch.rand(shape, generator=g, device=dev)                 # noqa: E731
    obs, logits = r(rows, actor.num_in), r(rows, actor.num_logits)
    act = torch.randint(0, B + 1, (rows, actor.heads), generator=g, device=dev, dtype=torch.uint8)
    olp = torch.log_softmax(logits.view(rows, actor.heads, B + 1), -1).gather(-1, act.long().unsqueeze(-1)).squeeze(-1).contiguous()
    adv, vt, ovf = r(rows) - 0.5, r(rows), r(rows)
    stats = torch.zeros(5, device=dev)

    def step():
        learner.grads(obs, act, olp, logits, adv, vt, ovf, stats=stats)
        learner.apply()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def measure_update(torch, dev, w, calls=12):
    """One learner update() per call, wall clock with a device synchronise on both sides: the median of `calls` calls after two
    warm-up calls, in ms.  num_sgd_iter 4, four minibatches; a collect() batch of the shape.  update_c2: PPOLearner, 4 096 x 10 x 5
    central, T = 2, hidden 256, rows; update_c3s: PPOLearner, 1 024 x 32 x 10 multi, T = 2, hidden 256, the compact record;
    update_per_ue: PerUELearner(grouped=True), 256 x 10 x 5, T = 4, hidden 64, ten policies."""
    import statistics
    import time
    from deepcomp_amd import scenarios
    from deepcomp_amd.actor import FcnetActor
    from deepcomp_amd.entities import build_from_scenario
    from deepcomp_amd.env import BatchedMobileEnv
    from deepcomp_amd.learner import PPOLearner
    from deepcomp_amd.policy_set import PerUEActor, PerUELearner
    from deepcomp_amd.sampler import collect
    kind, E, U, B, T, H, compact = {'update_c2': ('central', 4096, 10, 5, 2, 256, False), 'update_c3s': ('multi', 1024, 32, 10, 2, 256, True),
                                    'update_per_ue': ('multi', 256, 10, 5, 4, 64, False)}[w]
    m, bs, ues = build_from_scenario(scenarios.grid_map(B, 'mixed').with_ues(num_slow=U))
    env = BatchedMobileEnv(m, bs, ues, kind, num_envs=E, seed=42, episode_length=100, rng='philox', rand_episodes=True, device=dev)
    if w == 'update_per_ue':
        actor = PerUEActor.random(U, B, hidden=H, seed=3, bias_std=0.1, device=dev)
        mb = E * T // 4                                    # per policy: E x T rows
        learner, kw = PerUELearner(actor, lr=1e-5, max_rows=mb), {'grouped': True}
    else:
        actor = FcnetActor(kind, U, B, FcnetActor.random_weights(kind, U, B, H, seed=1, bias_std=0.1), device=dev,
                           value_weights=FcnetActor.random_value_weights(kind, U, B, H, seed=1, bias_std=0.1))
        mb = E * T * (U if kind == 'multi' else 1) // 4
        learner, kw = PPOLearner(actor, lr=1e-5, max_rows=mb), {}
    batch = collect(env, actor, T, gamma=0.99, lam=0.95, compact=compact, dist_inputs=True)
    ms = []
    for i in range(2 + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        learner.update(batch, num_sgd_iter=4, minibatch_rows=mb, seed=1, **kw)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms[2:])


def measure_env_step(torch, dev, w, calls=2000):
    """BatchedMobileEnv.step() at 64 x 32 x 10 multi, host-bound: wall clock per call in ms over `calls` calls (a reset() every 100, the
    episode length, timed with them) after 100 warm-up calls, one synchronise at the end."""
    import time
    from deepcomp_amd import scenarios
    from deepcomp_amd.entities import build_from_scenario
    from deepcomp_amd.env import BatchedMobileEnv
    m, bs, ues = build_from_scenario(scenarios.grid_map(10, 'mixed').with_ues(num_slow=32))
    env = BatchedMobileEnv(m, bs, ues, 'multi', num_envs=64, seed=42, episode_length=100, device=dev, **ENV_STEPS[w])
    g = torch.Generator(device=dev).manual_seed(7)
    pool = torch.randint(0, 11, (4, 64, env.U), generator=g, device=dev, dtype=torch.uint8)
    for timed in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(calls if timed else 100):
            if i % 100 == 0:
                env.reset()
            env.step(pool[i & 3])
        torch.cuda.synchronize()
    env.check()
    return (time.perf_counter() - t0) * 1e3 / calls


def measure(a):
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    sys.path.insert(0, REPO)
    if os.environ.get('DCOMP_AB_PYTREE'):                  # (a `py:TREE` tag: that checkout's deepcomp_amd, this tree's bench and library)
        sys.path.insert(0, os.environ['DCOMP_AB_PYTREE'])
    import torch
    import bench
    from deepcomp_amd import scenarios
    from deepcomp_amd.entities import build_from_scenario
    from deepcomp_amd.env import BatchedMobileEnv
    dev = torch.device('cuda', 0)
    mk = (torch, BatchedMobileEnv, scenarios, build_from_scenario, dev)
    only = a.only.split(',') if a.only else WORKLOADS
    out = {}
    for w in only:
        if w == 'big64':                               # the generic kernel (dcomp_big.h): 8 192 x 32 x 64 multi / 65 536 x 10 x 40 central
            out[w] = bench.measure_steps(*mk, 8192, 32, 64, 'multi')['kernel_ms']
        elif w == 'big40c':
            out[w] = bench.measure_steps(*mk, 65536, 10, 40, 'central')['kernel_ms']
        elif w == 'c3':
            out[w] = bench.measure_steps(*mk, 65536, 32, 10, 'multi')['kernel_ms']
        elif w == 'c3rf':
            out[w] = bench.measure_steps(*mk, 65536, 32, 10, 'multi', sharing='resource-fair')['kernel_ms']
        elif w == 'c5':
            out[w] = bench.measure_steps(*mk, 4096, 128, 32, 'multi')['kernel_ms']
        elif w == 'c5big':
            out[w] = bench.measure_steps(*mk, 32768, 128, 32, 'multi', steps=100)['kernel_ms']
        elif w == 'c5mid':
            out[w] = bench.measure_steps(*mk, 8192, 128, 32, 'multi', steps=200)['kernel_ms']
        elif w == 'c4big':
            out[w] = bench.measure_steps(*mk, 262144, 32, 10, 'multi', steps=200)['kernel_ms']
        elif w == 'c4share':
            out[w] = bench.measure_steps(*mk, 32768, 32, 10, 'multi')['kernel_ms']
        elif w == 'central10x5':
            out[w] = bench.measure_steps(*mk, 65536, 10, 5, 'central')['kernel_ms']
        elif w == 'central32x10':
            out[w] = bench.measure_steps(*mk, 65536, 32, 10, 'central')['kernel_ms']
        elif w == 'learner_c3':                    # profiles/r09_learner.txt: one minibatch of 65 536 x 32 rows, multi
            out[w] = measure_learner(torch, dev, 'multi', 65536, 32, 10, 10)
        elif w == 'learner_c2':                    # ... and of 4 096 central rows
            out[w] = measure_learner(torch, dev, 'central', 4096, 10, 5, 200)
        elif w == 'actor_c3':
            out[w] = measure_actor(torch, dev, 'multi', 65536, 32, 10, 50)
        elif w == 'actor_c2':
            out[w] = measure_actor(torch, dev, 'central', 4096, 10, 5, 500)
        elif w in UPDATES:
            out[w] = measure_update(torch, dev, w)
        elif w in ENV_STEPS:
            out[w] = measure_env_step(torch, dev, w)
        elif w in COMPAT:
            import compat_rate
            out[w] = compat_rate.loop(COMPAT[w]) * 1e3
        elif w in ('central10x5f', 'c3roll'):      # the fused rollout kernel forced onto a big batch, ONE step per launch
            os.environ['DCOMP_FUSE_MAX_WAVES'] = '100000000'
            E, U, B, kind = (65536, 10, 5, 'central') if w == 'central10x5f' else (65536, 32, 10, 'multi')
            scn = scenarios.grid_map(B, 'mixed').with_ues(num_slow=U)
            m, bs, ues = build_from_scenario(scn)
            env = BatchedMobileEnv(m, bs, ues, kind, num_envs=E, seed=42, episode_length=100, rng='philox', rand_episodes=True, device=dev)
            del os.environ['DCOMP_FUSE_MAX_WAVES']
            assert env.fused_rollout
            g = torch.Generator(device=dev).manual_seed(7)
            pool = torch.randint(0, B + 1, (4, 1, E, U), generator=g, device=dev, dtype=torch.uint8)
            env.reset()
            for i in range(300):
                env.rollout(pool[i & 3])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(300):
                env.rollout(pool[i & 3])
            e1.record()
            torch.cuda.synchronize()
            env.check()
            out[w] = e0.elapsed_time(e1) / 300
        elif w == 'central10x5roll':     # the 65 536-env central batch through rollout(T = 50): fused at any batch size
            out[w] = bench.measure_rollout(*mk, 65536, 10, 5, 'central', T=50, steps=1500)['ms_per_step']
        elif w == 'c2roll':
            out[w] = bench.measure_rollout(*mk, 4096, 10, 5, 'central', T=100, steps=6000)['ms_per_step']
        elif w == 'c2policy':
            scn = scenarios.grid_map(5, 'mixed').with_ues(num_slow=10)
            m, bs, ues = build_from_scenario(scn)
            env = BatchedMobileEnv(m, bs, ues, 'central', num_envs=4096, seed=42, episode_length=100, rng='philox', rand_episodes=True, device=dev)
            env.set_policy('3gpp')
            env.reset()
            env.rollout_policy(300, horizon=100)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            env.rollout_policy(3000, horizon=100)
            e1.record()
            torch.cuda.synchronize()
            env.check()
            out[w] = e0.elapsed_time(e1) / 3000
    print('AB_RESULT ' + json.dumps(out), flush=True)


def run(a):
    res = {t: {} for t in a.tags}
    for r in range(a.rounds):
        for t in a.tags:
            lib = os.path.join(VAR, f'libdcomp_hip_{t}.so') if t != 'tree' and not t.startswith('py:') else os.path.join(CSRC, 'libdcomp_hip.so')
            env = dict(os.environ, DCOMP_LIB=lib, DCOMP_AB_NO_BUILD='1', DCOMP_AB_PYTREE=os.path.abspath(t[3:]) if t.startswith('py:') else '')
            p = subprocess.run([sys.executable, os.path.abspath(__file__), 'measure'] + (['--only', a.only] if a.only else []), env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = [l for l in p.stdout.splitlines() if l.startswith('AB_RESULT ')]
            if not line:
                print(t, 'FAILED', p.stdout[-1500:], flush=True)
                sys.exit(1)                                # (a child that died may have left the device in a bad state: start no more)
            for k, v in json.loads(line[-1][10:]).items():
                res[t].setdefault(k, []).append(v)
            print(f'round {r} {t}: ' + '  '.join(f'{k} {v * 1e3:.2f}us' for k, v in json.loads(line[-1][10:]).items()), flush=True)
    ref = a.tags[0]
    print(f'\n{"workload":14s}' + ''.join(f'{t:>22s}' for t in a.tags))
    for w in WORKLOADS + WALL:
        if w not in res[ref]:
            continue
        base = min(res[ref][w])
        row = f'{w:14s}'
        for t in a.tags:
            if w in res[t]:
                v = min(res[t][w])
                row += f'{v * 1e3:12.2f} us {v / base:6.3f}x'
            else:
                row += f'{"-":>22s}'
        print(row)
    import statistics
    wall = [w for w in WALL if w in res[ref]]
    if wall:
        print(f'\nwall clock, median of {a.rounds} rounds (max - min), us')
    for w in wall:
        print(f'{w:20s}' + ''.join(f'{t}: {statistics.median(res[t][w]) * 1e3:10.2f} ({(max(res[t][w]) - min(res[t][w])) * 1e3:8.2f})   ' for t in a.tags if w in res[t]))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='cmd', required=True)
    b = sub.add_parser('build'); b.add_argument('tag'); b.add_argument('--ref', default=''); b.add_argument('--b', default='5,10,32'); b.add_argument('--flags', default=''); b.add_argument('--src', default='', help='a copy of the tree (with deepcomp_amd/csrc and include) to build instead of the working tree: experiments that leave the product sources alone')
    r = sub.add_parser('run'); r.add_argument('tags', nargs='+'); r.add_argument('--rounds', type=int, default=2); r.add_argument('--only', default='')
    m = sub.add_parser('measure'); m.add_argument('--only', default='')
    a = ap.parse_args()
    {'build': build, 'run': run, 'measure': measure}[a.cmd](a)
