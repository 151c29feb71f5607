#!/usr/bin/env python3
"""The per-UE policy set's launch (deepcomp_amd.policy_set.PerUEActor, include/dcomp_policy_set.h) on one GPU, next to what it replaces:

    python tools/policy_set_bench.py [--shapes 65536x32x10x256,4096x128x32x64,4096x128x32x256] [--launches 30] [--no-per-slot] [--out FILE]

Per shape E x U x B x hidden (multi-agent, tanh, value trunks of their own, P = U distinct random-init members; actions + logp + vf,
sampled, observation rows; synthetic observations: the time does not depend on the values), HIP events over back-to-back launches,
three interleaved timings each:
  (i)  the shared-policy launch (FcnetActor.actions of member 0) on the same batch: the floor
  the set's launch (dcomp_policy_set_actions_v)
  (ii) what per-UE networks cost without the set: per slot a strided copy of the slot's rows into E / U whole envs, the member's own
       launch, and three strided copies back (actions, logp, vf)
and one check that the set's outputs at slot 1 are its member's own, bit for bit.  profiles/r12_policy_set.txt sections 3 and 3b are
this output; DCOMP_LIB=<another build> times that library instead (a tools/ab/ab_lib.py variant, e.g. another tile order).

    python tools/policy_set_bench.py --by-id [--shapes 65536x32x10x256,4096x260x10x64] [--layouts static,dynamic] [--repeats 7] [--launches 30]

The set keyed by UE id (PerIdActor, include/dcomp_policy_set_uid.h) instead.  Per shape E x U x B x hidden, on real envs (reset and three
steps of random actions), actions + logp + vf, sampled, observation rows; each figure the MEDIAN of --repeats interleaved timings (at
least 5) with their spread:
  static   a static env of U UEs, P = U members: the launch by id (the words 1 ... U) against the slot-keyed launch of a PerUEActor over
           the SAME members on the same observations -- what the scan of the uid words and the slot read from LDS cost
  dynamic  an env with UE arrival and departure of the same U slots (U - 2 initial UEs, {1: 2, 2: -1, 3: -2, 5: 1}), P = env.max_id
           members: the launch by id against the shared-policy launch of member 0 on the same observations
and one check per layout that the launch by id writes its members' bits.  profiles/r23_policy_set_uid.txt is this output."""
import argparse
import sys

sys.path.insert(0, '.')
import torch

from deepcomp_amd.policy_set import PerIdActor, PerUEActor
from deepcomp_amd.tape import uid_fields

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', default='65536x32x10x256,4096x128x32x64,4096x128x32x256', help='comma-separated E x U x B x hidden; E must be a multiple of U')
ap.add_argument('--launches', type=int, default=30)
ap.add_argument('--no-per-slot', action='store_true', help='skip (ii)')
ap.add_argument('--out', default='', help='also write the lines to this file')
ap.add_argument('--by-id', action='store_true', help='the set keyed by UE id against the slot-keyed set (static env) and the shared policy (dynamic env)')
ap.add_argument('--layouts', default='static,dynamic', help='--by-id: which of the two comparisons')
ap.add_argument('--repeats', type=int, default=7, help='--by-id: interleaved timings per figure (at least 5)')
a = ap.parse_args()
dev = torch.device('cuda', 0)
log = open(a.out, 'w') if a.out else None


def say(line):
    print(line, flush=True)
    if log:
        log.write(line + '\n')
        log.flush()


def timed(fn, n):
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def by_id_env(E, U0, B, ue_arrival):
    from deepcomp_amd import scenarios
    from deepcomp_amd.entities import build_from_scenario
    from deepcomp_amd.env import BatchedMobileEnv
    m, bs, ues = build_from_scenario(scenarios.grid_map(B, 'mixed').with_ues(num_slow=U0))
    env = BatchedMobileEnv(m, bs, ues, 'multi', num_envs=E, seed=42, episode_length=100, rng='philox', rand_episodes=True, ue_arrival=ue_arrival, device=dev)
    env.reset()
    g = torch.Generator(device=dev).manual_seed(3)
    for _ in range(3):
        env.step(torch.randint(0, B + 1, (E, env.U), generator=g, device=dev, dtype=torch.uint8))
    return env


def by_id_lines(shape):
    E, U, B, H = (int(x) for x in shape.split('x'))
    repeats = max(5, a.repeats)
    for layout in a.layouts.split(','):
        env = by_id_env(E, U if layout == 'static' else U - 2, B, None if layout == 'static' else {1: 2, 2: -1, 3: -2, 5: 1})
        assert env.U == U
        members = PerIdActor._random_members(U, B, H, 'tanh', 0, 0.0, dev, env.max_id, True)
        by_id = PerIdActor(members)
        other = PerUEActor(members) if layout == 'static' else members[0]
        obs, uid, rows = env.obs, by_id.uid_of(env), E * U
        out = torch.zeros((E, U), dtype=torch.uint8, device=dev)
        logp, vf = torch.zeros((rows, 1), device=dev), torch.zeros(rows, device=dev)
        variants = [('by_id', 'dcomp_policy_set_actions_uid', lambda i: by_id.actions(obs, uid=uid, sample=True, seed=1, step=i, out=out, logp=logp, vf=vf)),
                    ('other', 'dcomp_policy_set_actions_v (slot-keyed, same members)' if layout == 'static' else 'dcomp_actor_actions_v (shared policy, member 0)',
                     lambda i: other.actions(obs, sample=True, seed=1, step=i, out=out, logp=logp, vf=vf))]
        res = {k: [] for k, _, _ in variants}
        for _ in range(repeats):
            for k, _, fn in variants:
                res[k].append(timed(fn, a.launches))
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        listed = int((uid != 0).sum())
        say(f'{layout}: {E} x {U} x {B} multi, 2x{H} tanh + value trunk, actions + logp + vf, sampled, rows obs; {env.max_id} members, '
            f'{listed} of {rows} slots listed; median of {repeats} x {a.launches} launches [min .. max]')
        for k, name, _ in variants:
            say(f'   {name:<56}: {med[k] * 1e3:9.1f} us  [{min(res[k]) * 1e3:.1f} .. {max(res[k]) * 1e3:.1f}]')
        say(f'   by id / {"slot-keyed" if layout == "static" else "shared"} = {med["by_id"] / med["other"]:.3f} x')
        got = torch.zeros_like(out), torch.zeros_like(logp), torch.zeros_like(vf)
        by_id.actions(obs, uid=uid, sample=True, seed=1, step=0, out=got[0], logp=got[1], vf=got[2])
        ids = uid_fields(uid.reshape(-1))[0]
        ue = int(ids[1])                                         # the UE at slot 1 of env 0: its member's own launch, at its rows
        members[ue - 1].actions(obs, sample=True, seed=1, step=0, out=out, logp=logp, vf=vf)
        at = torch.nonzero(ids == ue).reshape(-1)
        same = all(torch.equal(x.reshape(rows)[at], y.reshape(rows)[at]) for x, y in zip(got, (out, logp, vf)))
        say(f'   the rows of UE {ue} ({at.numel()}) equal its member\'s own launch: {bool(same)}')
        del by_id, other, members, env


if a.by_id:
    for shape in (a.shapes if a.shapes != ap.get_default('shapes') else '65536x32x10x256').split(','):
        by_id_lines(shape)
    if log:
        log.close()
    sys.exit(0)

for shape in a.shapes.split(','):
    E, U, B, H = (int(x) for x in shape.split('x'))
    if E % U:
        ap.error(f'{shape}: E must be a multiple of U (the rows of one slot are handed to a member as E / U whole envs)')
    pset = PerUEActor.random(U, B, hidden=H, seed=0, device=dev)
    shared = pset.members[0]
    rows, K = E * U, 4 * B + 1
    g = torch.Generator(device=dev).manual_seed(3)
    obs = torch.rand((E, U, K), generator=g, device=dev)
    out = torch.zeros((E, U), dtype=torch.uint8, device=dev)
    logp, vf = torch.zeros((rows, 1), device=dev), torch.zeros(rows, device=dev)
    g_obs = torch.zeros((E // U, U, K), device=dev)
    g_out = torch.zeros((E // U, U), dtype=torch.uint8, device=dev)
    g_logp, g_vf = torch.zeros((E, 1), device=dev), torch.zeros(E, device=dev)
    logp2, vf2 = logp.view(E, U), vf.view(E, U)

    def launch(actor):
        return lambda i: actor.actions(obs, sample=True, seed=1, step=i, out=out, logp=logp, vf=vf)

    def per_slot(i):
        for u in range(U):
            g_obs.view(E, K).copy_(obs[:, u])
            pset.members[u].actions(g_obs, sample=True, seed=1, step=i, out=g_out, logp=g_logp, vf=g_vf)
            out[:, u].copy_(g_out.view(E))
            logp2[:, u].copy_(g_logp.view(E))
            vf2[:, u].copy_(g_vf)

    variants = [('shared', '(i) shared-policy launch, dcomp_actor_actions_v', launch(shared), a.launches),
                ('set', 'dcomp_policy_set_actions_v', launch(pset), a.launches)]
    if not a.no_per_slot:
        variants.append(('per_slot', '(ii) per slot: gather, member launch, 3 scatters', per_slot, max(3, a.launches // 10)))
    res = {k: [] for k, _, _, _ in variants}
    for _ in range(3):                                   # interleaved: drift of the clocks shows as spread, not as a difference
        for k, _, fn, n in variants:
            res[k].append(timed(fn, n))
    say(f'{E} x {U} x {B} multi, 2x{H} tanh + value trunk, actions + logp + vf, sampled, rows obs; {U} distinct members')
    for k, name, _, _ in variants:
        say(f'   {name:<50}: ' + ' / '.join(f'{t * 1e3:.1f}' for t in res[k]) + ' us')
    best = {k: min(v) for k, v in res.items()}
    say(f'   set / shared = {best["set"] / best["shared"]:.3f} x' + ('' if a.no_per_slot else f'    per-slot / set = {best["per_slot"] / best["set"]:.2f} x'))
    want = torch.zeros_like(out), torch.zeros_like(logp), torch.zeros_like(vf)
    pset.actions(obs, sample=True, seed=1, step=0, out=out, logp=logp, vf=vf)
    pset.members[1 % U].actions(obs, sample=True, seed=1, step=0, out=want[0], logp=want[1], vf=want[2])
    s1 = 1 % U
    same = torch.equal(out[:, s1], want[0][:, s1]) and torch.equal(logp2[:, s1], want[1].view(E, U)[:, s1]) and torch.equal(vf2[:, s1], want[2].view(E, U)[:, s1])
    say(f'   slot {s1} equals its member: {bool(same)}')
    del pset, shared
if log:
    log.close()
