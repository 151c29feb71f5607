#!/usr/bin/env python3
"""dcomp_gae_uid (include/dcomp_gae_uid.h) next to dcomp_gae on the same static trace: every row of uid / uid_next holds 1 ... U, so both
compute the same advantages (checked here, bit for bit) and the difference is what following the words costs -- two more 2-byte loads
and one more 1-byte store per element, and the per-step look-up of the word and fetch of the carry.

    python tools/gae_uid_bench.py [--steps 50] [--envs 65536] [--slots 16] [--launches 40] [--rounds 5]

HIP events over back-to-back launches in steady state, the variants interleaved round by round; prints per variant the median and the range
of the time per launch, the bytes the algorithm moves (16 B per element for dcomp_gae: two loads, two stores of 4 B; 21 B for dcomp_gae_uid)
and the rate that gives.  max_shift = 0 is what collect(by_ue=True) passes on a static env, 2 stands for a schedule with two departures in
one step, -1 searches the whole prefix.
"""
import argparse
import statistics
import sys

sys.path.insert(0, '.')
import torch

from deepcomp_amd.sampler import gae, gae_uid

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=50)
ap.add_argument('--envs', type=int, default=65536)
ap.add_argument('--slots', type=int, default=16)
ap.add_argument('--launches', type=int, default=40, help='back-to-back launches per timing')
ap.add_argument('--rounds', type=int, default=5)
a = ap.parse_args()

T, E, U = a.steps, a.envs, a.slots
dev = torch.device('cuda', 0)
g = torch.Generator(device=dev)
g.manual_seed(0)
reward = torch.rand((T, E, U), generator=g, device=dev) * 2 - 1
vf = torch.randn((T, E, U), generator=g, device=dev)
last_vf = torch.randn((E, U), generator=g, device=dev)
end = torch.zeros(T, dtype=torch.uint8, device=dev)
end[T // 2] = 1
uid = torch.arange(1, U + 1, dtype=torch.int16, device=dev).expand(T, E, U).contiguous()
uid_next = uid.clone()
out2 = (torch.empty_like(reward), torch.empty_like(reward))
out3 = (torch.empty_like(reward), torch.empty_like(reward), torch.empty((T, E, U), dtype=torch.uint8, device=dev))

variants = [('dcomp_gae', 16, lambda: gae(reward, vf, last_vf, end, 0.99, 0.95, out=out2))]
for shift in (0, 2, -1):
    variants.append((f'dcomp_gae_uid max_shift {shift}', 21,
                     lambda shift=shift: gae_uid(reward, vf, uid, uid_next, last_vf, end, 0.99, 0.95, max_shift=shift, out=out3)))

for name, _, fn in variants:                       # warm-up, and the same bits
    fn()
    torch.cuda.synchronize()
    if name != 'dcomp_gae':
        assert torch.equal(out3[0].view(torch.int32), out2[0].view(torch.int32)) and torch.equal(out3[1].view(torch.int32), out2[1].view(torch.int32)), name
        assert bool(out3[2].all())
        out3[0].zero_()
        out3[1].zero_()

times = {name: [] for name, _, _ in variants}
for _ in range(a.rounds):
    for name, _, fn in variants:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        start.record()
        for _ in range(a.launches):
            fn()
        stop.record()
        torch.cuda.synchronize()
        times[name].append(start.elapsed_time(stop) * 1e3 / a.launches)

n = T * E * U
print(f'static trace [{T}, {E} x {U}] = {n} elements, {a.launches} back-to-back launches per timing, {a.rounds} rounds interleaved; outputs equal bit for bit')
base = statistics.median(times['dcomp_gae'])
for name, nbytes, _ in variants:
    ts = times[name]
    med = statistics.median(ts)
    print(f'{name:<28}: median {med:8.1f} us  (min {min(ts):8.1f}, max {max(ts):8.1f})  {nbytes} B/element -> {n * nbytes / med * 1e-3:7.1f} GB/s  {med / base:5.2f} x dcomp_gae')
