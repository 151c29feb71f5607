#!/usr/bin/env python3
"""Steps/s of the drop-in single-env classes (num_envs = 1, reference-shaped Python returns, one host round trip per
step) -- the mode an unmodified RLlib worker uses.  Compare BASELINE.md: reference env 69.9 steps/s at 32 x 10.
tools/ab/ab_lib.py times the same loops (compat_*) under the Python package of two checkouts."""
import random
import sys
import time

LOOPS = {'multi 32x10': ('MultiAgentMobileEnv', 10, 32), 'central 10x5': ('CentralRelNormEnv', 5, 10), 'central 3x3': ('CentralRelNormEnv', 0, 3)}


def loop(name, n=300):
    """Seconds per step of loop `name`: n steps with a reset every 100, after 20 warm-up steps."""
    from deepcomp_amd import env as env_mod, scenarios
    from deepcomp_amd.entities import make_env_config
    cls, B, U = LOOPS[name]
    multi = cls == 'MultiAgentMobileEnv'
    scn = (scenarios.grid_map(B, 'mixed') if B else scenarios.medium_map('mixed')).with_ues(num_slow=U)
    env = getattr(env_mod, cls)(make_env_config(scn, seed=42))
    rng = random.Random(1)
    U, B = env.num_ue, env.num_bs
    env.reset()
    acts = [({ue.id: rng.randint(0, B) for ue in env.ue_list} if multi else [rng.randint(0, B) for _ in range(U)]) for _ in range(n)]
    for a in acts[:20]:
        env.step(a)
    t0 = time.perf_counter()
    for i, a in enumerate(acts):
        if i % 100 == 0:
            env.reset()
        env.step(a)
    return (time.perf_counter() - t0) / n


if __name__ == '__main__':
    sys.path.insert(0, '.')
    for name in LOOPS:
        dt = loop(name)
        print(f'{name}: {1 / dt:.0f} env-steps/s ({dt * 1e3:.2f} ms per step, E = 1, PCIe round trip included)')
