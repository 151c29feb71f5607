"""GPU characterization of PPO's SGD phase (PPOLearner.update, PerUELearner.update, run_lockstep over DataParallelLearner.update_phases).

The other learner tests hold the variants to EACH OTHER (grouped = sequential, micro-batches = whole, compact = rows = gathered loop);
a change that moved all of them together would pass them.  This module holds every variant to a RECORDING of itself,
tests/golden/sgd_characterization.json, written by this module's own entry at the commit that added it:

    python -m tests.<this module> --write            (on an MI355X, from the repository root)

Per scenario the recording holds (1) the library calls the update makes, in order, through a forwarding proxy around the ``_L`` the
learners hold: the entry point, the ``rows`` of its batch struct, ``source_rows`` and whether an index was given for the indexed and
grouped structs, the ``rows[p]`` array of dcomp_learner_group_grads; (2) the returned statistics as float.hex(); (3) the sha256 of
every learner's state afterwards (master weights, Adam's m and v in ARRAYS order, step, kl_coeff); (4) the sha256 of the input batch
and of the first permutation, so that a mismatch on a moved environment (another torch build, another device) says so instead of
blaming the code.  Every comparison is exact.

Shapes are the smallest at which each path can go wrong: hidden 32, num_sgd_iter 2, minibatches that leave a ragged last one."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from tests import fcnet_cases as fc
from tests import fcnet_support as fs
from tests.fcnet_support import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sgd_characterization.json')
ITERS = 2
MULTI = ('multi', 8, 3, 4, 32, 4)                # (kind, E, U, B, hidden, T): 96 source rows
CENTRAL = ('central', 16, 3, 4, 32, 4)           # 64 source rows
SLOTS = [0, 0, 1]                                # two policies: 64 and 32 rows


# ---------------------------------------------------------------------------------------------- the recording
class _Recorder:
    """Forwards every attribute to the library; while `log` is a list, every call through it is described there first."""

    def __init__(self, lib, policies=1):
        self._lib, self._policies, self.log = lib, policies, None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if self.log is None:
            return fn

        def call(*args):
            self.log.append(self._describe(name, args))
            return fn(*args)
        return call

    def _describe(self, name, args):
        from deepcomp_amd import _lib
        d = {'call': name}
        for a in args:
            b = getattr(a, '_obj', None)                                               # (ctypes.byref(struct))
            if isinstance(b, _lib.DcompPpoBatch):
                d['rows'] = int(b.rows)
            elif isinstance(b, _lib.DcompSgdBatch):
                d.update(rows=int(b.rows), source_rows=int(b.source_rows), index=bool(b.index))
            elif isinstance(b, _lib.DcompGroupBatch):
                d.update(rows=[int(b.rows[p]) for p in range(self._policies)], source_rows=int(b.source_rows), index=bool(b.index))
        return d


def _sha(*chunks):
    h = hashlib.sha256()
    for c in chunks:
        h.update(c)
    return h.hexdigest()


def _state_sha(learner):
    from deepcomp_amd.learner import ARRAYS
    s = learner.state_dict()
    return _sha(*[np.ascontiguousarray(s[k][n], dtype=np.float32).tobytes() for k in ('weights', 'm', 'v') for n in ARRAYS],
                f"{int(s['step'])} {float(s['kl_coeff']).hex()}".encode())


def _batch_sha(batches):
    """Over the tensors update() reads (the others may hold whatever their buffers were allocated with)."""
    keys = ('obs', 'obs_compact', 'actions', 'action_logp', 'action_dist_inputs', 'advantages', 'value_targets', 'vf_preds')
    return _sha(*[b[k].contiguous().cpu().numpy().tobytes() for b in batches for k in keys if k in b])


def _perm_sha(torch, n, seed):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed)
    return _sha(torch.randperm(n, generator=gen, device='cuda').cpu().numpy().tobytes())


def _hex(out):
    return None if out is None else {k: float(v).hex() for k, v in sorted(out.items())}


def _record(torch, learners, batches, seed, holders, run):
    """Run `run()` with a recording proxy in every holder's ``_L``; the scenario's record."""
    rec = _Recorder(holders[0]._L, policies=len(learners))
    for h in holders:
        h._L = rec
    rec.log = []
    outs = run()
    calls, rec.log = rec.log, None
    outs = outs if isinstance(outs, list) else [outs]
    n = int(batches[0]['actions'].numel() // learners[0].actor.heads)
    return {'calls': calls, 'stats': [_hex(o) for o in outs], 'state': [_state_sha(ln) for ln in learners],
            'inputs': _batch_sha(batches), 'perm': _perm_sha(torch, n, seed)}


# ---------------------------------------------------------------------------------------------- the scenarios
def _single(shape, compact, max_rows, **kw):
    """PPOLearner.update(batch, **kw) on the shape's collect() batch by a learner on the weights the batch was collected with."""
    def scenario(torch):
        kind, E, U, B, H, T = shape
        w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, compact)
        ln = fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=max_rows, perturb=False, lr=1e-3)
        args = dict(kw)
        if args.pop('half', False):                                                    # rows=: a shuffled half of the source rows
            n = int(batch['actions'].numel())
            gen = torch.Generator(device='cuda')
            gen.manual_seed(11)
            args.update(rows=torch.randperm(n, generator=gen, device='cuda')[:n // 2].contiguous(), check_rows=True)
        return _record(torch, [ln], [batch], args['seed'], [ln], lambda: ln.update(batch, num_sgd_iter=ITERS, **args))
    return scenario


def _per_ue(compact, grouped):
    def scenario(torch):
        kind, E, U, B, H, T = MULTI
        batch = fs.group_collected(('characterization', compact), U, B, H, 'tanh', E, T, SLOTS, compact)
        ln = fs.per_ue_learner(fs.policy_set(U, B, H, 'tanh', SLOTS), max_rows=32)
        return _record(torch, ln.learners, [batch], 6, [ln.actor] + ln.learners,
                       lambda: ln.update(batch, num_sgd_iter=ITERS, minibatch_rows=24, seed=6, grouped=grouped))
    return scenario


def _lockstep(compact):
    def scenario(torch):
        from deepcomp_amd.dp_learner import DataParallelLearner, run_lockstep
        kind, E, U, B, H, T = MULTI
        w, vw, batch = fs.collected(torch, kind, E, U, B, H, 'tanh', T, compact)
        shards = [fs.shard(batch, r, 2, E, U, T) for r in range(2)]
        lns = [fs.ppo_learner(kind, U, B, w, vw, 'tanh', max_rows=24, perturb=False, lr=1e-3) for _ in range(2)]
        dps = [DataParallelLearner(ln, rank=r, world=2) for r, ln in enumerate(lns)]
        return _record(torch, lns, shards, 8, lns, lambda: run_lockstep(dps, shards, num_sgd_iter=ITERS, minibatch_rows=48, seed=8))
    return scenario


SCENARIOS = {}
for _c in (False, True):
    _f = 'compact' if _c else 'rows'
    # 96 rows in minibatches of 40: two full ones and a ragged one of 16
    SCENARIOS[f'multi-{_f}-direct'] = _single(MULTI, _c, 40, minibatch_rows=40, seed=3)
    SCENARIOS[f'multi-{_f}-num_active'] = _single(MULTI, _c, 40, minibatch_rows=40, seed=4, num_active=2)
    SCENARIOS[f'multi-{_f}-rows'] = _single(MULTI, _c, 40, minibatch_rows=40, seed=5, half=True)
    # test_update_with_micro_rows_equals_update's shape: 6 464 rows in minibatches of 4 096 = 2 048 + 2 048, then 2 368 = 2 048 + 320
    SCENARIOS[f'accum-{_f}-micro'] = _single(fc.ACCUM_MULTI, _c, fc.CHUNK, minibatch_rows=4096, seed=3, micro_rows=fc.CHUNK)
    SCENARIOS[f'accum-{_f}-micro-clip'] = _single(fc.ACCUM_MULTI, _c, fc.CHUNK, minibatch_rows=4096, seed=3, micro_rows=fc.CHUNK, grad_clip=0.01)
    SCENARIOS[f'accum-{_f}-clip-alone'] = _single(fc.ACCUM_MULTI, _c, 4096, minibatch_rows=4096, seed=3, grad_clip=0.01)
    for _g in (False, True):
        SCENARIOS[f"per-ue-{_f}-{'grouped' if _g else 'sequential'}"] = _per_ue(_c, _g)
    SCENARIOS[f'lockstep-{_f}'] = _lockstep(_c)
# central: unlisted heads are left out by the kernel (kernel_active), 64 rows in minibatches of 24
SCENARIOS['central-rows-num_active'] = _single(CENTRAL, False, 24, minibatch_rows=24, seed=7, num_active=2)


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_scenarios():
    assert sorted(_fixture()) == sorted(SCENARIOS)


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_update_does_what_the_recording_did(torch_cuda, name):
    from deepcomp_amd.learner import chunk_unit
    assert fc.CHUNK == chunk_unit()                                                  # (the accumulated scenarios' micro_rows)
    got, want = SCENARIOS[name](torch_cuda), _fixture()[name]
    if got == want:
        return
    differ = [k for k in want if got[k] != want[k]]
    if 'inputs' in differ or 'perm' in differ:
        pytest.fail(f"{name}: the environment moved, not (only) the code -- the input batch or the first permutation is not the recorded one "
                    f"(another torch build or device?); differing: {differ}")
    first = next((i for i, (g, w) in enumerate(zip(got['calls'], want['calls'])) if g != w), None)
    detail = '' if 'calls' not in differ else \
        f"; {len(got['calls'])} library calls against {len(want['calls'])} recorded, the first that differs: #{first} " \
        f"{got['calls'][first] if first is not None else None} against {want['calls'][first] if first is not None else None}"
    pytest.fail(f"{name}: on the recorded inputs the update no longer does what it did; differing: {differ}{detail}")


if __name__ == '__main__':
    if sys.argv[1:] != ['--write']:
        sys.exit(__doc__)
    import torch as _torch
    assert _torch.cuda.is_available(), "recording needs the MI355X"
    _recorded = {name: SCENARIOS[name](_torch) for name in sorted(SCENARIOS)}
    with open(FIXTURE, 'w') as f:
        json.dump(_recorded, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', FIXTURE, sum(len(r['calls']) for r in _recorded.values()), 'library calls in', len(_recorded), 'scenarios')
