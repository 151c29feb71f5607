"""GPU characterization of BatchedMobileEnv's host side (deepcomp_amd/env.py, rng.py, tape.py) and of the reference-named classes.

The golden fixtures (reseed_*, dyn_*, reseeddyn_*, traj_*) hold the env to the REFERENCE where the reference was run.  This module holds
it to a RECORDING of itself, tests/golden/env_characterization.json, on the host sequences those fixtures do not walk: a tape extended
after a splice, rollouts cut into stretches after a splice, the order of the library calls.  Written by this module's own entry with
env.py and rng.py as they stood before the draw tape got one owner (the parent commit's):

    python -m tests.<this module> --write            (on an MI355X, from the repository root)

Per public call of a script the recording holds (1) the library calls it makes, in order, through a forwarding proxy around the ``_L``
the env holds: the entry point; for dcomp_reset whether a tape was given and its num_ids, for dcomp_set_tape the depth, for both the
sha256 of the two device tensors under ``env._tape_dev``; for dcomp_step_dyn n_remove / n_add and whether the two pointers are set; for
dcomp_rollout_ex T, the four scalar options, the ev_n_remove / ev_n_add host arrays and whether ev_remove_idx / ev_add_xy are set; the
argument of dcomp_set_seed / dcomp_set_episode; whether dcomp_set_policy got a policy and a buffer; (2) afterwards time, episode, num_ue,
tape_depth, the sha256 of every state tensor that exists, of ``_outbuf`` or of the `out` buffers handed in, and of every array of
state_host().  The scripts of the reference-named classes record repr() of everything reset() / step() return and the ids of ue_list.
(3) the sha256 of the action tapes (numpy's PCG64), so that a mismatch on a moved environment says so instead of blaming the code.
Every comparison is exact.  The fixture keeps one line per public call (_compact): the call, its library calls in brief and time / episode
/ num_ue / tape_depth afterwards in clear, and one sha256 over (1), (2) and what the call returned, in full; a mismatch prints the full
record of the call as it is now.

Shapes are the smallest at which each path can go wrong: the medium map (3 stations) with 3 slow UEs, E = 2, episode_length 8,
tape_depth 2 (outgrown within a few steps), UE 1 with pause_duration 0 (it may redraw every step, so the tape is sized for that), and in
the arrival scenarios UE 2 with the fixed velocity 2.5 (a number the movement word cannot hold: _vel_host)."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'env_characterization.json')
E, L, DEPTH = 2, 8, 2
STATE = ('pos', 'mv', 'conn', 'conn_hi', 'ewma', 'uid', 'orig_consumed')
OUT_KEYS = ('obs', 'reward', 'sum_utility', 'ue_dr', 'ue_utility')
ARRIVAL = {1: 1, 3: -1, 5: 2}


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _sha(*chunks):
    h = hashlib.sha256()
    for c in chunks:
        h.update(c)
    return h.hexdigest()


def _tsha(t):
    return _sha(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())


# ---------------------------------------------------------------------------------------------- the recording
class _Recorder:
    """Forwards every attribute to the library; while `log` is a list, every call through it is described there first."""

    def __init__(self, lib, env):
        self._lib, self._env, self.log = lib, env, None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if self.log is None:
            return fn

        def call(*args):
            self.log.append(self._describe(name, args))
            return fn(*args)
        return call

    def _tape(self):
        dev = self._env._tape_dev
        return None if dev is None else [_tsha(dev[0]), _tsha(dev[1])]

    def _describe(self, name, args):
        from deepcomp_amd import _lib
        d = {'call': name}
        obj = [getattr(a, '_obj', None) for a in args]                                 # (ctypes.byref(struct))
        if name == 'dcomp_reset':
            d.update(tape=obj[2] is not None, num_ids=None if obj[2] is None else int(obj[2].num_ids), tape_dev=self._tape())
        elif name == 'dcomp_set_tape':
            d.update(depth=int(args[2]), num_ids=int(obj[1].num_ids), tape_dev=self._tape())
        elif name == 'dcomp_step_dyn':
            ev = obj[4]
            d.update(n_remove=int(ev.n_remove), n_add=int(ev.n_add), remove_idx=bool(ev.remove_idx), add_xy=bool(ev.add_xy))
        elif name == 'dcomp_rollout_ex':
            T, o = int(args[3]), obj[5]
            d.update(T=T, every_step=int(o.every_step), horizon=int(o.horizon), new_episode_draws=int(o.new_episode_draws),
                     policy_loop=int(o.policy_loop), ev_remove_idx=bool(o.ev_remove_idx), ev_add_xy=bool(o.ev_add_xy))
            for k in ('ev_n_remove', 'ev_n_add'):
                p = getattr(o, k)
                d[k] = list((ctypes.c_int32 * T).from_address(p)) if p else None
        elif name == 'dcomp_set_seed':
            d['seed'] = int(args[1].value)
        elif name == 'dcomp_set_episode':
            d['episode'] = int(args[1])
        elif name == 'dcomp_set_policy':
            d.update(policy=args[1] is not None, buffer=args[2] is not None)
        elif name == 'dcomp_heuristic_actions':
            assert isinstance(obj[0], _lib.DcompPolicy)
            d.update(policy=int(obj[0].policy), num_active=int(obj[0].num_active), epsilon=float(obj[0].epsilon).hex(),
                     cluster_mask=bool(obj[0].cluster_mask))
        return d


def _snapshot(torch, env, out=None):
    """What a public call left behind (taken with the recording paused)."""
    torch.cuda.synchronize()
    d = {'time': int(env.time), 'episode': int(env.episode), 'num_ue': int(env.num_ue), 'tape_depth': int(env.tape_depth),
         'seed_value': int(env.seed_value), 'env_seeds': [int(s) for s in env.env_seeds],
         'state': {k: _tsha(getattr(env, k)) for k in STATE if getattr(env, k) is not None},
         'out': _tsha(env._outbuf) if out is None else {k: _tsha(v) for k, v in sorted(out.items())},
         'state_host': {k: _sha(np.ascontiguousarray(v).tobytes()) for k, v in sorted(env.state_host().items())}}
    return d


class _Script:
    """Runs public calls on `env` with a recording proxy in the ``_L`` of `core` (the BatchedMobileEnv underneath)."""

    def __init__(self, torch, env, core=None):
        self.torch, self.env, self.core = torch, env, env if core is None else core
        self.rec = _Recorder(self.core._L, self.core)
        self.core._L = self.rec
        self.steps, self.tapes = [], []

    def do(self, label, fn, out=None, extra=None, refused=False):
        self.rec.log = []
        err, ret = None, None
        try:
            ret = fn()
            assert not refused, f"{label} was expected to raise ValueError"
        except ValueError as e:                                                        # (the refusals of the Philox script: text recorded)
            if not refused:
                raise
            err = str(e)
        calls, self.rec.log = self.rec.log, None
        step = {'do': label, 'calls': calls, 'after': _snapshot(self.torch, self.core, out)}
        if err is not None:
            step['error'] = err
        if extra is not None:
            step['returned'] = extra(ret)
        self.steps.append(step)
        return ret

    def actions(self, seed, *shape):
        """A uint8 action tape (values 0 .. B) on the device; its sha256 goes into the record."""
        a = np.random.default_rng(seed).integers(0, self.core.B + 1, size=shape).astype(np.uint8)
        self.tapes.append(_sha(a.tobytes()))
        return self.torch.from_numpy(a).to(self.core.device)

    def steps_(self, n, seed):
        for t, a in enumerate(self.actions(seed, n, self.core.E, self.core.U)):
            self.do(f'step[{seed}:{t}]', lambda a=a: self.env.step(a))

    def out(self, T):
        c, z = self.core, self.torch.zeros
        return {'obs': z((T,) + tuple(c.obs.shape), dtype=self.torch.float32, device=c.device),
                'reward': z((T,) + tuple(c.reward.shape), dtype=self.torch.float32, device=c.device),
                'sum_utility': z((T, c.E), dtype=self.torch.float32, device=c.device),
                'ue_dr': z((T, c.E, c.U), dtype=self.torch.float32, device=c.device),
                'ue_utility': z((T, c.E, c.U), dtype=self.torch.float32, device=c.device)}

    def rollout(self, T, seed, with_out, horizon=L):
        out = self.out(T) if with_out else None
        a = self.actions(seed, T, self.core.E, self.core.U)
        self.do(f"rollout(T={T}, horizon={horizon}{', out' if with_out else ''})", lambda: self.env.rollout(a, out=out, horizon=horizon), out=out)

    def record(self):
        return {'steps': self.steps, 'actions': self.tapes}


def _env(torch, rng='reference', fixed_velocity=False, **kw):
    from deepcomp_amd import scenarios
    from deepcomp_amd.entities import build_from_scenario
    from deepcomp_amd.env import BatchedMobileEnv
    return BatchedMobileEnv(*build_from_scenario(_scenario(scenarios, fixed_velocity)), 'multi', num_envs=E, episode_length=L,
                            rng=rng, device='cuda:0', tape_depth=DEPTH, **dict({'seed': 42}, **kw))


def _scenario(scenarios, fixed_velocity=False):
    scn = scenarios.medium_map('mixed').with_ues(num_slow=3)
    scn.ue_specs[0]['pause_duration'] = 0
    if fixed_velocity:
        scn.ue_specs[1]['velocity'] = 2.5
    return scn


# ---------------------------------------------------------------------------------------------- the scripts
def _fixed(torch):
    s = _Script(torch, _env(torch))
    s.do('reset', s.env.reset)
    s.steps_(5, 1)
    s.do('reset', s.env.reset)
    s.steps_(12, 2)                                                                    # the tape is extended
    s.do('reset', s.env.reset)                                                         # (the library refuses a horizon behind env.time)
    s.rollout(20, 3, False)
    s.rollout(20, 4, True)
    return s.record()


def _fixed_live(torch):
    s = _Script(torch, _env(torch))
    s.do('reset', s.env.reset)
    s.steps_(3, 1)
    s.do('seed(977, immediate)', lambda: s.env.seed(977, immediate=True))
    s.steps_(10, 2)                                                                    # extends a spliced tape
    s.rollout(12, 3, False)                                                            # cut into stretches because of the splice
    s.do('reset', s.env.reset)                                                         # back to the configured seed
    s.steps_(3, 4)
    s.do('seed(555, immediate)', lambda: s.env.seed(555, immediate=True))
    s.rollout(12, 5, True)                                                             # stretches that START on a spliced tape
    return s.record()


def _rand(torch):
    s = _Script(torch, _env(torch, rand_episodes=True))
    s.do('seed(311, immediate)', lambda: s.env.seed(311, immediate=True))              # before the first reset
    s.do('reset', s.env.reset)
    s.steps_(4, 1)
    s.do('reset', s.env.reset)                                                         # cursors are read back
    s.steps_(2, 2)
    s.do('seed(977, immediate)', lambda: s.env.seed(977, immediate=True))
    s.steps_(9, 3)
    s.do('reset', s.env.reset)
    s.rollout(19, 4, True)
    return s.record()


def _arrival(**kw):
    def script(torch):
        s = _Script(torch, _env(torch, fixed_velocity=True, **kw))
        s.do('reset', s.env.reset)
        s.steps_(4, 1)                                                                 # (both schedules: past the first arrival)
        s.do('seed(977, immediate)', lambda: s.env.seed(977, immediate=True))
        s.steps_(4, 2)                                                                 # across every event; the tape is extended
        s.do('reset', s.env.reset)                                                     # end_lists / consumed
        s.rollout(18, 3, True)
        s.do("set_policy('3gpp')", lambda: s.env.set_policy('3gpp'))
        s.do('reset', s.env.reset)
        out = s.out(18)
        s.do('rollout_policy(18, horizon=8, out)', lambda: s.env.rollout_policy(18, out=out, horizon=L), out=out)
        s.do('rollout_policy(5, horizon=8)', lambda: s.env.rollout_policy(5, horizon=L))
        return s.record()
    return script


def _philox(torch):
    s = _Script(torch, _env(torch, rng='philox'))
    s.do('seed(5)', lambda: s.env.seed(5))
    s.do('reset', s.env.reset)
    s.steps_(3, 1)
    s.rollout(10, 2, False)
    sd = s.do('state_dict', s.env.state_dict)
    s2 = _Script(torch, _env(torch, rng='philox', seed=5))                             # (a checkpoint names the seed its episode draws from)
    s2.do('seed(6)', lambda: s2.env.seed(6))                                           # staged here: not part of the checkpointed run
    s2.do('load_state_dict', lambda: s2.env.load_state_dict(sd))
    s2.steps_(2, 3)
    s2.do('reset', s2.env.reset)
    sha = lambda t: _tsha(t)                                                           # noqa: E731
    s.do("set_policy('dynamic', 0.5)", lambda: s.env.set_policy('dynamic', epsilon=0.5), extra=bool)
    s.do('reset', s.env.reset)
    s.do('step(next_action)', lambda: s.env.step(s.env.next_action))
    s.do('next_action', lambda: s.env.next_action, extra=sha)
    mask = torch.tensor([0b011, 0b011, 0b100], dtype=torch.int32, device=s.env.device)
    s.do("heuristic_actions('cluster', mask)", lambda: s.env.heuristic_actions('cluster', cluster_mask=mask), extra=sha)
    s.do("heuristic_actions('cluster')", lambda: s.env.heuristic_actions('cluster'), refused=True)
    s.do("heuristic_actions('nearest')", lambda: s.env.heuristic_actions('nearest'), refused=True)
    s.do("set_policy('cluster')", lambda: s.env.set_policy('cluster'), refused=True)
    s.do("set_policy('nearest')", lambda: s.env.set_policy('nearest'), refused=True)
    s.do("set_policy('cluster', mask)", lambda: s.env.set_policy('cluster', cluster_mask=mask), extra=bool)
    s.do('step(next_action)', lambda: s.env.step(s.env.next_action))
    s.do('set_policy(None)', lambda: s.env.set_policy(None), extra=bool)
    return {'steps': s.steps, 'restored': s2.steps, 'actions': s.tapes + s2.tapes}


def _named(cls_name, fixed_velocity=False, **kw):
    """reset, 10 steps with a seed() in the middle through a reference-named class at num_envs = 1 (rng='reference', pinned host I/O)."""
    def script(torch):
        from deepcomp_amd import env as env_mod, scenarios
        from deepcomp_amd.entities import make_env_config
        env = getattr(env_mod, cls_name)(make_env_config(_scenario(scenarios, fixed_velocity), seed=42, episode_length=L, **kw))
        s = _Script(torch, env, core=env.core)
        ids = lambda: [ue.id for ue in env.ue_list]                                    # noqa: E731
        s.do('reset', env.reset, extra=lambda r: {'returned': repr(r), 'ue_list': ids()})
        B = env.num_bs
        a = np.random.default_rng(7).integers(0, B + 1, size=(10, env.max_ues))
        s.tapes.append(_sha(a.astype(np.uint8).tobytes()))
        for t in range(10):
            if t == 4:
                s.do('seed(977)', lambda: env.seed(977))
            if cls_name == 'CentralRelNormEnv':
                act = [int(x) for x in a[t]]
            elif cls_name == 'MultiAgentMobileEnv':
                act = {ue.id: int(a[t, i]) for i, ue in enumerate(env.ue_list)}
            else:
                act = int(a[t, 0])
            s.do(f'step[{t}]', lambda: env.step(act), extra=lambda r: {'returned': repr(r), 'ue_list': ids()})
        return s.record()
    return script


SCENARIOS = {
    'fixed': _fixed,
    'fixed-live': _fixed_live,
    'rand': _rand,
    'arrival-fixed': _arrival(ue_arrival=ARRIVAL),
    'arrival-rand': _arrival(ue_arrival=ARRIVAL, rand_episodes=True),
    'arrival-interval': _arrival(new_ue_interval=3),
    'philox': _philox,
    'named-central': _named('CentralRelNormEnv'),
    'named-multi-arrival': _named('MultiAgentMobileEnv', fixed_velocity=True, ue_arrival=ARRIVAL),
    'named-single': _named('RelNormEnv'),
}


def _jsha(x):
    return _sha(json.dumps(x, sort_keys=True).encode())


def _brief(c):
    """A library call as the fixture shows it in clear: the entry point (without its dcomp_ prefix) and the one figure that says most."""
    n = c['call'][len('dcomp_'):]
    return {'set_tape': lambda: f"{n}({c['depth']})", 'step_dyn': lambda: f"{n}(-{c['n_remove']}+{c['n_add']})",
            'rollout_ex': lambda: f"{n}({c['T']})"}.get(n, lambda: n)()


def _compact(record):
    """What the fixture keeps of a script's record, one line per public call: the call, its library calls in brief, time / episode /
    num_ue / tape_depth afterwards -- in clear, for the reader -- and ONE sha256 over the full description of the library calls, the full
    snapshot afterwards and what the call returned, which is what holds the comparison exact."""
    out = {'actions': record['actions']}
    for key in (k for k in record if k != 'actions'):
        out[key] = []
        for s in record[key]:
            a = s['after']
            c = {'do': s['do'], 'calls': ' '.join(_brief(x) for x in s['calls']), 'at': [a['time'], a['episode'], a['num_ue'], a['tape_depth']],
                 'sha': _jsha([s['calls'], a, s.get('returned')])}
            if 'error' in s:
                c['error'] = s['error']
            out[key].append(c)
    return out


def _dump(recorded, f):
    """One line per public call."""
    rows = []
    for name in sorted(recorded):
        parts = [f' "actions": {json.dumps(recorded[name]["actions"])}']
        for key in sorted(k for k in recorded[name] if k != 'actions'):
            parts.append(f' "{key}": [\n' + ',\n'.join('  ' + json.dumps(s, sort_keys=True) for s in recorded[name][key]) + '\n ]')
        rows.append(f'"{name}": {{\n' + ',\n'.join(parts) + '\n}')
    f.write('{\n' + ',\n'.join(rows) + '\n}\n')


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_scenarios():
    assert sorted(_fixture()) == sorted(SCENARIOS)


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_env_does_what_the_recording_did(torch_cuda, name):
    full = SCENARIOS[name](torch_cuda)
    got, want = _compact(full), _fixture()[name]
    if got == want:
        return
    if got['actions'] != want['actions']:
        pytest.fail(f"{name}: the environment moved, not (only) the code -- the action tapes are not the recorded ones (another numpy?)")
    for key in sorted(k for k in want if k != 'actions'):
        assert [s['do'] for s in got[key]] == [s['do'] for s in want[key]], f"{name}: the script itself changed"
        for i, (g, w) in enumerate(zip(got[key], want[key])):
            if g == w:
                continue
            differ = sorted(k for k in set(g) | set(w) if g.get(k) != w.get(k))
            detail = f"; library calls now: {g['calls']!r}, recorded: {w['calls']!r}; afterwards (time, episode, num_ue, tape_depth) " \
                     f"{g['at']} against {w['at']}; in full, now: {json.dumps(full[key][i], sort_keys=True)}"
            pytest.fail(f"{name}: {key}[{i}] {w['do']} no longer does what it did; differing: {differ}{detail}")
    pytest.fail(f"{name}: differs from the recording")


if __name__ == '__main__':
    if sys.argv[1:] != ['--write']:
        sys.exit(__doc__)
    import torch as _torch
    assert _torch.cuda.is_available(), "recording needs the MI355X"
    _full = {name: SCENARIOS[name](_torch) for name in sorted(SCENARIOS)}
    with open(FIXTURE, 'w') as f:
        _dump({name: _compact(r) for name, r in _full.items()}, f)
    print('wrote', FIXTURE, sum(len(s['calls']) for r in _full.values() for k in r if k != 'actions' for s in r[k]),
          'library calls in', len(_full), 'scenarios')
