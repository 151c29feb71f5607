"""CPU-side checks of the value function and the advantage entry point (dcomp_actor_set_value / dcomp_actor_actions_v / dcomp_gae in
include/dcomp.h, deepcomp_amd/actor.py, deepcomp_amd/sampler.py): the symbols exist, arguments are refused on the host before the
first HIP call, the ctypes mirrors match the header, RLlib's value-branch names map onto the value arrays, and gae_reference is
RLlib's compute_advantages.  No GPU compute is called here.  The two refusals that need a live handle -- a handle without a value
function, a second dcomp_actor_set_value -- are in tests/test_critic_gpu.py: a handle cannot be created without a device."""
import ctypes
import re

import numpy as np
import pytest

from tests import c_surface as cs
from tests.c_surface import EABI, EINVAL, lib  # noqa: F401  (lib: the fixture)

NEW = ('dcomp_actor_set_value', 'dcomp_actor_actions_v', 'dcomp_gae')


def test_symbols_are_exported_and_declared(lib):
    from deepcomp_amd import _lib
    hdr = open(cs.header('dcomp.h')).read()
    for name in NEW:
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr)
        getattr(lib, name)
    assert len(_lib.EXPORTS) == 42 and len(set(_lib.EXPORTS)) == 42
    assert '#define DCOMP_ABI_VERSION 3' in hdr                          # the new structs carry their own size: no version bump


def _value_cfg(shared=0, size=None, null=(), H=64, nin=21, keep=None):
    from deepcomp_amd import _lib
    fp = ctypes.POINTER(ctypes.c_float)
    shapes = {'w1': (nin, H), 'b1': (H,), 'w2': (H, H), 'b2': (H,), 'wv': (H,), 'bv': (1,)}
    arrs = {n: np.zeros(s, dtype=np.float32) for n, s in shapes.items()}
    if keep is not None:
        keep.append(arrs)
    ptr = lambda n: None if n in null else arrs[n].ctypes.data_as(fp)      # noqa: E731
    return _lib.DcompActorValueCfg(ctypes.sizeof(_lib.DcompActorValueCfg) if size is None else size, shared,
                                   *[ptr(n) for n in ('w1', 'b1', 'w2', 'b2', 'wv', 'bv')])


TRUNK = ('w1', 'b1', 'w2', 'b2')


def test_set_value_refuses_bad_arguments_on_the_host(lib):
    """Every case fails validation before the handle is read (a fake one is never dereferenced) and before any HIP call."""
    from deepcomp_amd import _lib
    keep = []
    fake = ctypes.c_void_p(4096)
    assert lib.dcomp_actor_set_value(None, ctypes.byref(_value_cfg(keep=keep))) == EINVAL
    assert lib.dcomp_actor_set_value(fake, None) == EINVAL
    for size in (0, ctypes.sizeof(_lib.DcompActorValueCfg) - 8, ctypes.sizeof(_lib.DcompActorValueCfg) + 8):
        assert lib.dcomp_actor_set_value(fake, ctypes.byref(_value_cfg(size=size, keep=keep))) == EABI
        assert b'dcomp_actor_value_cfg' in lib.dcomp_last_error()
    cases = [(dict(shared=2), 'shared'), (dict(shared=-1), 'shared'),
             (dict(null=('wv',)), 'NULL'), (dict(null=('bv',)), 'NULL'), (dict(shared=1, null=TRUNK + ('bv',)), 'NULL'),
             (dict(shared=1), 'trunk'),                                  # a trunk given with shared
             (dict(shared=1, null=('w1', 'b1', 'w2')), 'trunk'),         # ... even a single pointer of it
             (dict(shared=0, null=('w2',)), 'NULL'), (dict(shared=0, null=TRUNK), 'NULL')]
    for kw, word in cases:
        rc = lib.dcomp_actor_set_value(fake, ctypes.byref(_value_cfg(keep=keep, **kw)))
        assert rc == EINVAL, (kw, rc, lib.dcomp_last_error())
        assert word.encode() in lib.dcomp_last_error(), (kw, lib.dcomp_last_error())


def test_actions_v_refuses_bad_arguments_on_the_host(lib):
    from deepcomp_amd import _lib
    fake = ctypes.c_void_p(4096)
    run = _lib.DcompActorRun(ctypes.sizeof(_lib.DcompActorRun), 0, 1, 1, 0, 0, 0, 0, None, None)
    assert lib.dcomp_actor_actions_v(None, ctypes.byref(run), fake, fake, fake, None) == EINVAL
    assert lib.dcomp_actor_actions_v(fake, None, fake, fake, fake, None) == EINVAL
    bad = _lib.DcompActorRun(ctypes.sizeof(_lib.DcompActorRun) + 8, 0, 1, 1, 0, 0, 0, 0, None, None)
    assert lib.dcomp_actor_actions_v(fake, ctypes.byref(bad), fake, fake, fake, None) == EABI
    assert lib.dcomp_actor_actions_v(fake, ctypes.byref(run), None, fake, fake, None) == EINVAL and b'obs' in lib.dcomp_last_error()
    assert lib.dcomp_actor_actions_v(fake, ctypes.byref(run), fake, fake, None, None) == EINVAL and b'vf' in lib.dcomp_last_error()
    for logits, logp in ((fake, None), (None, fake)):                    # action == NULL is the value-only call: nothing of the policy may be asked for
        r = _lib.DcompActorRun(ctypes.sizeof(_lib.DcompActorRun), 0, 1, 1, 0, 0, 0, 0, logits, logp)
        assert lib.dcomp_actor_actions_v(fake, ctypes.byref(r), fake, None, fake, None) == EINVAL
        assert b'value-only' in lib.dcomp_last_error()


def _gae_args(size=None, T=3, R=5, null=()):
    from deepcomp_amd import _lib
    p = lambda n: None if n in null else 4096                            # noqa: E731  (never dereferenced)
    return _lib.DcompGaeArgs(ctypes.sizeof(_lib.DcompGaeArgs) if size is None else size, T, R, 0.99, 0.95, p('reward'), p('vf'),
                             p('last_vf'), p('end'), p('advantages'), p('value_targets'))


def test_gae_refuses_bad_arguments_on_the_host(lib):
    from deepcomp_amd import _lib
    assert lib.dcomp_gae(None, None) == EINVAL
    for size in (0, ctypes.sizeof(_lib.DcompGaeArgs) - 8, ctypes.sizeof(_lib.DcompGaeArgs) + 8):
        assert lib.dcomp_gae(ctypes.byref(_gae_args(size=size)), None) == EABI
        assert b'dcomp_gae_args' in lib.dcomp_last_error()
    cases = [dict(null=('reward',)), dict(null=('vf',)), dict(null=('advantages',)), dict(null=('value_targets',)),
             dict(T=0), dict(T=-1), dict(R=0), dict(R=-5), dict(T=1, R=2 ** 40), dict(T=2 ** 10, R=2 ** 30), dict(T=2 ** 20, R=2 ** 20)]
    for kw in cases:
        rc = lib.dcomp_gae(ctypes.byref(_gae_args(**kw)), None)
        assert rc == EINVAL, (kw, rc, lib.dcomp_last_error())


def test_ctypes_mirrors_match_the_header(tmp_path):
    """Member names from the header text, sizes from a C program compiled against it."""
    from deepcomp_amd import _lib
    mirrors = (('dcomp_actor_value_cfg', _lib.DcompActorValueCfg), ('dcomp_gae_args', _lib.DcompGaeArgs))
    for cname, mirror in mirrors:
        members = cs.struct_members(cs.header('dcomp_types.h'), cname)
        assert members == [f[0] for f in mirror._fields_], (cname, members)
    sizes, = cs.c_program_output(
        tmp_path, '#include <stdio.h>\n#include "dcomp.h"\n'
                   'int f(dcomp_actor *a, const dcomp_actor_run *r, float *vf) {\n'
                   '    dcomp_actor_value_cfg c = {0};\n'
                   '    dcomp_gae_args g = {0};\n'
                   '    c.struct_size = (int32_t)sizeof c; c.shared = 1; c.wv = vf; c.bv = vf;\n'
                   '    g.struct_size = (int32_t)sizeof g; g.num_steps = 1; g.num_rows = 1; g.gamma = 0.99f; g.lambda = 1.0f;\n'
                   '    return dcomp_actor_set_value(a, &c) + dcomp_actor_actions_v(a, r, 0, 0, vf, 0) + dcomp_gae(&g, 0);\n'
                   '}\n'
                   'int main(void) {\n'
                   '    printf("%zu %zu %zu %zu\\n", sizeof(dcomp_actor_value_cfg), sizeof(dcomp_gae_args), sizeof(dcomp_actor_cfg), sizeof(dcomp_actor_run));\n'
                   '    return 0;\n'
                   '}\n', link=['-Wl,--unresolved-symbols=ignore-all'])
    assert sizes == [ctypes.sizeof(_lib.DcompActorValueCfg), ctypes.sizeof(_lib.DcompGaeArgs), ctypes.sizeof(_lib.DcompActorCfg),
                     ctypes.sizeof(_lib.DcompActorRun)]
    assert sizes[2:] == [24 + 6 * ctypes.sizeof(ctypes.c_void_p), 56]     # the existing structs stay as they are


def test_map_rllib_value_weights():
    from deepcomp_amd.actor import FcnetActor, layer_shapes
    U, B, H = 3, 4, 32
    nin, _, nout, shapes = layer_shapes('multi', U, B, H)
    rng = np.random.default_rng(0)
    pol = {n: rng.normal(size=s).astype(np.float32) for n, s in shapes.items()}
    v = {'w1': rng.normal(size=(nin, H)), 'b1': rng.normal(size=H), 'w2': rng.normal(size=(H, H)), 'b2': rng.normal(size=H),
         'wv': rng.normal(size=(H, 1)), 'bv': rng.normal(size=1)}
    v = {n: a.astype(np.float32) for n, a in v.items()}
    p = 'default_policy/'
    rl = {p + 'fc_1/kernel': pol['w1'], p + 'fc_1/bias': pol['b1'], p + 'fc_2/kernel': pol['w2'], p + 'fc_2/bias': pol['b2'],
          p + 'fc_out/kernel': pol['w3'], p + 'fc_out/bias': pol['b3'],
          p + 'fc_value_1/kernel': v['w1'], p + 'fc_value_1/bias': v['b1'], p + 'value_out/bias': v['bv'],
          p + 'fc_value_2/kernel': v['w2'], p + 'fc_value_2/bias': v['b2'], p + 'value_out/kernel': v['wv']}
    for style in (rl, {k + ':0': a for k, a in rl.items()}, {k[len(p):]: a for k, a in rl.items()}):      # RLlib, TF variable names, bare
        got = FcnetActor.map_rllib_value_weights(style)
        assert sorted(got) == sorted(v)
        for n in v:
            assert np.array_equal(got[n], v[n].reshape(got[n].shape)), n
        assert got['wv'].shape == (H,) and got['bv'].shape == (1,)
        assert np.array_equal(FcnetActor.map_rllib_weights(style)['w1'], pol['w1'])        # the policy's mapping is unaffected
    shared = {k: a for k, a in rl.items() if 'fc_value' not in k}                           # vf_share_layers: value_out only
    got = FcnetActor.map_rllib_value_weights(shared)
    assert sorted(got) == ['bv', 'wv'] and np.array_equal(got['wv'], v['wv'].reshape(-1))
    with pytest.raises(ValueError):
        FcnetActor.map_rllib_value_weights({k: a for k, a in rl.items() if 'value_out' not in k})
    with pytest.raises(ValueError):
        FcnetActor.map_rllib_value_weights({k: a for k, a in rl.items() if 'fc_value_2/bias' not in k})
    # [in][out], y = x W + b, in both forms of the branch
    x = rng.random((5, nin)).astype(np.float32)
    own = FcnetActor.map_rllib_value_weights(rl)
    want = np.tanh(np.tanh(x @ v['w1'] + v['b1']) @ v['w2'] + v['b2']) @ v['wv'][:, 0] + v['bv'][0]
    ref = FcnetActor.reference_value_of(pol, own, x, 'tanh', 'float64').numpy()
    assert ref.shape == (5,) and np.abs(ref - want).max() < 0.15          # (bf16-rounded weights: close, not equal)
    want = np.tanh(np.tanh(x @ pol['w1'] + pol['b1']) @ pol['w2'] + pol['b2']) @ v['wv'][:, 0] + v['bv'][0]
    ref = FcnetActor.reference_value_of(pol, got, x, 'tanh', 'float64').numpy()
    assert np.abs(ref - want).max() < 0.15
    chain = FcnetActor.reference_value_of(pol, got, x, 'tanh', 'bf16').numpy()
    assert chain.dtype == np.float32 and np.abs(chain - ref).max() < 0.1


def _discount_cumsum(x, g):
    """RLlib's discount_cumsum (scipy.signal.lfilter form), in float64."""
    out = np.zeros_like(x)
    run = np.zeros(x.shape[1:])
    for t in range(x.shape[0] - 1, -1, -1):
        run = x[t] + g * run
        out[t] = run
    return out


@pytest.mark.parametrize('lam', [1.0, 0.95])
def test_gae_reference_is_compute_advantages(lam):
    """RLlib's compute_advantages(use_gae=True) in float64 -- vpred_t = [vf_preds, last_r]; delta = rewards + gamma vpred_t[1:] -
    vpred_t[:-1]; advantages = discount_cumsum(delta, gamma lambda); value_targets = advantages + vf_preds -- within 1e-5 relative."""
    from deepcomp_amd.sampler import gae_reference
    rng = np.random.default_rng(3)
    T, R, gamma = 50, 37, 0.99
    rew = rng.uniform(-1, 1, size=(T, R)).astype(np.float32)
    vf = rng.normal(size=(T, R)).astype(np.float32)
    last = rng.normal(size=R).astype(np.float32)
    for last_vf in (last, None):
        adv, tgt = gae_reference(rew, vf, last_vf, None, gamma, lam)
        assert adv.dtype == tgt.dtype == np.float32 and adv.shape == tgt.shape == (T, R)
        vpred = np.concatenate([vf.astype(np.float64), (last if last_vf is not None else np.zeros(R))[None].astype(np.float64)])
        delta = rew.astype(np.float64) + gamma * vpred[1:] - vpred[:-1]
        want = _discount_cumsum(delta, gamma * lam)
        scale = np.abs(want).max()
        assert np.abs(adv - want).max() <= 1e-5 * scale
        assert np.abs(tgt - (want + vf)).max() <= 1e-5 * np.abs(want + vf).max()
    # episode ends: each stretch is a fragment of its own that ends with last_r = 0
    end = np.zeros(T, dtype=np.uint8)
    end[[11, 30]] = 1
    adv, _ = gae_reference(rew, vf, last, end, gamma, lam)
    for lo, hi, lr in ((0, 12, None), (12, 31, None), (31, T, last)):
        a, _ = gae_reference(rew[lo:hi], vf[lo:hi], lr, None, gamma, lam)
        assert np.array_equal(a, adv[lo:hi])


def test_gae_reference_hand_worked():
    """T = 3, one column, gamma = 0.5, lambda = 0.5 (every value a dyadic fraction: exact), step 1 ends an episode:
       t = 2: d = (1 + 0.5 * 4) - 2 = 1,       A = 1
       t = 1: end -> nv = 0, A = 0;  d = (2 + 0) - 1 = 1,  A = 1
       t = 0: d = (4 + 0.5 * 1) - 0.5 = 4,     A = 4 + 0.25 * 1 = 4.25"""
    from deepcomp_amd.sampler import gae_reference
    rew = np.array([[4.0], [2.0], [1.0]], dtype=np.float32)
    vf = np.array([[0.5], [1.0], [2.0]], dtype=np.float32)
    adv, tgt = gae_reference(rew, vf, np.array([4.0], dtype=np.float32), np.array([0, 1, 0], dtype=np.uint8), 0.5, 0.5)
    assert adv[:, 0].tolist() == [4.25, 1.0, 1.0]
    assert tgt[:, 0].tolist() == [4.75, 2.0, 3.0]
    # without the end the middle step sees what follows it: d = (2 + 0.5 * 2) - 1 = 2, A = 2 + 0.25 = 2.25; t = 0: d = 4, A = 4.5625
    adv, _ = gae_reference(rew, vf, np.array([4.0], dtype=np.float32), None, 0.5, 0.5)
    assert adv[:, 0].tolist() == [4.5625, 2.25, 1.0]
