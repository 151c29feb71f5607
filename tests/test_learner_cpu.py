"""CPU-side checks of the PPO learner (include/dcomp_learner.h, deepcomp_amd/learner.py): the symbols exist and are declared, the
ctypes mirrors match the header, arguments are refused on the host before the first HIP call and before the handle is read (a fake
one is never dereferenced), and the specification -- ppo_loss_reference, adam_reference, the kl_coeff rule, the RLlib weight
names -- is what it claims to be.  No GPU compute is called here.  Refusals that need a live handle (rows > max_rows, an actor
without a value trunk, a shared value) are in tests/test_learner_gpu.py."""
import ctypes
import re

import numpy as np
import pytest

from tests import c_surface as cs
from tests.c_surface import EABI, EINVAL, EUNSUPPORTED, OK, lib  # noqa: F401  (lib: the fixture)
from tests.c_surface import LOSS_INPUTS as _LOSS_INPUTS
from tests.c_surface import ppo_batch as _batch
from tests.c_surface import ppo_hyper as _hyper


def test_symbols_are_exported_and_declared(lib):
    from deepcomp_amd import _lib
    hdr = open(cs.header('dcomp_learner.h')).read()
    assert len(_lib.LEARNER_EXPORTS) == 7 and len(set(_lib.LEARNER_EXPORTS)) == 7
    for name in _lib.LEARNER_EXPORTS:
        assert re.search(r'\bint %s\s*\(' % name, hdr), name
        getattr(lib, name)
        assert name not in _lib.EXPORTS                                   # EXPORTS stays what include/dcomp.h declares
    assert sorted(re.findall(r'\bint (dcomp_learner_\w+)\s*\(', hdr)) == sorted(_lib.LEARNER_EXPORTS)
    assert len(_lib.EXPORTS) == 42
    assert '#include "dcomp_types.h"' in hdr and 'DCOMP_ABI_VERSION 3' in open(cs.header('dcomp.h')).read()


def test_ctypes_mirrors_match_the_header(tmp_path):
    """Member names from the header text, sizes from a C program compiled against it (C99, pedantic)."""
    from deepcomp_amd import _lib
    mirrors = (('dcomp_learner_arrays', _lib.DcompLearnerArrays), ('dcomp_learner_cfg', _lib.DcompLearnerCfg),
               ('dcomp_ppo_batch', _lib.DcompPpoBatch), ('dcomp_ppo_hyper', _lib.DcompPpoHyper))
    for cname, mirror in mirrors:
        members = cs.struct_members(cs.header('dcomp_learner.h'), cname)
        assert members == [f[0] for f in mirror._fields_], (cname, members)
    assert tuple(f[0] for f in _lib.DcompLearnerArrays._fields_[2:]) == _lib.LEARNER_ARRAYS
    sizes, = cs.c_program_output(
        tmp_path, '#include <stdio.h>\n#include "dcomp_learner.h"\n'
                   'int main(void) {\n'
                   '    printf("%zu %zu %zu %zu %d %d\\n", sizeof(dcomp_learner_arrays), sizeof(dcomp_learner_cfg), sizeof(dcomp_ppo_batch),\n'
                   '           sizeof(dcomp_ppo_hyper), DCOMP_PPO_NUM_STATS, DCOMP_LEARNER_ADAM_V);\n'
                   '    return 0;\n'
                   '}\n')
    # the two public headers side by side
    cs.compiles_as_c99(tmp_path, 'both', ['#include "dcomp.h"\n#include "dcomp_learner.h"\nint main(void) { return DCOMP_EABI == -7 ? 0 : 1; }\n'])
    assert sizes == [ctypes.sizeof(_lib.DcompLearnerArrays), ctypes.sizeof(_lib.DcompLearnerCfg), ctypes.sizeof(_lib.DcompPpoBatch),
                     ctypes.sizeof(_lib.DcompPpoHyper), _lib.PPO_NUM_STATS, _lib.LEARNER_ADAM_V]
    assert len(_lib.PPO_STATS) == _lib.PPO_NUM_STATS


def _arrays(keep, null=(), size=None):
    from deepcomp_amd import _lib
    fp = ctypes.POINTER(ctypes.c_float)
    arrs = {n: np.zeros(4, dtype=np.float32) for n in _lib.LEARNER_ARRAYS}
    keep.append(arrs)
    return _lib.DcompLearnerArrays(ctypes.sizeof(_lib.DcompLearnerArrays) if size is None else size, 0,
                                   *[None if n in null else arrs[n].ctypes.data_as(fp) for n in _lib.LEARNER_ARRAYS])


def _cfg(keep, size=None, shared=0, max_rows=64, beta1=0.9, beta2=0.999, eps=1e-8, weights='ok'):
    from deepcomp_amd import _lib
    w = _arrays(keep) if weights == 'ok' else weights
    keep.append(w)
    return _lib.DcompLearnerCfg(ctypes.sizeof(_lib.DcompLearnerCfg) if size is None else size, shared, max_rows, beta1, beta2, eps, 0,
                                ctypes.pointer(w) if w is not None else None)


def test_create_refuses_bad_arguments_on_the_host(lib):
    from deepcomp_amd import _lib
    keep, fake, out = [], ctypes.c_void_p(4096), ctypes.c_void_p()
    assert lib.dcomp_learner_create(None, ctypes.byref(_cfg(keep)), ctypes.byref(out)) == EINVAL
    assert lib.dcomp_learner_create(fake, None, ctypes.byref(out)) == EINVAL
    assert lib.dcomp_learner_create(fake, ctypes.byref(_cfg(keep)), None) == EINVAL
    for size in (0, ctypes.sizeof(_lib.DcompLearnerCfg) - 8, ctypes.sizeof(_lib.DcompLearnerCfg) + 8):
        assert lib.dcomp_learner_create(fake, ctypes.byref(_cfg(keep, size=size)), ctypes.byref(out)) == EABI
        assert b'dcomp_learner_cfg' in lib.dcomp_last_error()
    assert lib.dcomp_learner_create(fake, ctypes.byref(_cfg(keep, shared=1)), ctypes.byref(out)) == EUNSUPPORTED
    assert b'shared' in lib.dcomp_last_error()
    cases = [dict(shared=2), dict(shared=-1), dict(max_rows=0), dict(max_rows=-3), dict(max_rows=2 ** 28 + 1), dict(beta1=1.0), dict(beta1=-0.1),
             dict(beta2=1.5), dict(beta2=float('nan')), dict(eps=0.0), dict(eps=-1e-8), dict(weights=None)] + \
            [dict(weights=_arrays(keep, null=(n,))) for n in _lib.LEARNER_ARRAYS]
    for kw in cases:
        rc = lib.dcomp_learner_create(fake, ctypes.byref(_cfg(keep, **kw)), ctypes.byref(out))
        assert rc == EINVAL, (kw, rc, lib.dcomp_last_error())
        assert out.value is None
    bad = _arrays(keep, size=ctypes.sizeof(_lib.DcompLearnerArrays) - 8)
    assert lib.dcomp_learner_create(fake, ctypes.byref(_cfg(keep, weights=bad)), ctypes.byref(out)) == EABI
    assert b'dcomp_learner_arrays' in lib.dcomp_last_error()
    assert lib.dcomp_learner_destroy(None) == OK


def test_grads_refuses_bad_arguments_on_the_host(lib):
    from deepcomp_amd import _lib
    fake = ctypes.c_void_p(4096)
    g = lambda l, b, h, s: lib.dcomp_learner_grads(l, ctypes.byref(b) if b is not None else None, ctypes.byref(h) if h is not None else None, s, None)      # noqa: E731
    assert g(None, _batch(), _hyper(), fake) == EINVAL
    assert g(fake, None, _hyper(), fake) == EINVAL
    assert g(fake, _batch(), None, fake) == EINVAL
    assert g(fake, _batch(), _hyper(), None) == EINVAL and b'stats_dev' in lib.dcomp_last_error()
    assert g(fake, _batch(size=ctypes.sizeof(_lib.DcompPpoBatch) + 8), _hyper(), fake) == EABI and b'dcomp_ppo_batch' in lib.dcomp_last_error()
    assert g(fake, _batch(), _hyper(size=8), fake) == EABI and b'dcomp_ppo_hyper' in lib.dcomp_last_error()
    assert g(fake, _batch(fmt=1), _hyper(), fake) == EUNSUPPORTED and b'compact' in lib.dcomp_last_error()
    assert g(fake, _batch(fmt=2), _hyper(), fake) == EINVAL
    for missing in _LOSS_INPUTS:
        rc = g(fake, _batch(given=[n for n in _LOSS_INPUTS if n != missing]), _hyper(), fake)
        assert rc == EINVAL and b'NULL' in lib.dcomp_last_error(), missing
    assert g(fake, _batch(given=('obs', 'dlogits')), _hyper(), fake) == EINVAL and b'together' in lib.dcomp_last_error()
    assert g(fake, _batch(given=('obs', 'dvalue')), _hyper(), fake) == EINVAL
    assert g(fake, _batch(rows=0), _hyper(), fake) == EINVAL
    assert g(fake, _batch(given=('obs', 'dlogits', 'dvalue'), rows=-1), _hyper(), fake) == EINVAL and b'rows' in lib.dcomp_last_error()
    assert g(fake, _batch(), _hyper(clip=-0.1), fake) == EINVAL
    assert g(fake, _batch(), _hyper(vf_clip=float('nan')), fake) == EINVAL


def test_evaluate_apply_read_load_refuse_bad_arguments_on_the_host(lib):
    from deepcomp_amd import _lib
    keep, fake = [], ctypes.c_void_p(4096)
    ev = lambda l, b: lib.dcomp_learner_evaluate(l, ctypes.byref(b) if b is not None else None, None)      # noqa: E731
    assert ev(None, _batch(given=('obs', 'actions', 'logp'))) == EINVAL
    assert ev(fake, None) == EINVAL
    assert ev(fake, _batch(given=('obs', 'actions', 'logp'), size=16)) == EABI
    assert ev(fake, _batch(given=('obs', 'actions', 'logp'), fmt=1)) == EUNSUPPORTED
    assert ev(fake, _batch(given=('actions', 'logp'))) == EINVAL and b'obs' in lib.dcomp_last_error()
    assert ev(fake, _batch(given=('obs', 'logp'))) == EINVAL and b'actions' in lib.dcomp_last_error()
    assert ev(fake, _batch(given=('obs', 'actions'))) == EINVAL and b'nothing to write' in lib.dcomp_last_error()
    assert ev(fake, _batch(given=('obs', 'actions', 'vf', 'dlogits', 'dvalue'))) == EINVAL
    assert ev(fake, _batch(given=('obs', 'actions', 'vf'), rows=0)) == EINVAL

    assert lib.dcomp_learner_apply(None, 1e-3, None) == EINVAL
    for lr in (-1e-3, float('nan'), float('inf')):
        assert lib.dcomp_learner_apply(fake, lr, None) == EINVAL and b'lr' in lib.dcomp_last_error()

    arr = _arrays(keep)
    assert lib.dcomp_learner_read(None, 0, ctypes.byref(arr), None, None) == EINVAL
    assert lib.dcomp_learner_read(fake, 4, ctypes.byref(arr), None, None) == EINVAL and b'which' in lib.dcomp_last_error()
    assert lib.dcomp_learner_read(fake, -1, ctypes.byref(arr), None, None) == EINVAL
    assert lib.dcomp_learner_read(fake, 0, None, None, None) == EINVAL
    assert lib.dcomp_learner_read(fake, 0, ctypes.byref(_arrays(keep, size=8)), None, None) == EABI

    ok = lambda: ctypes.byref(_arrays(keep))                              # noqa: E731
    assert lib.dcomp_learner_load_state(None, ok(), ok(), ok(), 0, None) == EINVAL
    assert lib.dcomp_learner_load_state(fake, None, ok(), ok(), 0, None) == EINVAL
    assert lib.dcomp_learner_load_state(fake, ok(), ok(), None, 0, None) == EINVAL
    assert lib.dcomp_learner_load_state(fake, ok(), ctypes.byref(_arrays(keep, null=('vb2',))), ok(), 0, None) == EINVAL and b'adam_m.vb2' in lib.dcomp_last_error()
    assert lib.dcomp_learner_load_state(fake, ok(), ok(), ctypes.byref(_arrays(keep, size=8)), 0, None) == EABI
    assert lib.dcomp_learner_load_state(fake, ok(), ok(), ok(), -1, None) == EINVAL and b'step' in lib.dcomp_last_error()


def _case(kind, U, B, H, rows, seed, activation='tanh'):
    """Weights, and a batch whose old_* come from a perturbed weight set."""
    from deepcomp_amd.actor import FcnetActor, layer_shapes
    rng = np.random.default_rng(seed)
    nin, heads, n3, _ = layer_shapes(kind, U, B, H)
    w = FcnetActor.random_weights(kind, U, B, H, seed, bias_std=0.1)
    vw = FcnetActor.random_value_weights(kind, U, B, H, seed, bias_std=0.1)
    pert = lambda d: {n: (a + rng.normal(size=a.shape).astype(np.float32) * 0.3 * (a.std() + 0.05)) for n, a in d.items()}      # noqa: E731
    w0, vw0 = pert(w), pert(vw)
    obs = rng.random((rows, nin)).astype(np.float32)
    old_logits = FcnetActor.reference_logits_of(w0, obs, activation, 'bf16').numpy()
    actions = rng.integers(0, B + 1, size=(rows, heads)).astype(np.uint8)
    lsm = old_logits.reshape(rows, heads, B + 1).astype(np.float64)
    lsm = lsm - np.log(np.exp(lsm).sum(-1, keepdims=True))
    old_logp = np.take_along_axis(lsm, actions[..., None].astype(np.int64), -1)[..., 0].astype(np.float32)
    old_vf = FcnetActor.reference_value_of(w0, vw0, obs, activation, 'bf16').numpy()
    batch = {'obs': obs, 'actions': actions, 'old_logp': old_logp, 'old_logits': old_logits, 'advantages': rng.normal(size=rows).astype(np.float32),
             'value_targets': (old_vf + rng.normal(size=rows) * 0.5).astype(np.float32), 'old_vf': old_vf}
    return w, vw, batch


@pytest.mark.parametrize('kind,activation', [('multi', 'tanh'), ('central', 'tanh'), ('central', 'relu')])
def test_float64_gradients_agree_with_finite_differences(kind, activation):
    """Central differences of ppo_loss_reference(form='float64')'s own total_loss on a 3-row case, at entries of every array,
    with every coefficient switched on and rows inside and outside both clips.  The weights sit on the bf16 grid, so the model's
    rounding is the identity at the point of differentiation; the difference quotient runs with round_weights=False."""
    import torch
    from deepcomp_amd import learner
    U, B, H = 3, 2, 32
    w, vw, batch = _case(kind, U, B, H, 3, 11, activation)
    batch['value_targets'] = batch['old_vf'] + np.array([0.2, 3.0, -2.5], dtype=np.float32)
    hy = {'clip_param': 0.3, 'vf_clip_param': 1.0, 'vf_loss_coeff': 0.7, 'entropy_coeff': 0.05, 'kl_coeff': 0.2}
    if kind == 'central':
        batch['num_active'] = 2
    grid = lambda n, a: a if n in ('b1', 'b2', 'b3', 'bv') else torch.as_tensor(a).to(torch.bfloat16).to(torch.float32).numpy()      # noqa: E731
    w, vw = {n: grid(n, a) for n, a in w.items()}, {n: grid(n, a) for n, a in vw.items()}
    _, grads, _ = learner.ppo_loss_reference(w, vw, batch, hy, activation, 'float64')
    arrays = learner.join_weights(w, vw, np.float64)
    rng = np.random.default_rng(0)
    eps = 1e-5
    for n in learner.ARRAYS:
        size = arrays[n].size
        for i in rng.choice(size, size=min(4, size), replace=False):
            vals = []
            for sgn in (1, -1):
                mod = {k: a.copy() for k, a in arrays.items()}
                mod[n].reshape(-1)[i] += sgn * eps
                vals.append(learner.ppo_loss_reference(*learner.split_weights(mod), batch, hy, activation, 'float64', round_weights=False)[0]['total_loss'])
            fd, got = (vals[0] - vals[1]) / (2 * eps), float(grads[n].reshape(-1)[i])
            assert abs(fd - got) <= 1e-6 * max(1.0, abs(fd)), (n, i, fd, got)     # (float64, a smooth loss away from its kinks: the quotient's own error is ~eps^2)
    assert any(np.abs(g).max() > 0 for g in grads.values())


def test_bf16_chain_follows_the_model():
    """The hand-written chain is the model up to its bf16 roundings: every statistic and gradient array close, and the forward pass
    is reference_logits_of / reference_value_of(form='bf16') to the bit."""
    from deepcomp_amd import learner
    from deepcomp_amd.actor import FcnetActor
    for kind, act in (('multi', 'tanh'), ('central', 'relu')):
        w, vw, batch = _case(kind, 4, 3, 64, 50, 5, act)
        hy = {'vf_clip_param': 0.05, 'entropy_coeff': 0.01}
        s64, g64, r64 = learner.ppo_loss_reference(w, vw, batch, hy, act, 'float64')
        s16, g16, r16 = learner.ppo_loss_reference(w, vw, batch, hy, act, 'bf16')
        assert 0 < r64['clipped'].sum() < 50 and 0 < r64['vf_clipped'].sum() < 50      # both branches of both clips occur
        for n in learner.STATS:
            assert abs(s64[n] - s16[n]) <= 0.02 * max(1.0, abs(s64[n])), (n, s64[n], s16[n])
        for n in learner.ARRAYS:
            scale = np.abs(g64[n]).max()
            assert scale > 0 and np.abs(g64[n] - g16[n]).max() <= 0.05 * scale, (n, scale, np.abs(g64[n] - g16[n]).max())
        assert np.array_equal(r16['vf'].numpy(), FcnetActor.reference_value_of(w, vw, batch['obs'], act, 'bf16').numpy())
    # upstream gradients instead of the loss's: a linear functional, whose gradient of b3 is the column sum of dlogits
    w, vw, batch = _case('multi', 4, 3, 32, 10, 6)
    up = {'obs': batch['obs'], 'dlogits': np.ones((10, 4), dtype=np.float32), 'dvalue': np.full(10, 2.0, dtype=np.float32)}
    for form in ('float64', 'bf16'):
        _, g, _ = learner.ppo_loss_reference(w, vw, up, None, 'tanh', form)
        assert np.allclose(g['b3'], 10.0) and np.allclose(g['bv'], 20.0)


def test_adam_reference_is_torch_adam():
    """20 steps of adam_reference against torch.optim.Adam on CPU float32 (which orders its operations differently: lerp for the
    first moment, addcdiv at the end).  Measured here: the largest difference relative to the weight's own size (|w| >= 0.01) over
    all 20 steps is 2.33e-7, two float32 roundings (2^-23 = 1.19e-7); asserted with a margin of two more: 4 x 2^-23."""
    import torch
    from deepcomp_amd.learner import adam_reference
    rng = np.random.default_rng(2)
    w0 = rng.normal(size=2000).astype(np.float32)
    w0[np.abs(w0) < 0.01] = 0.01
    grads = [(rng.normal(size=2000) * 10.0 ** rng.uniform(-4, 1, size=2000)).astype(np.float32) for _ in range(20)]
    lr = 1e-3
    p = torch.nn.Parameter(torch.as_tensor(w0.copy()))
    opt = torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    w, m, v = w0.copy(), np.zeros_like(w0), np.zeros_like(w0)
    worst = 0.0
    for t, g in enumerate(grads, 1):
        p.grad = torch.as_tensor(g.copy())
        opt.step()
        w, m, v = adam_reference(w, g, m, v, t, lr)
        assert w.dtype == m.dtype == v.dtype == np.float32
        worst = max(worst, float((np.abs(w - p.detach().numpy()) / np.maximum(np.abs(w), 0.01)).max()))
    print(f'adam_reference vs torch.optim.Adam, 20 steps: largest relative difference {worst:.3e}')
    assert worst <= 4 * 2.0 ** -23
    assert np.abs(w - w0).max() > 1e-3                                    # (the weights did move)


def test_kl_coeff_rule():
    from deepcomp_amd.learner import adapt_kl_coeff
    assert adapt_kl_coeff(0.2, 0.021, 0.01) == pytest.approx(0.3)         # above twice the target
    assert adapt_kl_coeff(0.2, 0.0049, 0.01) == pytest.approx(0.1)        # below half of it
    for kl in (0.005, 0.01, 0.02):
        assert adapt_kl_coeff(0.2, kl, 0.01) == 0.2                       # the band, its ends included


def test_to_rllib_weights_round_trips():
    from deepcomp_amd import learner
    from deepcomp_amd.actor import FcnetActor
    for kind in ('multi', 'central'):
        w = FcnetActor.random_weights(kind, 3, 4, 32, 1, bias_std=0.1)
        vw = FcnetActor.random_value_weights(kind, 3, 4, 32, 1, bias_std=0.1)
        rl = learner.to_rllib_weights(learner.join_weights(w, vw))
        assert len(rl) == 12 and rl['default_policy/value_out/kernel'].shape == (32, 1)
        back, vback = FcnetActor.map_rllib_weights(rl), FcnetActor.map_rllib_value_weights(rl)
        assert sorted(back) == sorted(w) and sorted(vback) == sorted(vw)
        for n in w:
            assert np.array_equal(back[n], w[n]), n
        for n in vw:
            assert np.array_equal(vback[n], vw[n].reshape(vback[n].shape)), n
        a2, v2 = learner.split_weights(learner.join_weights(w, vw))
        assert all(np.array_equal(a2[n], w[n]) for n in w) and all(np.array_equal(v2[n], vw[n].reshape(-1) if n in ('wv', 'bv') else vw[n]) for n in vw)
