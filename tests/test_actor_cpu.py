"""CPU-side checks of the fcnet actor (deepcomp_amd/actor.py, dcomp_actor_* in include/dcomp.h): argument validation happens on the
host before the first HIP call, the ctypes mirrors match the header, RLlib's weight names map onto the six arrays, and the two
forms of the reference arithmetic agree within the bf16 chain's error.  No GPU compute is called here."""
import ctypes
import re

import numpy as np
import pytest

from tests import c_surface as cs
from tests.c_surface import EABI, EINVAL, EUNSUPPORTED, OK, lib  # noqa: F401  (lib: the fixture)


def _cfg(kind=1, U=4, B=5, H=64, act=0, size=None, keep=None, null=()):
    """A dcomp_actor_cfg with zero weights of the right shapes (keep: list that holds the arrays alive)."""
    from deepcomp_amd import _lib
    from deepcomp_amd.actor import layer_shapes
    fp = ctypes.POINTER(ctypes.c_float)
    _, _, _, shapes = layer_shapes(kind, max(U, 1), max(B, 1), max(H, 1))
    arrs = {n: np.zeros(s, dtype=np.float32) for n, s in shapes.items()}
    if keep is not None:
        keep.append(arrs)
    ptr = lambda n: None if n in null else arrs[n].ctypes.data_as(fp)      # noqa: E731
    return _lib.DcompActorCfg(ctypes.sizeof(_lib.DcompActorCfg) if size is None else size, kind, U, B, H, act,
                              *[ptr(n) for n in ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')])


def test_actor_create_refuses_bad_arguments_on_the_host(lib):
    """Every case fails validation before any HIP call (there is no GPU here) and names its cause."""
    keep = []
    h = ctypes.c_void_p()
    assert lib.dcomp_actor_create(None, ctypes.byref(h)) == EINVAL
    assert lib.dcomp_actor_create(ctypes.byref(_cfg(keep=keep)), None) == EINVAL
    cases = [(dict(kind=2), EINVAL, 'obs_kind'), (dict(U=0), EINVAL, 'num_ue'), (dict(B=0), EINVAL, 'num_bs'),
             (dict(H=48), EINVAL, 'hidden'), (dict(H=0), EINVAL, 'hidden'), (dict(act=2), EINVAL, 'activation'),
             (dict(null=('w2',)), EINVAL, 'NULL'), (dict(null=('b3',)), EINVAL, 'NULL'),
             (dict(B=65), EUNSUPPORTED, 'num_bs'), (dict(U=1025, B=1), EUNSUPPORTED, 'num_ue'), (dict(H=288), EUNSUPPORTED, 'hidden'),
             (dict(kind=0, U=94, B=5), EUNSUPPORTED, 'inputs'),          # 94 * 11 = 1 034 inputs > 1 024
             (dict(kind=0, U=100, B=5), EUNSUPPORTED, 'inputs'),
             (dict(kind=0, U=200, B=2), EUNSUPPORTED, 'logits')]         # 200 * 5 = 1 000 inputs, 200 * 3 = 600 logits > 512
    for kw, code, word in cases:
        h = ctypes.c_void_p(1)
        rc = lib.dcomp_actor_create(ctypes.byref(_cfg(keep=keep, **kw)), ctypes.byref(h))
        assert rc == code, (kw, rc, lib.dcomp_last_error())
        assert h.value is None, kw                                       # *out is cleared
        assert word.encode() in lib.dcomp_last_error(), (kw, lib.dcomp_last_error())


def test_actor_struct_size_mismatch_is_an_abi_error(lib):
    from deepcomp_amd import _lib
    keep = []
    h = ctypes.c_void_p()
    for size in (0, ctypes.sizeof(_lib.DcompActorCfg) - 8, ctypes.sizeof(_lib.DcompActorCfg) + 8):
        assert lib.dcomp_actor_create(ctypes.byref(_cfg(keep=keep, size=size)), ctypes.byref(h)) == EABI
        assert b'dcomp_actor_cfg' in lib.dcomp_last_error()
    fake = ctypes.c_void_p(4096)                       # never dereferenced: the calls below fail validation first
    run = _lib.DcompActorRun(ctypes.sizeof(_lib.DcompActorRun), 0, 1, 1, 0, 0, 0, 0, None, None)
    assert lib.dcomp_actor_actions(None, ctypes.byref(run), fake, fake, None) == EINVAL
    assert lib.dcomp_actor_destroy(None) == OK


def test_actor_ctypes_mirrors_match_the_header():
    from deepcomp_amd import _lib
    for cname, mirror in (('dcomp_actor_cfg', _lib.DcompActorCfg), ('dcomp_actor_run', _lib.DcompActorRun)):
        members = cs.struct_members(cs.header('dcomp_types.h'), cname)
        assert members == [f[0] for f in mirror._fields_], (cname, members)
    assert ctypes.sizeof(_lib.DcompActorCfg) == 24 + 6 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.DcompActorRun) == 56
    hdr = open(cs.header('dcomp.h')).read()
    assert '#define DCOMP_ABI_VERSION 3' in hdr                          # the new structs carry their own size: no version bump
    for name in ('dcomp_actor_create', 'dcomp_actor_destroy', 'dcomp_actor_actions'):
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr)


def test_from_rllib_weights_maps_names_and_orders():
    from deepcomp_amd.actor import FcnetActor, layer_shapes
    U, B, H = 3, 4, 32
    nin, _, nout, shapes = layer_shapes('multi', U, B, H)
    rng = np.random.default_rng(0)
    w = {n: rng.normal(size=s).astype(np.float32) for n, s in shapes.items()}
    rl = {'default_policy/fc_1/kernel': w['w1'], 'default_policy/fc_1/bias': w['b1'], 'default_policy/fc_out/bias': w['b3'],
          'default_policy/fc_2/kernel': w['w2'], 'default_policy/fc_2/bias': w['b2'], 'default_policy/fc_out/kernel': w['w3'],
          'default_policy/fc_value_1/kernel': np.zeros((nin, H), np.float32), 'default_policy/fc_value_1/bias': np.zeros(H, np.float32),
          'default_policy/value_out/kernel': np.zeros((H, 1), np.float32), 'default_policy/value_out/bias': np.zeros(1, np.float32)}
    got = FcnetActor.map_rllib_weights(rl)
    assert sorted(got) == sorted(w)
    for n in w:
        assert np.array_equal(got[n], w[n]), n
    assert np.array_equal(FcnetActor.map_rllib_weights({k + ':0': v for k, v in rl.items()})['w3'], w['w3'])       # TF variable names
    with pytest.raises(ValueError):
        FcnetActor.map_rllib_weights({k: v for k, v in rl.items() if 'fc_2/bias' not in k})
    # [in][out]: y = x W + b, as reference_logits reads it
    x = rng.random((5, nin)).astype(np.float32)
    want = np.tanh(np.tanh(x @ w['w1'] + w['b1']) @ w['w2'] + w['b2']) @ w['w3'] + w['b3']
    ref = FcnetActor.reference_logits_of(got, x, 'tanh', 'float64').numpy()
    assert ref.shape == (5, nout) and np.abs(ref - want).max() < 0.1      # (bf16-rounded weights: close, not equal)


@pytest.mark.parametrize('kind,U,B,H', [('multi', 32, 10, 256), ('multi', 6, 64, 256), ('central', 10, 5, 256), ('central', 32, 10, 64)])
def test_reference_forms_agree_within_the_chain_error(kind, U, B, H):
    """The bf16 / f32 chain against the same bf16-rounded model in float64: three roundings to bf16 (2^-9 relative each) in front of
    sums of up to 256 terms -- a few 1e-3 at logit std ~0.4, and the choice differs in well under 1 % of the decisions."""
    from deepcomp_amd.actor import FcnetActor, layer_shapes
    nin, heads, nout, _ = layer_shapes(kind, U, B, H)
    w = FcnetActor.random_weights(kind, U, B, H, seed=1, bias_std=0.1)
    rng = np.random.default_rng(2)
    x = rng.random((512, nin)).astype(np.float32)
    x[:, :B] = x[:, :B] > 0.5
    chain = FcnetActor.reference_logits_of(w, x, 'tanh', 'bf16')
    ref = FcnetActor.reference_logits_of(w, x, 'tanh', 'float64')
    assert chain.dtype.is_floating_point and chain.shape == ref.shape == (512, nout)
    err = float(np.abs(chain.numpy().astype(np.float64) - ref.numpy()).max())
    std = float(ref.numpy().std())
    assert 0.2 < std < 1.0
    assert 0 < err < 0.03 * std, (err, std)
    a, b = chain.numpy().reshape(512, heads, B + 1).argmax(-1), ref.numpy().reshape(512, heads, B + 1).argmax(-1)
    assert (a != b).mean() < 0.01
    # relu with integer data is exact in both forms
    wi = {n: np.round(3 * v) for n, v in w.items()}
    xi = (x > 0.5).astype(np.float32)
    assert np.array_equal(FcnetActor.reference_logits_of(wi, xi, 'relu', 'bf16').numpy().astype(np.float64),
                          FcnetActor.reference_logits_of(wi, xi, 'relu', 'float64').numpy())


def test_gumbel_noise_uses_the_documented_counter_layout():
    from deepcomp_amd.actor import DRAW_TAG, gumbel_noise
    seen = []

    def philox(ctr, key):
        seen.append((tuple(ctr), tuple(key)))
        return [0x00000000, 0x80000000, 0xFFFFFFFF, 0x12345678]
    g = gumbel_noise(philox, (7 << 32) | 5, 9, [2 ** 32 - 1], 2, 6)
    assert g.shape == (1, 2, 6) and np.isfinite(g).all()
    assert seen == [((2 ** 32 - 1, (hd << 16) | blk, 9, DRAW_TAG), (5, 7)) for hd in range(2) for blk in range(2)]
    u = [(0 + 0.5) / 2 ** 24, (0x800000 + 0.5) / 2 ** 24, 1 - 2.0 ** -24]
    assert np.allclose(g[0, 0, :3], [-np.log(-np.log(v)) for v in u], rtol=1e-6)


def test_header_with_the_actor_entry_points_is_c99(tmp_path):
    cs.compiles_as_c99(tmp_path, 'actor_hdr', [
        '#include "dcomp.h"\n'
        'int f(const float *w, dcomp_actor **a) {\n'
        '    dcomp_actor_cfg c = {0};\n'
        '    dcomp_actor_run r = {0};\n'
        '    c.struct_size = (int32_t)sizeof c; c.obs_kind = DCOMP_MULTI; c.activation = DCOMP_ACT_TANH; c.w1 = w;\n'
        '    r.struct_size = (int32_t)sizeof r; r.obs_format = DCOMP_ACTOR_COMPACT;\n'
        '    return dcomp_actor_create(&c, a) + dcomp_actor_actions(*a, &r, 0, 0, 0) + dcomp_actor_destroy(*a);\n'
        '}\n'])
