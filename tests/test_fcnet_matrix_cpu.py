"""The self-check of tests/fcnet_cases.py, without a GPU: (1) the library's own constants and plans (dcomp_fcnet_describe) on known
shapes, and what the kernels rely on over every accepted shape (tests/fcnet_plan_check.cpp); (2) the table reaches every
instantiation of actor_kernel / learner_kernel / wgrad_block / wgrad_bias and every host-side branch listed in REQUIRED -- a case
taken out of the table fails here, by the name of the cell it alone reached; (3) every integer case's float64 reference meets its
exactness conditions, so a case that does not is found here and not on the device; (4) float32 emulations of the log-sum-exp walk
and of the loss epilogue stay inside the bounds the GPU tests hold the kernels to, and the logits do go past expf's float32 range."""
import numpy as np
import pytest

from tests import fcnet_cases as fc


def test_constants_are_the_librarys():
    assert (fc.KC, fc.TILE, fc.WAVES) == (144, 32, 4)
    assert (fc.CHUNK_UNIT, fc.MAX_CHUNKS) == (2048, 128)
    assert fc.CHUNK_UNIT == fc.CHUNK
    assert fc.GRID_TILES == 2048                                  # tests/test_actor_gpu.py: "2 048 tiles a round on 256 CUs"
    assert fc.grid_tiles(256) == 2048 and fc.grid_tiles(0) == 2048 and fc.grid_tiles(64) == 512      # (0: the library's fallback)


def test_the_librarys_plan_on_known_shapes():
    """Shapes whose dispatch the existing tests' comments state."""
    d = fc.actor_dispatch('multi', 32, 64, 256)                   # test_actor_gpu: K = 257 (two input chunks), N = 65
    assert (d['K1'], d['chunks'], d['N3'], d['NT3'], d['mt']) == (257, 2, 65, 3, 8)
    d = fc.actor_dispatch('central', 32, 10, 64)                  # K = 672: five chunks
    assert (d['K1'], d['chunks'], d['mt']) == (672, 5, 2)
    d = fc.actor_dispatch('central', 8, 63, 32)                   # the limits: DCOMP_ACTOR_MAX_IN 1 024, DCOMP_ACTOR_MAX_LOGITS 512
    assert (d['K1'], d['K1p'], d['chunks'], d['N3'], d['NT3'], d['NT3v']) == (1016, 1024, 8, 512, 16, 17)
    d = fc.actor_dispatch('multi', 4, 31, 64)
    assert (d['N3'], d['NT3'], d['NT3v']) == (32, 1, 2)
    d = fc.learner_dispatch('multi', 7, 5, 256)                   # an odd number of input tiles, output tiles a multiple of 4
    assert d['blocks'][0] == (1, 4) and d['blocks'][1] == (2, 4) and d['blocks'][2] == (2, 1)
    d = fc.learner_dispatch('central', 8, 63, 32)
    assert d['blocks'][:3] == [(2, 1), (1, 1), (1, 4)] and d['bias'][:3] == [1, 1, 4]
    assert fc.row_split(6400) == dict(mult=1, chunk_rows=2048, nchunks=4)          # test_learner_gpu: three chunks and a partial one
    assert fc.row_split(128 * 2048)['mult'] == 1 and fc.row_split(128 * 2048 + 1)['mult'] == 2
    assert fc.row_split(fc.rows_of(*fc.MULT2_SHAPE[:3])) == dict(mult=2, chunk_rows=4096, nchunks=65)
    assert [fc.wgrad_mb(t) for t in (1, 2, 3, 8)] == [1, 2, 1, 2] and [fc.wgrad_nb(t) for t in (1, 3, 4, 16)] == [1, 1, 4, 4]
    # a shape dcomp_actor_create refuses (tests/test_actor_cpu.py) is refused with the same code
    with pytest.raises(NotImplementedError, match='inputs'):
        fc.describe('central', 94, 5, 64)
    with pytest.raises(ValueError, match='hidden'):
        fc.describe('multi', 4, 5, 48)


def test_what_the_kernels_rely_on_holds_for_every_accepted_shape(tmp_path):
    """tests/fcnet_plan_check.cpp, a stand-alone host program over the plan header alone, under the host sanitizers: K1p a multiple
    of 16, XS an odd number of 16-byte slots, four waves' LDS under 64 KB, nchunks <= MAX_CHUNKS, ntask the sum of its parts, ..."""
    import os
    import subprocess
    exe = str(tmp_path / 'fcnet_plan_check')
    # (the runtimes linked statically: the program does not depend on where the loader puts them among its libraries)
    subprocess.run(['g++', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan', '-o', exe,
                    os.path.join(fc.REPO, 'tests', 'fcnet_plan_check.cpp')], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_every_cell_is_reached():
    got = fc.cells()
    missing = [c for c in fc.REQUIRED if not got.get(c)]
    assert not missing, f'no case of tests/fcnet_cases.py reaches {missing}'
    assert len([c for c in fc.REQUIRED if c[0] == 'actor']) == 24 and len([c for c in fc.REQUIRED if c[0] == 'policy set']) == 16
    assert len([c for c in fc.REQUIRED if c[0] == 'learner']) == 16


def test_a_case_taken_out_is_noticed(monkeypatch):
    """The 512-logit case alone reaches 16 logit tiles and 8 staging chunks; the 32-logit case alone the value's own tile."""
    monkeypatch.setattr(fc, 'ACTOR_SHAPES', [s for s in fc.ACTOR_SHAPES if s[:4] != ('central', 40, 8, 63)])
    got = fc.cells()
    assert {c for c in fc.REQUIRED if not got.get(c)} >= {('staging chunks', 8), ('logit tiles', 16)}
    monkeypatch.setattr(fc, 'ACTOR_SHAPES', [s for s in fc.ACTOR_SHAPES if s != ('multi', 5, 4, 31, 64)])
    assert not fc.cells().get(('N3 % 32 == 0 with the shared value',))
    monkeypatch.setattr(fc, 'LEARNER_SHAPES', [s for s in fc.LEARNER_SHAPES if s != ('central', 40, 8, 63, 32)])
    got = fc.cells()
    assert {c for c in fc.REQUIRED if not got.get(c)} >= {('learner: staging chunks', 8), ('learner: logit tiles', 16), ('learner', 1, 'tanh', False)}
    assert got[('wgrad_block', 1, 4)]                             # (dW1 of the other cases: another case covers it)


def test_the_limits_are_the_headers():
    import os
    import re
    hdr = open(os.path.join(fc.REPO, 'include', 'dcomp.h')).read() + open(os.path.join(fc.REPO, 'include', 'dcomp_types.h')).read()
    lim = {n: int(re.search(r'#define\s+%s\s+(\d+)' % n, hdr).group(1)) for n in ('DCOMP_ACTOR_MAX_IN', 'DCOMP_ACTOR_MAX_LOGITS', 'DCOMP_MAX_UE', 'DCOMP_MAX_BS')}
    d = fc.actor_dispatch('central', 8, 63, 32)
    assert lim['DCOMP_ACTOR_MAX_IN'] - 16 < d['K1'] <= lim['DCOMP_ACTOR_MAX_IN'] and d['N3'] == lim['DCOMP_ACTOR_MAX_LOGITS']
    assert lim['DCOMP_MAX_UE'] == 1024 and lim['DCOMP_MAX_BS'] == 64


# ------------------------------------------------------------------------------------------------------------ integer references
_INT_CASES = [(s, v) for s in fc.ACTOR_SHAPES for v in fc.INT_VARIANTS] + [(s, v) for s in fc.LOOP_SHAPES for v in fc.LOOP_VARIANTS] + \
    [(s, (1, False)) for s in fc.EPILOGUE_SHAPES]
_ACTOR_INT = {}


def _actor_int(shape, variant):
    if (shape, variant) not in _ACTOR_INT:
        _ACTOR_INT[shape, variant] = fc.actor_int_case(shape, *variant)          # (asserts hidden <= 82, logits and values <= 330)
    return _ACTOR_INT[shape, variant]


@pytest.mark.parametrize('shape,variant', _INT_CASES, ids=[f'{fc.sid(s)}-seed{v[0]}{"-wide" if v[1] else ""}' for s, v in _INT_CASES])
def test_actor_integer_references_are_exact_and_logp_emulation_is_inside_the_bound(shape, variant):
    """The float32 emulation of lse_push's sequence on the exact logits against float64 log-softmax at the first maximum: inside
    (NA + 8) 2^-24 max(1, max |logit|) -- the bound is reachable by a correct implementation."""
    c = _actor_int(shape, variant)
    B = shape[3]
    lg = c['logits'].reshape(c['rows'], -1, B + 1)
    assert np.array_equal(lg, np.round(lg))
    act = lg.argmax(-1)
    want = np.take_along_axis(fc.log_softmax64(lg), act[..., None], -1)[..., 0]
    err = np.abs(fc.logp_f32(lg, act).astype(np.float64) - want).max()
    bound = fc.lse_bound(B + 1, np.abs(lg).max())
    assert err <= bound, (err, bound)


def test_the_logits_go_past_the_float32_range_of_exp():
    """At least one case has max |logit| > 100 (expf overflows at 88.7): an implementation without the maximum subtracted cannot pass."""
    wide = [c for c in _INT_CASES if c[1][1]]
    worst = {(fc.sid(s), v): float(np.abs(_actor_int(s, v)['logits']).max()) for s, v in wide}
    assert min(worst.values()) > 100, worst                       # every shape has such a variant
    for s, v in wide:
        lg = _actor_int(s, v)['logits'].reshape(-1, s[3] + 1)
        assert (lg.max(-1) - lg.min(-1)).max() > 89                # within one head: exp(x - max) underflows, exp(x) overflows
        with np.errstate(over='ignore'):
            assert np.isinf(np.exp(lg.astype(np.float32))).any()


@pytest.mark.parametrize('shape', fc.LEARNER_SHAPES, ids=[fc.sid(s) for s in fc.LEARNER_SHAPES])
def test_learner_integer_references_are_exact(shape):
    """fc.learner_int_case asserts its own conditions while it builds the reference (seeds 1 and 2: the ones
    test_backward_integer_data_exact runs)."""
    kind, E, U, B, H = shape
    for seed in (1, 2):
        w, v, x, dl, dv, ref = fc.learner_int_case(kind, E, U, B, H, seed)
        again = fc.learner_int_reference(w, v, x, dl, dv)
        assert all(np.array_equal(ref[n], again[n]) for n in ref)
        assert any(np.abs(ref[n]).max() > 0 for n in ('w1', 'vw1'))


def test_mult2_integer_reference_is_exact():
    w, v, x, dl, dv, ref = fc.mult2_int_case(1)
    assert len(x) == 264250 and fc.row_split(len(x))['mult'] == 2
    assert (np.count_nonzero(dl, axis=1) <= 2).all() and set(np.unique(dl)) <= {-1.0, 0.0, 1.0}
    assert max(np.abs(ref[n]).max() for n in ref) < 2 ** 24 and np.abs(ref['w1']).max() > 0


# ------------------------------------------------------------------------------------------------------------ the loss epilogue
@pytest.mark.parametrize('run', list(fc.EPILOGUE_RUNS))
@pytest.mark.parametrize('shape', fc.EPILOGUE_SHAPES, ids=[fc.sid(s) for s in fc.EPILOGUE_SHAPES])
def test_epilogue_emulation_is_inside_the_bars(shape, run):
    c = fc.epilogue_case(shape)
    hy = fc.EPILOGUE_RUNS[run]
    adv = c['advantages'] if fc.EPILOGUE_ADV[run] else c['zero_adv']
    r64, r32, bars = fc.epilogue_f64(c, hy, adv), fc.epilogue_f32(c, hy, adv), fc.epilogue_bars(c)
    for k in ('logp', 'entropy', 'kl'):
        assert np.abs(r32[k].astype(np.float64) - r64[k]).max() <= bars[k], k
    assert (np.abs(r32['ratio'].astype(np.float64) - r64['ratio']) <= r64['ratio'] * bars['ratio_rel']).all()
    err, bound = fc.b3_gradient_check(r32['dlogits'].astype(np.float64).reshape(c['rows'], -1).mean(0), r64['dlogits'])
    assert (err <= bound).all(), (err.max(), bound.min())
    assert np.abs(r64['dlogits']).max() > 1e-3                    # (the run's term is alive)
    # the old policy's ratios fall on both sides of the clip
    assert r64['ratio'].min() < 0.7 and r64['ratio'].max() > 1.3
    # a wrong sign of the run's term is an error far outside the bar
    if run != 'all':
        flipped = dict(hy)
        key = {'kl': 'kl_coeff', 'entropy': 'entropy_coeff', 'surrogate': None}[run]
        if key:
            flipped[key] = -hy[key]
            wrong = fc.epilogue_f64(c, flipped, adv)['dlogits']
        else:
            wrong = fc.epilogue_f64(c, hy, -adv)['dlogits']
        e2, b2 = fc.b3_gradient_check(wrong.reshape(c['rows'], -1).mean(0), r64['dlogits'])
        assert (e2 > b2).any()
