"""The fcnet kernels' instantiations and host-side branches as a table of cases (tests/test_fcnet_matrix_cpu.py checks the table,
tests/test_fcnet_matrix_gpu.py runs it).

The kernels are template families -- actor_kernel<MT, RELU, VF, PER> (24 shared + 16 policy-set instantiations), learner_kernel<MT,
RELU, IDX> (16), wgrad_block<MB, NB> (4), wgrad_bias<NB> (2) -- and the host picks among them, and among loop counts inside them, from
the shape alone.  Which cell a shape reaches is the LIBRARY's answer: dcomp_fcnet_describe (deepcomp_amd/csrc/dcomp_fcnet_plan.h, the
one statement of that dispatch, which the create and launch functions read too) is asked here, so a changed formula moves the cases
and the CPU test says which cell lost its case.  The module lists the cases with the cells each one reaches, and builds the
references that need no device: the integer nets' float64 outputs with their exactness conditions, and float32 emulations of the
log-sum-exp walk and of the loss epilogue, which show that the stated bounds are reachable by a correct implementation.

To extend: a new template parameter or dispatch branch gets its number in the plan header, a cell in cells(), a line in REQUIRED, and
the smallest case that reaches it.  Pure numpy / torch on the CPU; nothing here touches the device (dcomp_fcnet_describe makes no
HIP call).

The shape tables and integer nets of the per-feature tests (tests/test_actor_gpu.py ... tests/test_learner_accum_gpu.py) are here too,
with HYPER, so that every file reads them from one place; what runs the device is in tests/fcnet_support.py, which imports this
module.  Neither imports a test module."""
import ctypes
import functools
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the host dispatch
def _i32(*names):
    return [(n, ctypes.c_int32) for n in names]


class _ActorPlan(ctypes.Structure):
    _fields_ = _i32('multi', 'hidden', 'K1', 'heads', 'N3', 'mt', 'Hp', 'KS2', 'K1p', 'NT3', 'NT3v', 'chunks', 'XS', 'lds_per_wave')


class _LearnerPlan(ctypes.Structure):
    _fields_ = _i32('K1pp', 'N3p') + [(n, ctypes.c_int32 * 6) for n in ('in_p', 'out_p', 'mb', 'nb', 'nmain', 'first_task')] + _i32('ntask') + \
        [(n, ctypes.c_int32 * 12) for n in ('nin', 'nout', 'off', 'len')] + _i32('total')


class _RowSplit(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ('tiles', 'rows_pad', 'mult', 'chunk_rows')] + _i32('nchunks')


class _Shape(ctypes.Structure):
    _fields_ = _i32('struct_size', 'obs_kind', 'num_ue', 'num_bs', 'hidden') + [('rows', ctypes.c_int64)] + _i32('compute_units')


class _Desc(ctypes.Structure):
    _fields_ = _i32('struct_size', 'TILE', 'WAVES', 'BLOCK', 'KC', 'LT', 'CHUNK_UNIT', 'MAX_CHUNKS', 'max_blocks', 'grid_tiles') + \
        [('actor', _ActorPlan), ('learner', _LearnerPlan), ('split', _RowSplit)]


@functools.lru_cache(maxsize=None)
def describe(kind, U, B, H, rows=0, cus=0):
    """dcomp_fcnet_describe of a shape (bound on first use; the struct sizes guard these mirrors): the library's own plan.
    rows: the row split of that many rows; cus: the device's compute units, 0 = the library's fallback."""
    from deepcomp_amd import _lib
    L = _lib.load()
    L.dcomp_fcnet_describe.argtypes = [ctypes.POINTER(_Shape), ctypes.POINTER(_Desc)]
    s = _Shape(ctypes.sizeof(_Shape), _lib.MULTI if kind == 'multi' else _lib.CENTRAL, U, B, H, rows, cus)
    d = _Desc(ctypes.sizeof(_Desc))
    _lib.check(L.dcomp_fcnet_describe(ctypes.byref(s), ctypes.byref(d)))
    return d


_ANY = ('multi', 1, 1, 32)                                    # the constants and the row split are the same for every shape
_CONSTANTS = ('KC', 'TILE', 'WAVES', 'CHUNK_UNIT', 'MAX_CHUNKS')


def grid_tiles(cus=256):
    """Tiles of one round of the persistent grid on a device of `cus` compute units (256: an MI355X)."""
    return describe(*_ANY, cus=cus).grid_tiles


def __getattr__(name):
    """fc.KC, fc.TILE, fc.WAVES, fc.CHUNK_UNIT, fc.MAX_CHUNKS: the library's; fc.GRID_TILES: of an MI355X."""
    if name in _CONSTANTS:
        return getattr(describe(*_ANY), name)
    if name == 'GRID_TILES':
        return grid_tiles()
    raise AttributeError(name)


def actor_dispatch(kind, U, B, H):
    a = describe(kind, U, B, H).actor
    return dict(multi=bool(a.multi), K1=a.K1, heads=a.heads, N3=a.N3, mt=a.mt, K1p=a.K1p, NT3=a.NT3, chunks=a.chunks, NT3v=a.NT3v, Hp=a.Hp)


def learner_dispatch(kind, U, B, H):
    """The six weight-gradient products dW1 dW2 dW3 | dvW1 dvW2 dwv."""
    p = describe(kind, U, B, H).learner
    return dict(actor_dispatch(kind, U, B, H), K1pp=p.K1pp, pairs=list(zip(p.in_p, p.out_p)), blocks=list(zip(p.mb, p.nb)), bias=list(p.nb))


def wgrad_mb(mi_tiles):
    """Of a product of mi_tiles (<= 8) input tiles: dW1 of a multi-agent net of 8 mi_tiles - 1 stations."""
    p = describe('multi', 1, 8 * mi_tiles - 1, 32).learner
    assert p.in_p[0] == 32 * mi_tiles
    return p.mb[0]


def wgrad_nb(ni_tiles):
    """Of a product of ni_tiles (<= 16) output tiles: dW3 of a central net of 16 ni_tiles UEs and one station."""
    p = describe('central', 16 * ni_tiles, 1, 32).learner
    assert p.out_p[2] == 32 * ni_tiles
    return p.nb[2]


def row_split(rows):
    s = describe(*_ANY, rows=rows).split
    return dict(mult=s.mult, chunk_rows=s.chunk_rows, nchunks=s.nchunks)


def rows_of(kind, E, U):
    return E * U if kind == 'multi' else E


def tiles_of(kind, E, U):
    return describe(*_ANY, rows=rows_of(kind, E, U)).split.tiles


# ------------------------------------------------------------------------------------------------------------ primitive builders
def dims(kind, U, B):
    from deepcomp_amd.actor import layer_shapes
    nin, heads, nout, _ = layer_shapes(kind, U, B, 32)
    return nin, heads, nout


def sparse_pm1(rng, nin, nout, nnz):
    """[nin, nout] with at most nnz entries of -1 / +1 per column at random positions."""
    w = np.zeros((nin, nout), dtype=np.float32)
    for c in range(nout):
        rows = rng.choice(nin, size=min(nnz, nin), replace=False)
        w[rows, c] = rng.choice([-1.0, 1.0], size=len(rows))
    return w


def int_weights(kind, U, B, H, seed):
    rng = np.random.default_rng(seed)
    nin, _, nout = dims(kind, U, B)
    ib = lambda n: rng.integers(-2, 3, size=n).astype(np.float32)      # noqa: E731
    return {'w1': sparse_pm1(rng, nin, H, 8), 'b1': ib(H), 'w2': sparse_pm1(rng, H, H, 8), 'b2': ib(H),
            'w3': sparse_pm1(rng, H, nout, 4), 'b3': ib(nout)}


def int_value_weights(kind, U, B, H, seed, form):
    rng = np.random.default_rng(1000 + seed)
    nin, _, _ = dims(kind, U, B)
    ib = lambda n: rng.integers(-2, 3, size=n).astype(np.float32)      # noqa: E731
    v = {'wv': sparse_pm1(rng, H, 1, 4)[:, 0], 'bv': ib(1)}
    if form == 'own':
        v.update({'w1': sparse_pm1(rng, nin, H, 8), 'b1': ib(H), 'w2': sparse_pm1(rng, H, H, 8), 'b2': ib(H)})
    return v


def obs_shape(kind, E, U, B):
    nin, _, _ = dims(kind, U, B)
    return (E, U, nin) if kind == 'multi' else (E, nin)


# ------------------------------------------------------------------------------------------------------------ the cases
ACTIVATIONS = ('relu', 'tanh')
VF_OF = {None: 0, 'own': 1, 'shared': 2}                      # the value form of a launch -> the kernel's VF
FORMS = ['own', 'shared']                                      # the value forms tests/test_critic_gpu.py runs

# tests/test_actor_gpu.py and test_critic_gpu.py: (kind, E, U, B, hidden): partial tile / K = 13; 256 wide; K = 129 and N = 33 cross a
# tile; K = 257 (two input chunks), N = 65, two mask words; central with 10 and 32 heads (K = 672: five chunks); more rows than one
# round of the grid's waves takes
BASE_SHAPES = [('multi', 3, 7, 3, 32), ('multi', 5, 32, 10, 256), ('multi', 9, 5, 32, 64), ('multi', 4, 6, 64, 256),
               ('central', 9, 10, 5, 256), ('central', 3, 32, 10, 64), ('multi', 1300, 32, 10, 256)]
# the persistent grid is at most two workgroups of four waves per CU (2 048 tiles a round on 256 CUs): 2 200 tiles of 32 rows
BASE_LOOP_SHAPE = ('multi', 2200, 32, 10, 32)
BASE_IDS = [f'{k}{e}x{u}x{b}h{h}' for k, e, u, b, h in BASE_SHAPES]

CHUNK = 2048                      # dcomp_learner.hip CHUNK_UNIT: rows of a weight-gradient chunk (while the batch has <= 128 of them)
# tests/test_learner_gpu.py: (kind, E, U, B, hidden); the last: 6 400 rows = three chunks and a partial one
LEARNER_BASE_SHAPES = [('multi', 3, 7, 3, 32), ('multi', 5, 32, 10, 256), ('multi', 9, 5, 32, 64), ('central', 9, 10, 5, 256),
                       ('central', 3, 32, 10, 64), ('multi', 4, 6, 10, 96), ('multi', 200, 32, 10, 256)]
LEARNER_BASE_IDS = [f'{k}{e}x{u}x{b}h{h}' for k, e, u, b, h in LEARNER_BASE_SHAPES]
assert 3 * CHUNK < 200 * 32 < 4 * CHUNK

# tests/test_policy_set_gpu.py: U, B, hidden, activation, E
SET_SHAPES = {'a': (5, 3, 32, 'tanh', 70), 'b': (3, 36, 64, 'relu', 33), 'c': (4, 10, 256, 'tanh', 40)}
SET_SLOTS = {'a': [0, 1, 1, 0, 1], 'b': [0, 1, 2], 'c': [0, 1, 2, 3]}
SET_GUARD = 97
SET_T = 5

# (kind, E, U, B, hidden).  Every one runs relu and tanh, without a value, with a trunk of its own and with the shared value.
ACTOR_SHAPES = [('multi', 3, 7, 3, 96), ('multi', 3, 7, 3, 128), ('multi', 3, 7, 3, 160), ('multi', 3, 7, 3, 224),      # MT 4 and 8, padded widths
                ('multi', 5, 4, 31, 64),           # 32 logits: a full last tile; shared value: column 32 alone in a second tile
                ('central', 40, 8, 63, 32),        # 1 016 inputs = 8 staging chunks, 512 logits = 16 tiles (17 with the value), rows 32 + 8
                ('central', 40, 8, 63, 128),
                ('multi', 4, 6, 64, 128),          # 64 stations at MT 4
                ('multi', 2, 1024, 3, 32),         # 1 024 UE slots
                ('multi', 3, 5, 35, 32)]           # added by the self-check: K1p == KC (141 inputs padded to 144), two logit tiles
COMPACT_SHAPE = ('multi', 2, 1024, 3, 32)          # rows and FragmentCodec.pack of them: bit-identical
NO_ACTIVE_SHAPE = ACTOR_SHAPES[0]
# the integer (relu) variants of a shape: (seed, wide head bias)
INT_VARIANTS = [(1, False), (2, True)]
LOOP_VARIANTS = [(1, True)]
# more tiles than one round of the persistent grid: relu, a value trunk of its own, the exact bar only.  Hidden 32 added by the
# self-check (every MT): it is tests/test_actor_gpu.py's LOOP_SHAPE with 3 stations.
LOOP_SHAPES = [('multi', 2200, 32, 3, H) for H in (32, 64, 128, 256)]

POLICY_SET = dict(U=5, B=3, E=70, slots=[0, 1, 1, 0, 1])      # shape (a) of tests/test_policy_set_gpu.py
POLICY_SET_HIDDEN = (32, 64, 128, 256)                        # x relu / tanh x members without a value / with a trunk of their own
POLICY_SET_WIDE = dict(U=1024, B=3, E=2, H=32, P=3)            # slot_policy[u] = u % 3: 1 024 tiles of two rows

LEARNER_SHAPES = [('multi', 3, 7, 5, 256),         # dW1 through wgrad_block<1, 4>
                  ('central', 40, 8, 63, 32),      # dW3 through <1, 4>, wgrad_bias<4> on D3, 16 logit tiles, 8 staging chunks
                  ('multi', 4, 6, 64, 128), ('multi', 3, 7, 3, 160), ('multi', 5, 4, 31, 64)]
MULT2_SHAPE = ('multi', 37750, 7, 3, 32)           # 264 250 rows: relu, exact
INDEXED = dict(kind='multi', E=16, U=5, B=4, T=2)  # x hidden 32 / 64 / 128 / 256 x relu / tanh, rows and compact
INDEXED_HIDDEN = (32, 64, 128, 256)
REUSE_SHAPE = ('multi', 200, 32, 10, 256)          # tests/test_learner_gpu.py's 6 400-row case
EPILOGUE_SHAPES = [('multi', 5, 32, 10, 64), ('central', 9, 10, 5, 64)]
# tests/test_learner_accum_gpu.py: (kind, E, U, B, hidden, T)
ACCUM_MULTI = ('multi', 101, 4, 5, 32, 16)      # 6 464 source rows
ACCUM_CENTRAL = ('central', 404, 10, 5, 64, 16)  # EPILOGUE_SHAPES[1]'s net: 6 464 source rows
assert EPILOGUE_SHAPES[1][0] == 'central' and EPILOGUE_SHAPES[1][2:] == ACCUM_CENTRAL[2:5]
ACCUM_ROWS = 6444                                # three full chunks and a partial one
ACCUM_LOCK = ('multi', 96, 4, 5, 32, 8)         # 3 072 rows: 1 536 per rank of two, 1 024 per rank of three


def sid(shape):
    k, e, u, b, h = shape
    return f'{k}{e}x{u}x{b}h{h}'


def cells():
    """{cell: [the cases that reach it]}.  A cell is a tuple that names a template instantiation or a dispatch branch."""
    out = {}

    def reach(cell, case):
        out.setdefault(cell, []).append(case)
    for shape in ACTOR_SHAPES:
        kind, E, U, B, H = shape
        d = actor_dispatch(kind, U, B, H)
        for act in ACTIVATIONS:
            for form, vf in VF_OF.items():
                reach(('actor', d['mt'], act, vf), sid(shape))
        reach(('staging chunks', d['chunks']), sid(shape))
        reach(('logit tiles', d['NT3']), sid(shape))
        reach(('hidden', H), sid(shape))
        if d['K1p'] == describe(*_ANY).KC:
            reach(('K1p == KC',), sid(shape))
        if d['N3'] % 32 == 0:
            assert d['NT3v'] == d['NT3'] + 1, f"{sid(shape)}: ('N3 % 32 == 0 with the shared value',) needs a tile of its own for the value, NT3v {d['NT3v']}"
            reach(('N3 % 32 == 0 with the shared value',), sid(shape))
        reach(('num_ue', U), sid(shape))
        reach(('num_bs', B), sid(shape))
    for shape in LOOP_SHAPES:
        kind, E, U, B, H = shape
        d = actor_dispatch(kind, U, B, H)
        reach(('actor', d['mt'], 'relu', 1), sid(shape))
        if tiles_of(kind, E, U) > grid_tiles():
            reach(('actor: more tiles than one round of the grid', d['mt']), sid(shape))
    ps = POLICY_SET
    for H in POLICY_SET_HIDDEN:
        d = actor_dispatch('multi', ps['U'], ps['B'], H)
        for act in ACTIVATIONS:
            for vf in (0, 1):
                reach(('policy set', d['mt'], act, vf), f'set h{H} {act} vf{vf}')
    pw = POLICY_SET_WIDE
    d = actor_dispatch('multi', pw['U'], pw['B'], pw['H'])
    reach(('policy set', d['mt'], 'tanh', 1), 'set 1024')
    reach(('policy set: num_ue', pw['U']), 'set 1024')
    for shape in LEARNER_SHAPES + [MULT2_SHAPE]:
        kind, E, U, B, H = shape
        d = learner_dispatch(kind, U, B, H)
        for act in (ACTIVATIONS if shape != MULT2_SHAPE else ('relu',)):
            reach(('learner', d['mt'], act, False), sid(shape))
        for blk in d['blocks']:                                # every case runs relu under the exact bar
            reach(('wgrad_block',) + blk, sid(shape))
        for nb in d['bias']:
            reach(('wgrad_bias', nb), sid(shape))
        reach(('mult', row_split(rows_of(kind, E, U))['mult']), sid(shape))
        reach(('learner: staging chunks', d['chunks']), sid(shape))
        reach(('learner: logit tiles', d['NT3']), sid(shape))
        reach(('learner: num_bs', B), sid(shape))
        if tiles_of(kind, E, U) > grid_tiles():
            reach(('learner: more tiles than one round of the grid', d['mt']), sid(shape))
    ix = INDEXED
    for H in INDEXED_HIDDEN:
        d = learner_dispatch(ix['kind'], ix['U'], ix['B'], H)
        for act in ACTIVATIONS:
            reach(('learner', d['mt'], act, True), f'indexed h{H} {act}')
    return out


REQUIRED = ([('actor', mt, act, vf) for mt in (1, 2, 4, 8) for act in ACTIVATIONS for vf in (0, 1, 2)] +
            [('policy set', mt, act, vf) for mt in (1, 2, 4, 8) for act in ACTIVATIONS for vf in (0, 1)] +
            [('learner', mt, act, idx) for mt in (1, 2, 4, 8) for act in ACTIVATIONS for idx in (False, True)] +
            [('wgrad_block', mb, nb) for mb in (1, 2) for nb in (1, 4)] + [('wgrad_bias', 1), ('wgrad_bias', 4)] +
            [('staging chunks', 1), ('staging chunks', 2), ('staging chunks', 8), ('K1p == KC',)] +
            [('logit tiles', n) for n in (1, 2, 3, 16)] + [('N3 % 32 == 0 with the shared value',)] +
            [('mult', 1), ('mult', 2)] + [('hidden', H) for H in (96, 128, 160, 224)] +
            [('num_ue', 1024), ('policy set: num_ue', 1024), ('num_bs', 64), ('learner: num_bs', 64)] +
            [('learner: staging chunks', 8), ('learner: logit tiles', 16)] +
            [('actor: more tiles than one round of the grid', mt) for mt in (1, 2, 4, 8)])


# ------------------------------------------------------------------------------------------------------------ integer nets
WIDE_B3 = 150


def actor_int_case(shape, seed, wide=False):
    """tests/test_actor_gpu.py's integer net (relu, inputs in {0, 1}, sparse +-1 weights, integer biases in [-2, 2]) with both value
    forms of tests/test_critic_gpu.py; the float64 logits and values with the exactness conditions those tests assert: hidden
    magnitudes <= 82 (exact in bf16), logits and values <= 330 (exact in f32).
    wide: b3 drawn from the integers in [-150, 150] instead.  As the recipe stands its logits stay below 34 at every shape of the
    table (the 330 is the worst case of the construction, never met), inside expf's float32 range; with the wide head bias the
    logits of one head lie more than 88.7 apart and reach past +-100, and they are still integers below 2^24: exact."""
    kind, E, U, B, H = shape
    rows = rows_of(kind, E, U)
    w = int_weights(kind, U, B, H, seed)
    if wide:
        w['b3'] = np.random.default_rng(700 + seed).integers(-WIDE_B3, WIDE_B3 + 1, size=w['b3'].shape).astype(np.float32)
    x = np.random.default_rng(100 + seed).integers(0, 2, size=obs_shape(kind, E, U, B)).astype(np.float32)
    x2 = x.reshape(rows, -1).astype(np.float64)
    out = dict(w=w, x=x, rows=rows, v={}, vf={})

    def trunk(t):
        h = np.maximum(x2 @ t['w1'] + t['b1'], 0)
        h = np.maximum(h @ t['w2'] + t['b2'], 0)
        assert np.abs(h).max() <= 82
        return h
    h = trunk(w)
    out['logits'] = h @ w['w3'] + w['b3']
    assert np.abs(out['logits']).max() <= 330
    for form in ('own', 'shared'):
        v = int_value_weights(kind, U, B, H, seed, form)
        hv = trunk(v) if form == 'own' else h
        out['v'][form] = v
        out['vf'][form] = hv @ v['wv'].astype(np.float64) + float(v['bv'][0])
        assert np.count_nonzero(v['wv']) <= 4 and np.abs(out['vf'][form]).max() <= 330
    return out


def learner_int_reference(w, v, x, dl, dv):
    """The float64 reference of all twelve gradients from upstream gradients, with the conditions learner_int_case
    asserts (integers of magnitude <= 256 everywhere, every sum below 2^24: exact in f32 in any order)."""
    grads = {}
    x = x.astype(np.float64)
    rows, H = len(x), w['w1'].shape[1]

    def trunk(t, w3, d3, names):
        h1 = np.maximum(x @ t['w1'] + t['b1'], 0)
        h2 = np.maximum(h1 @ t['w2'] + t['b2'], 0)
        d2 = (d3 @ w3.T) * (h2 > 0)
        d1 = (d2 @ t['w2'].astype(np.float64).T) * (h1 > 0)
        for a in (h1, h2, d1, d2, d3):
            assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= 256
        for (a, d), (wn, bn) in zip(((x, d1), (h1, d2), (h2, d3)), names):
            assert (np.abs(a).T @ np.abs(d)).max() < 2 ** 24
            assert np.abs(d).sum(0).max() < 2 ** 24
            grads[wn], grads[bn] = a.T @ d, d.sum(0)
    trunk(w, w['w3'].astype(np.float64), dl.astype(np.float64), (('w1', 'b1'), ('w2', 'b2'), ('w3', 'b3')))
    trunk(v, v['wv'].astype(np.float64).reshape(H, 1), dv.astype(np.float64).reshape(rows, 1), (('vw1', 'vb1'), ('vw2', 'vb2'), ('wv', 'bv')))
    grads['wv'] = grads['wv'].reshape(-1)
    return grads


def learner_int_case(kind, E, U, B, H, seed):
    """relu, inputs in {0, 1}, sparse +-1 weights and small integer biases in both trunks, dlogits with <= 2 entries of +-1 per row,
    dvalue in {-1, 0, 1}; the float64 reference of all twelve gradients, with both exactness bounds asserted."""
    rng = np.random.default_rng(500 + seed)
    rows = rows_of(kind, E, U)
    nin, _, n3 = dims(kind, U, B)
    w, v = int_weights(kind, U, B, H, seed), int_value_weights(kind, U, B, H, seed, 'own')
    x = rng.integers(0, 2, size=(rows, nin)).astype(np.float64)
    dl = np.zeros((rows, n3))
    for r in range(rows):
        cols = rng.choice(n3, size=min(2, n3), replace=False)
        dl[r, cols] = rng.choice([-1.0, 0.0, 1.0], size=len(cols))
    dv = rng.integers(-1, 2, size=rows).astype(np.float64)
    grads = {}

    def trunk(t, w3, d3, names):
        h1 = np.maximum(x @ t['w1'] + t['b1'], 0)
        h2 = np.maximum(h1 @ t['w2'] + t['b2'], 0)
        d2 = (d3 @ w3.T) * (h2 > 0)
        d1 = (d2 @ t['w2'].astype(np.float64).T) * (h1 > 0)
        for a in (h1, h2, d1, d2, d3):
            assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= 256          # integers, exact in bf16
        for (a, d), (wn, bn) in zip(((x, d1), (h1, d2), (h2, d3)), names):
            assert (np.abs(a).T @ np.abs(d)).max() < 2 ** 24                          # exact in f32 in any order
            assert np.abs(d).sum(0).max() < 2 ** 24
            grads[wn], grads[bn] = a.T @ d, d.sum(0)
    trunk(w, w['w3'].astype(np.float64), dl, (('w1', 'b1'), ('w2', 'b2'), ('w3', 'b3')))
    trunk(v, v['wv'].astype(np.float64).reshape(H, 1), dv.reshape(rows, 1), (('vw1', 'vb1'), ('vw2', 'vb2'), ('wv', 'bv')))
    grads['wv'] = grads['wv'].reshape(-1)
    return w, v, x.astype(np.float32), dl.astype(np.float32), dv.astype(np.float32), grads


def mult2_int_case(seed=1):
    """learner_int_case for MULT2_SHAPE with dlogits built vectorised (two distinct columns per row, entries in
    {-1, 0, 1}) instead of row by row: (weights, value weights, x, dlogits, dvalue, the twelve float64 gradients)."""
    kind, E, U, B, H = MULT2_SHAPE
    rng = np.random.default_rng(500 + seed)
    rows = rows_of(kind, E, U)
    nin, _, n3 = dims(kind, U, B)
    w, v = int_weights(kind, U, B, H, seed), int_value_weights(kind, U, B, H, seed, 'own')
    x = rng.integers(0, 2, size=(rows, nin)).astype(np.float32)
    c0 = rng.integers(0, n3, size=rows)
    c1 = (c0 + 1 + rng.integers(0, n3 - 1, size=rows)) % n3
    dl = np.zeros((rows, n3), dtype=np.float32)
    r = np.arange(rows)
    dl[r, c0] = rng.integers(-1, 2, size=rows)
    dl[r, c1] = rng.integers(-1, 2, size=rows)
    dv = rng.integers(-1, 2, size=rows).astype(np.float32)
    return w, v, x, dl, dv, learner_int_reference(w, v, x, dl, dv)


# ------------------------------------------------------------------------------------------------------------ log-sum-exp
def log_softmax64(lg):
    lg = np.asarray(lg, dtype=np.float64)
    m = lg.max(-1, keepdims=True)
    return lg - (np.log(np.exp(lg - m).sum(-1, keepdims=True)) + m)


def lse_bound(num_actions, max_abs_logit):
    """(NA + 8) 2^-24 max(1, max |logit|) per head: NA rescale-and-add steps of the online sum, each a few roundings at the
    magnitude of the logits, plus expf, logf and the final subtraction (tests/test_actor_gpu.py's
    test_logp_is_log_softmax_of_chosen_action, with the magnitude no longer capped at 10)."""
    return (num_actions + 8) * 2.0 ** -24 * max(1.0, float(max_abs_logit))


def lse_walk_f32(lg):
    """dcomp_actor_impl.h's lse_push over the last axis in float32, column by column as the kernels walk it, with the sum tn that
    rides along in the learner (tn = tn e1 + x e2): (mx, sm, tn)."""
    f = np.float32
    lg = np.asarray(lg, dtype=f)
    mx = np.full(lg.shape[:-1], -np.inf, dtype=f)
    sm, tn = np.zeros(lg.shape[:-1], dtype=f), np.zeros(lg.shape[:-1], dtype=f)
    with np.errstate(invalid='ignore'):
        for c in range(lg.shape[-1]):
            x = lg[..., c]
            m2 = np.maximum(mx, x)
            e1 = np.where(np.isneginf(mx), f(0), np.exp((mx - m2).astype(f))).astype(f)      # expf(-inf) = 0
            e2 = np.exp((x - m2).astype(f)).astype(f)
            sm = (sm * e1).astype(f) + e2
            tn = (tn * e1).astype(f) + (x * e2).astype(f)
            mx = m2
    return mx, sm.astype(f), tn.astype(f)


def logp_f32(lg, actions):
    """The actor's logp of `actions` [..]: x_a - (mx + logf(sm)) in float32."""
    f = np.float32
    mx, sm, _ = lse_walk_f32(lg)
    xa = np.take_along_axis(np.asarray(lg, dtype=f), actions[..., None].astype(np.int64), -1)[..., 0]
    return (xa - (mx + np.log(sm).astype(f)).astype(f)).astype(f)


# ------------------------------------------------------------------------------------------------------------ the loss epilogue
RATIOS = (1.7, 0.5, 0.85, 1.15)            # tests/test_learner_gpu.py's: row i's ratio, i % 4
VF_SHIFT = (0.2, -0.02, -0.2, 0.02)
HYPER = dict(clip_param=0.3, vf_clip_param=0.05, vf_loss_coeff=1.0, entropy_coeff=0.01, kl_coeff=0.2)
# one term of dlogits alive at a time, then all three
EPILOGUE_RUNS = {'kl': dict(HYPER, entropy_coeff=0.0), 'entropy': dict(HYPER, kl_coeff=0.0), 'surrogate': dict(HYPER, kl_coeff=0.0, entropy_coeff=0.0),
                 'all': dict(HYPER)}
EPILOGUE_ADV = {'kl': False, 'entropy': False, 'surrogate': True, 'all': True}      # advantages != 0


def epilogue_case(shape, seed=1):
    """The relu integer net of a shape driven through the REAL loss.  The forward pass is exact, so the float64 reference of every
    per-row output follows from the integer logits alone: actions random, old_logits = logits + integer noise in [-3, 3], old_logp =
    float64 logp - log(RATIOS[i % 4]) / heads, advantages and value inputs as tests/fcnet_support.py's old_policy_inputs places
    them (around the exact value here)."""
    kind, E, U, B, H = shape
    c = actor_int_case(shape, seed)
    rows, NA = c['rows'], B + 1
    heads = c['logits'].shape[1] // NA
    rng = np.random.default_rng(900 + seed)
    lg = c['logits'].reshape(rows, heads, NA)
    actions = rng.integers(0, NA, size=(rows, heads)).astype(np.uint8)
    old = (lg + rng.integers(-3, 4, size=lg.shape)).astype(np.float32)
    lsm = log_softmax64(lg)
    logp = np.take_along_axis(lsm, actions[..., None].astype(np.int64), -1)[..., 0]
    i = np.arange(rows)
    old_logp = (logp - np.log(np.array(RATIOS))[i % 4, None] / heads).astype(np.float32)
    v = c['vf']['own']
    old_vf = (v + np.array(VF_SHIFT)[i % 4]).astype(np.float32)
    adv = ((np.abs(rng.normal(size=rows)) + 0.1) * np.where(i % 8 < 4, 1.0, -1.0)).astype(np.float32)
    vt = np.where(i % 4 == 0, v - 0.3, np.where(i % 4 == 2, v - 0.4, v + rng.normal(size=rows) * 0.3)).astype(np.float32)
    return dict(c, heads=heads, NA=NA, lg=lg, actions=actions, old_logits=old.reshape(rows, -1), old_logp=old_logp, old_vf=old_vf,
                advantages=adv, value_targets=vt, zero_adv=np.zeros(rows, dtype=np.float32))


def epilogue_f64(c, hyper, adv):
    """Float64: logp [rows, heads], entropy, kl, ratio [rows], dlogits [rows, heads, NA] of the loss's policy part (per row, before
    the 1 / N), from the exact logits and the float32 inputs as given."""
    lg, old = c['lg'], c['old_logits'].astype(np.float64).reshape(c['lg'].shape)
    lsm, lso = log_softmax64(lg), log_softmax64(old)
    p, po = np.exp(lsm), np.exp(lso)
    a = c['actions'][..., None].astype(np.int64)
    logp = np.take_along_axis(lsm, a, -1)[..., 0]
    ent_h = -(p * lsm).sum(-1)
    kl = (po * (lso - lsm)).sum(-1).sum(1)
    ratio = np.exp(logp.sum(1) - c['old_logp'].astype(np.float64).sum(1))
    adv = adv.astype(np.float64)
    s1, s2 = adv * ratio, adv * np.clip(ratio, 1 - hyper['clip_param'], 1 + hyper['clip_param'])
    c_lp = np.where(s1 <= s2, -s1, 0.0)
    onehot = np.zeros_like(p)
    np.put_along_axis(onehot, a, 1.0, -1)
    dl = c_lp[:, None, None] * (onehot - p) + hyper['kl_coeff'] * (p - po) + hyper['entropy_coeff'] * (p * (lsm + ent_h[..., None]))
    return dict(logp=logp, entropy=ent_h.sum(1), kl=kl, ratio=ratio, dlogits=dl)


def _bf16_f32(a):
    """float32 -> bfloat16 (round to nearest even) -> float32, as dcomp_actor_impl.h's bf16_rne."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    u = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) << np.uint32(16)
    return u.view(np.float32)


def epilogue_f32(c, hyper, adv):
    """The learner kernel's two walks in float32, operation by operation (dcomp_learner.hip, learner_kernel): the same outputs as
    epilogue_f64, dlogits rounded to bf16 as the kernel stores them for the weight gradients."""
    f = np.float32
    lg = c['lg'].astype(f)
    old = c['old_logits'].astype(f).reshape(lg.shape)
    a = c['actions'][..., None].astype(np.int64)
    mx, sm, tn = lse_walk_f32(lg)
    mo, so, _ = lse_walk_f32(old)
    lse = (mx + np.log(sm).astype(f)).astype(f)
    xa = np.take_along_axis(lg, a, -1)[..., 0]
    lp = (xa - lse).astype(f)
    eh = (lse - (tn / sm).astype(f)).astype(f)
    lse_o = (mo + np.log(so).astype(f)).astype(f)
    logp_sum, old_sum, ent_sum = np.zeros(len(lg), dtype=f), np.zeros(len(lg), dtype=f), np.zeros(len(lg), dtype=f)
    for hd in range(lg.shape[1]):
        logp_sum = (logp_sum + lp[:, hd]).astype(f)
        ent_sum = (ent_sum + eh[:, hd]).astype(f)
        old_sum = (old_sum + c['old_logp'][:, hd].astype(f)).astype(f)
    ratio = np.exp((logp_sum - old_sum).astype(f)).astype(f)
    adv = adv.astype(f)
    s1 = (adv * ratio).astype(f)
    s2 = (adv * np.minimum(np.maximum(ratio, f(1.0) - f(hyper['clip_param'])), f(1.0) + f(hyper['clip_param']))).astype(f)
    c_lp = np.where(s1 <= s2, -s1, f(0)).astype(f)
    klc, entc = f(hyper['kl_coeff']), f(hyper['entropy_coeff'])
    lpn = (lg - lse[..., None]).astype(f)
    pn = np.exp(lpn).astype(f)
    lpo = (old - lse_o[..., None]).astype(f)
    po = np.exp(lpo).astype(f)
    kl = np.zeros(len(lg), dtype=f)
    for hd in range(lg.shape[1]):
        for col in range(lg.shape[2]):
            kl = (kl + (po[:, hd, col] * (lpo[:, hd, col] - lpn[:, hd, col]).astype(f)).astype(f)).astype(f)
    onehot = np.zeros_like(pn)
    np.put_along_axis(onehot, a, f(1), -1)
    dl = ((c_lp[:, None, None] * (onehot - pn).astype(f)).astype(f) + (klc * (pn - po).astype(f)).astype(f)).astype(f)
    dl = (dl + (entc * (pn * (lpn + eh[..., None]).astype(f)).astype(f)).astype(f)).astype(f)
    return dict(logp=lp, entropy=ent_sum, kl=kl, ratio=ratio, dlogits=_bf16_f32(dl))


def epilogue_bars(c):
    """The per-row bars: b per head, then logp b, entropy and kl 2 heads b (each a difference of two such quantities, summed over
    the heads), ratio relative heads b + 2^-22."""
    b = lse_bound(c['NA'], np.abs(c['lg']).max())
    return dict(b=b, logp=b, entropy=2 * c['heads'] * b, kl=2 * c['heads'] * b, ratio_rel=c['heads'] * b + 2.0 ** -22)


def b3_gradient_check(dl_got_mean, dl64):
    """db3 per column against the float64 mean of dlogits: 2^-8 mean_r |dlogit64| + 1e-6.  The kernel rounds each dlogit to bf16
    (half an ulp is 2^-9 relative); the factor 2 covers the f32 dlogit's own error.  Returns (error, bound) per column."""
    d = dl64.reshape(len(dl64), -1)
    return np.abs(np.asarray(dl_got_mean, dtype=np.float64) - d.mean(0)), 2.0 ** -8 * np.abs(d).mean(0) + 1e-6
