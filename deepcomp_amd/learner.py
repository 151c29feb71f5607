"""The PPO learner of the fcnet policy on the device (include/dcomp_learner.h): loss, backward pass and Adam on the train batch
``sampler.collect`` leaves in HBM, writing the new weights straight into the actor's handle.

    actor = FcnetActor('multi', U, B, weights, value_weights=value_weights)        # a value trunk of its own
    learner = PPOLearner(actor, lr=5e-5, max_rows=rows_per_minibatch)
    for _ in range(iters):
        batch = collect(env, actor, num_steps=50, gamma=0.99, lam=0.95, dist_inputs=True)
        stats = learner.update(batch, num_sgd_iter=30, minibatch_rows=rows_per_minibatch)
    rllib_weights = learner.to_rllib_weights()

Supported: ``multi`` and ``central``, tanh and relu, every hidden width the actor takes, the value function as a trunk of its own
(``vf_share_layers=False``, PPO's default); ``update`` takes the batch as observation rows or as the compact record
(``collect(compact=True)``, multi), whose minibatches it picks through a row index (``grads_indexed``): from a compact batch no
observation row is ever written.  The shared value function is refused (NotImplementedError), and so is the
compact record by ``grads`` / ``evaluate``, which take a contiguous minibatch of rows.  Envs with UE arrival / departure: ``collect(..., by_ue=True)`` marks the rows that count
(a slot is not one UE there) and ``update(batch, rows=sampler.live_rows(batch))`` trains on them; the learner itself needed no change.
``accumulate`` / ``accumulate_indexed`` / ``finish`` (include/dcomp_learner_accum.h) keep the unnormalised gradient as a running
sum in a buffer of the caller's: ``update(micro_rows=, grad_clip=)`` trains minibatches larger than the handle micro-batch by micro-batch and
clips by the global norm, and deepcomp_amd.dp_learner sums the buffer across the ranks of a data-parallel learner.

The arithmetic is the specification, spelled out here in torch / numpy on the CPU: ``ppo_loss_reference`` (RLlib's
ppo_surrogate_loss and its gradients, as the float64 model and as the bf16 chain the kernels implement) and ``adam_reference``
(torch.optim.Adam as pinned float32 operations)."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .actor import FcnetActor, _bf16

ARRAYS = _lib.LEARNER_ARRAYS
_POLICY, _VALUE = ARRAYS[:6], ARRAYS[6:]
_VALUE_KEYS = ('w1', 'b1', 'w2', 'b2', 'wv', 'bv')            # FcnetActor.value_weights' names of vw1 ... bv
DEFAULT_HYPER = {'clip_param': 0.3, 'vf_clip_param': 10.0, 'vf_loss_coeff': 1.0, 'entropy_coeff': 0.0, 'kl_coeff': 0.2}
STATS = _lib.PPO_STATS


def join_weights(weights, value_weights, dtype=np.float32):
    """The twelve arrays of a learner from FcnetActor.weights and FcnetActor.value_weights (a trunk of its own)."""
    out = {n: np.asarray(weights[n], dtype=dtype) for n in _POLICY}
    out.update({a: np.asarray(value_weights[k], dtype=dtype).reshape(-1) if k in ('wv', 'bv') else np.asarray(value_weights[k], dtype=dtype)
                for a, k in zip(_VALUE, _VALUE_KEYS)})
    return out


def split_weights(arrays):
    """The inverse of join_weights: (weights, value_weights)."""
    return {n: arrays[n] for n in _POLICY}, {k: arrays[a] for a, k in zip(_VALUE, _VALUE_KEYS)}


def _act(activation):
    return torch.tanh if activation == 'tanh' else torch.relu


def _dact(activation, h):
    """The activation's derivative from its OUTPUT h (the stored activation): tanh 1 - h^2, relu h > 0."""
    return 1 - h * h if activation == 'tanh' else (h > 0).to(h.dtype)


def _row_terms(logits, v, b, hy):
    """Per-row terms of RLlib's ppo_surrogate_loss on the heads that count.  logits [R, heads, A], v [R]; b: actions [R, heads]
    (int64), old_logp [R, heads], old_logits [R, heads, A], advantages, value_targets, old_vf [R]."""
    lsm = torch.log_softmax(logits, -1)
    lso = torch.log_softmax(b['old_logits'], -1)
    p, po = lsm.exp(), lso.exp()
    logp_h = lsm.gather(-1, b['actions'].unsqueeze(-1)).squeeze(-1)
    logp = logp_h.sum(1)
    ratio = (logp - b['old_logp'].sum(1)).exp()
    adv = b['advantages']
    s1, s2 = adv * ratio, adv * ratio.clamp(1 - hy['clip_param'], 1 + hy['clip_param'])
    ent_h = -(p * lsm).sum(-1)
    kl = (po * (lso - lsm)).sum(-1).sum(1)
    d1 = v - b['value_targets']
    d2 = b['old_vf'] + (v - b['old_vf']).clamp(-hy['vf_clip_param'], hy['vf_clip_param']) - b['value_targets']
    return {'logp_h': logp_h, 'ratio': ratio, 's1': s1, 's2': s2, 'surr': torch.minimum(s1, s2), 'kl': kl, 'ent_h': ent_h, 'ent': ent_h.sum(1),
            'd1': d1, 'd2': d2, 'vf_loss': torch.maximum(d1 * d1, d2 * d2), 'p': p, 'po': po, 'lsm': lsm}


def ppo_loss_reference(weights, value_weights, batch, hyper=None, activation='tanh', form='float64', round_weights=True):
    """RLlib's ppo_surrogate_loss and its gradients with respect to the twelve arrays, on the CPU.

    weights / value_weights: FcnetActor.weights / .value_weights (a value trunk of its own).  batch: a dict of arrays -- obs
    [rows, inputs], actions [rows, heads], old_logp [rows, heads], old_logits [rows, logits], advantages, value_targets, old_vf
    [rows]; optional num_active with num_ue (multi: rows whose slot row % num_ue is >= num_active contribute nothing and are not
    counted; central: heads >= num_active are left out of logp, kl and the entropy); optional dlogits [rows, logits] with dvalue
    [rows]: upstream gradients used instead of the loss's (no statistics, no 1 / N).  hyper: clip_param, vf_clip_param,
    vf_loss_coeff, entropy_coeff, kl_coeff (RLlib's defaults where absent).

    Per counted row: logp = sum over heads of log_softmax(logits_head)[action]; ratio = exp(logp - sum old_logp); surr =
    min(adv ratio, adv clip(ratio, 1 - eps, 1 + eps)); kl = sum KL(old || new); ent = sum H(new); vf_loss = max((v - vt)^2,
    (old_v + clip(v - old_v, +-vf_clip) - vt)^2); loss = mean(-surr + kl_coeff kl + vf_loss_coeff vf_loss - entropy_coeff ent).

    form='float64': the model.  Weights and inputs rounded to bf16 as in reference_logits_of(form='float64'), everything else in
    float64, gradients from autograd.  (round_weights=False, float64 only: the weights are taken as they come, in float64 -- for
    finite differences of the model's own loss, which must be able to move a weight by less than a bf16 step.)
    form='bf16': the chain the kernels implement, by hand.  Forward = reference_logits_of / reference_value_of(form='bf16'); per-row
    terms, dlogits and dv in f32; backward matrix products with bf16 operands (dlogits, dA2 = (dlogits W3^T) * act'(h2), dA1,
    each rounded to bf16 where it becomes an operand; act' from the stored bf16 h) and f32 sums; dW = a^T d; db = column sums of
    the bf16 d; the 1 / N of the mean once, in f32, after the sum over rows.

    Returns (stats, grads, rows): stats total_loss, policy_loss (= -mean surr), vf_loss, kl, entropy; grads the twelve arrays
    (numpy); rows the per-row tensors logp [rows, heads], ratio, surr, kl, entropy, vf_loss, vf, and which of the two branches of
    surr / vf_loss each row took (clipped, vf_clipped) -- rows that do not count hold zeros."""
    if form not in ('float64', 'bf16'):
        raise ValueError("form is 'bf16' or 'float64'")
    hy = dict(DEFAULT_HYPER)
    hy.update(hyper or {})
    dt = torch.float64 if form == 'float64' else torch.float32
    if not round_weights and form != 'float64':
        raise ValueError("round_weights=False goes with form='float64'")
    arrays = join_weights(weights, value_weights, np.float32 if round_weights else np.float64)
    nin, H = arrays['w1'].shape
    N3 = arrays['w3'].shape[1]
    upstream = batch.get('dlogits') is not None
    obs = np.asarray(batch['obs'], dtype=np.float32).reshape(-1, nin)
    R = obs.shape[0]
    if upstream:
        heads = 1
    else:
        actions = torch.as_tensor(np.asarray(batch['actions']).astype(np.int64)).reshape(R, -1)
        heads = actions.shape[1]
    A = N3 // heads
    na, U = batch.get('num_active'), batch.get('num_ue')
    live = np.ones(R, dtype=bool)
    head_count = heads
    if na is not None:
        if heads == 1 and U is not None:                                   # multi: whole rows drop out
            live = (np.arange(R) % int(U)) < int(na)
        elif heads > 1:
            head_count = int(na)
    idx = torch.as_tensor(np.nonzero(live)[0])
    N = int(live.sum())
    act = _act(activation)

    x = _bf16(torch.as_tensor(obs[live])).to(dt)
    leaf = {}
    for n in ARRAYS:
        t = torch.as_tensor(arrays[n])
        t = (_bf16(t) if round_weights and n[-2] == 'w' else t).to(dt)
        leaf[n] = t.clone().requires_grad_(form == 'float64')
    rnd = (lambda t: t) if form == 'float64' else _bf16

    def trunk(w1, b1, w2, b2):
        h1 = rnd(act(x @ leaf[w1] + leaf[b1]))
        h2 = rnd(act(h1 @ leaf[w2] + leaf[b2]))
        return h1, h2
    h1, h2 = trunk('w1', 'b1', 'w2', 'b2')
    logits = h2 @ leaf['w3'] + leaf['b3']
    g1, g2 = trunk('vw1', 'vb1', 'vw2', 'vb2')
    v = g2 @ leaf['wv'] + leaf['bv'][0]

    stats = {n: 0.0 for n in STATS}
    rows = {}
    if upstream:
        dl = torch.as_tensor(np.asarray(batch['dlogits'], dtype=np.float32).reshape(R, N3)[live]).to(dt)
        dv = torch.as_tensor(np.asarray(batch['dvalue'], dtype=np.float32).reshape(R)[live]).to(dt)
        scale = 1.0
        if form == 'float64':
            ((logits * dl).sum() + (v * dv).sum()).backward()
    else:
        hc = head_count
        f = lambda k, shape: torch.as_tensor(np.asarray(batch[k], dtype=np.float32).reshape(shape)[live]).to(dt)      # noqa: E731
        b = {'actions': actions[idx][:, :hc], 'old_logp': f('old_logp', (R, heads))[:, :hc], 'old_logits': f('old_logits', (R, heads, A))[:, :hc],
             'advantages': f('advantages', (R,)), 'value_targets': f('value_targets', (R,)), 'old_vf': f('old_vf', (R,))}
        lg = logits.reshape(N, heads, A)[:, :hc]
        t = _row_terms(lg, v, b, hy)
        scale = 1.0 / N if N else 0.0
        pol, kl, ent, vfl = -t['surr'].sum() * scale, t['kl'].sum() * scale, t['ent'].sum() * scale, t['vf_loss'].sum() * scale
        total = pol + hy['kl_coeff'] * kl + hy['vf_loss_coeff'] * vfl - hy['entropy_coeff'] * ent
        stats = {n: float(t_.detach()) for n, t_ in zip(STATS, (total, pol, vfl, kl, ent))}
        full = lambda src, shape: torch.zeros(shape, dtype=dt).index_copy_(0, idx, src.detach())      # noqa: E731
        logp_full = torch.zeros((R, heads), dtype=dt)
        logp_full[idx, :hc] = t['logp_h'].detach()
        rows = {'logp': logp_full, 'ratio': full(t['ratio'], (R,)), 'surr': full(t['surr'], (R,)), 'kl': full(t['kl'], (R,)),
                'entropy': full(t['ent'], (R,)), 'vf_loss': full(t['vf_loss'], (R,)),
                'clipped': full((t['s2'] < t['s1']).to(dt), (R,)), 'vf_clipped': full((t['d2'] * t['d2'] > t['d1'] * t['d1']).to(dt), (R,))}
        if form == 'float64':
            total.backward()
        else:
            c_lp = torch.where(t['s1'] <= t['s2'], -t['s1'], torch.zeros_like(t['s1']))
            onehot = torch.zeros_like(t['p']).scatter_(-1, b['actions'].unsqueeze(-1), 1.0)
            d = c_lp[:, None, None] * (onehot - t['p']) + hy['kl_coeff'] * (t['p'] - t['po']) \
                + hy['entropy_coeff'] * (t['p'] * (t['lsm'] + t['ent_h'].unsqueeze(-1)))
            dl = torch.zeros((N, heads, A), dtype=dt)
            dl[:, :hc] = d
            dl = dl.reshape(N, N3)
            l1, l2 = t['d1'] * t['d1'], t['d2'] * t['d2']
            inside = ((v - b['old_vf']).abs() < hy['vf_clip_param']).to(dt)
            dv = hy['vf_loss_coeff'] * torch.where(l1 >= l2, 2 * t['d1'], 2 * t['d2'] * inside)
    rows['vf'] = torch.zeros(R, dtype=dt).index_copy_(0, idx, v.detach())

    if form == 'float64':
        grads = {n: (leaf[n].grad if leaf[n].grad is not None else torch.zeros_like(leaf[n])).numpy() for n in ARRAYS}
        return stats, grads, rows

    def backward(a0, a1, a2, w2, w3, d3):
        """dW1, db1, dW2, db2, dW3, db3 of one trunk: a0 = x, a1 = h1, a2 = h2 (bf16 values), d3 = the f32 delta of the output."""
        d3 = _bf16(d3)
        dA2 = _bf16((d3 @ w3.t()) * _dact(activation, a2))
        dA1 = _bf16((dA2 @ w2.t()) * _dact(activation, a1))
        s = np.float32(scale)
        return [(g * s).numpy() for g in (a0.t() @ dA1, dA1.sum(0), a1.t() @ dA2, dA2.sum(0), a2.t() @ d3, d3.sum(0))]
    with torch.no_grad():
        gp = backward(x, h1, h2, leaf['w2'], leaf['w3'], dl)
        gv = backward(x, g1, g2, leaf['vw2'], leaf['wv'].reshape(H, 1), dv.reshape(N, 1))
    grads = dict(zip(_POLICY, gp))
    grads.update(dict(zip(_VALUE, gv)))
    grads['wv'] = grads['wv'].reshape(-1)
    return stats, grads, rows


def adam_constants(t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """The f32 scalars of step t (1, 2, ...): the bias corrections 1 - beta^t are computed in double from the f32 betas."""
    f = np.float32
    b1, b2 = float(f(beta1)), float(f(beta2))
    return {'beta1': f(beta1), 'omb1': f(1.0 - b1), 'beta2': f(beta2), 'omb2': f(1.0 - b2),
            'step_size': f(float(f(lr)) / (1.0 - b1 ** int(t))), 'bc2_sqrt': f(math.sqrt(1.0 - b2 ** int(t))), 'eps': f(eps)}


def adam_reference(w, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam's update (no weight decay, no amsgrad) as numpy float32 operations, each rounded on its own, in this
    order -- what the kernel computes bit for bit.  t: the step being taken (1 for the first).  Returns (w, m, v)."""
    c = adam_constants(t, lr, beta1, beta2, eps)
    w, g, m, v = (np.asarray(a, dtype=np.float32) for a in (w, g, m, v))
    m = m * c['beta1'] + g * c['omb1']
    v = v * c['beta2'] + (g * g) * c['omb2']
    denom = np.sqrt(v) / c['bc2_sqrt'] + c['eps']
    w = w - c['step_size'] * (m / denom)
    return w, m, v


def clip_reference(g_flat, grad_clip):
    """torch.nn.utils.clip_grad_norm_ on the flat float32 gradient, as finish() computes it: the global L2 norm in float64, the
    coefficient min(1, grad_clip / (norm + 1e-6)) rounded to float32, one float32 product per entry.  grad_clip None or 0: the
    gradient as it is.  Returns (clipped gradient float32, norm as float32)."""
    g = np.asarray(g_flat, dtype=np.float32).reshape(-1)
    norm = math.sqrt(float((g.astype(np.float64) ** 2).sum()))
    if not grad_clip:
        return g.copy(), np.float32(norm)
    coef = np.float32(min(1.0, float(grad_clip) / (norm + 1e-6)))
    return g * coef, np.float32(norm)


class _FcnetDesc(ctypes.Structure):
    """The head of dcomp_fcnet_desc (csrc/dcomp_fcnet_plan.h): the constants; the plans behind them are not read here."""
    _fields_ = [(n, ctypes.c_int32) for n in ('struct_size', 'TILE', 'WAVES', 'BLOCK', 'KC', 'LT', 'CHUNK_UNIT', 'MAX_CHUNKS', 'max_blocks', 'grid_tiles')] + \
        [('actor', ctypes.c_int32 * 14), ('learner', ctypes.c_int32 * 88), ('split', ctypes.c_int64 * 5)]


class _FcnetShape(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('struct_size', 'obs_kind', 'num_ue', 'num_bs', 'hidden')] + [('rows', ctypes.c_int64), ('compute_units', ctypes.c_int32)]


def chunk_unit():
    """Rows of a weight-gradient chunk (CHUNK_UNIT), from the library: what a micro-batch must be a multiple of."""
    L = _lib.load()
    s = _FcnetShape(ctypes.sizeof(_FcnetShape), _lib.MULTI, 1, 1, 32, 0, 0)
    d = _FcnetDesc(ctypes.sizeof(_FcnetDesc))
    L.dcomp_fcnet_describe.argtypes = [ctypes.POINTER(_FcnetShape), ctypes.POINTER(_FcnetDesc)]
    _lib.check(L.dcomp_fcnet_describe(ctypes.byref(s), ctypes.byref(d)))
    return int(d.CHUNK_UNIT)


def check_micro_rows(micro_rows, max_rows):
    """update(micro_rows=...): a multiple of the chunk unit (every micro-batch but the last then ends on a chunk boundary, and the
    accumulated sum has the whole minibatch's order) and at most the handle's max_rows."""
    unit = chunk_unit()
    if isinstance(micro_rows, bool) or int(micro_rows) != micro_rows or int(micro_rows) < unit or int(micro_rows) % unit:
        raise ValueError(f"micro_rows {micro_rows!r} must be a positive multiple of {unit} rows (a weight-gradient chunk)")
    if int(micro_rows) > max_rows:
        raise ValueError(f"micro_rows {int(micro_rows)} > max_rows {max_rows} of the learner")
    return int(micro_rows)


def adapt_kl_coeff(kl_coeff, kl, kl_target):
    """RLlib's update_kl: x 1.5 above twice the target, x 0.5 below half of it."""
    if kl > 2.0 * kl_target:
        return kl_coeff * 1.5
    if kl < 0.5 * kl_target:
        return kl_coeff * 0.5
    return kl_coeff


def to_rllib_weights(arrays, prefix='default_policy/'):
    """The twelve arrays under RLlib's fcnet names (kernels [in][out], value_out's kernel [hidden][1]): the inverse of
    FcnetActor.map_rllib_weights / map_rllib_value_weights."""
    names = {'w1': 'fc_1/kernel', 'b1': 'fc_1/bias', 'w2': 'fc_2/kernel', 'b2': 'fc_2/bias', 'w3': 'fc_out/kernel', 'b3': 'fc_out/bias',
             'vw1': 'fc_value_1/kernel', 'vb1': 'fc_value_1/bias', 'vw2': 'fc_value_2/kernel', 'vb2': 'fc_value_2/bias',
             'wv': 'value_out/kernel', 'bv': 'value_out/bias'}
    out = {prefix + names[n]: np.array(arrays[n], dtype=np.float32) for n in ARRAYS}
    out[prefix + 'value_out/kernel'] = out[prefix + 'value_out/kernel'].reshape(-1, 1)
    return out


def _arrays_struct(arrays):
    """A dcomp_learner_arrays over the numpy arrays of a dict (which must stay alive while the struct is in use)."""
    fp = ctypes.POINTER(ctypes.c_float)
    return _lib.DcompLearnerArrays(ctypes.sizeof(_lib.DcompLearnerArrays), 0, *[arrays[n].ctypes.data_as(fp) for n in ARRAYS])


# ---------------------------------------------------------------------------------------------- the SGD phase, stated once
# PPOLearner.update, DataParallelLearner.update_phases and PerUELearner's grouped update are loops over these pieces; the entry
# methods (grads ... evaluate_indexed) and the three batch structs take their checks and pointers from FIELDS.
INPUT, UPSTREAM, OUTPUT = 'input', 'upstream', 'output'
SUM = 'sum'                                                    # the reduction a data-parallel learner applies where accumulated_step yields
_f32, _heads, _logits, _one = torch.float32, 'heads', 'num_logits', 1
# per-row field of a batch struct -> (dtype, elements per row: a number or the actor's attribute that holds it, role)
FIELDS = {'actions': (torch.uint8, _heads, INPUT), 'old_logp': (_f32, _heads, INPUT), 'old_logits': (_f32, _logits, INPUT),
          'advantages': (_f32, _one, INPUT), 'value_targets': (_f32, _one, INPUT), 'old_vf': (_f32, _one, INPUT),
          'dlogits': (_f32, _logits, UPSTREAM), 'dvalue': (_f32, _one, UPSTREAM),
          'logp': (_f32, _heads, OUTPUT), 'entropy': (_f32, _one, OUTPUT), 'kl': (_f32, _one, OUTPUT), 'vf': (_f32, _one, OUTPUT),
          'ratio': (_f32, _one, OUTPUT)}
INPUTS = tuple(n for n, f in FIELDS.items() if f[2] == INPUT)
# ... and the name a collect() batch has the input under
BATCH_KEYS = dict(zip(INPUTS, ('actions', 'action_logp', 'action_dist_inputs', 'advantages', 'value_targets', 'vf_preds')))


def per_row(actor, name):
    """Elements per row of a field for this actor."""
    n = FIELDS[name][1]
    return getattr(actor, n) if isinstance(n, str) else n


def fill(struct, **members):
    """A batch struct filled by member name, struct_size included.  (ctypes would take a misspelt member as a new attribute.)"""
    unknown = set(members) - {n for n, _ in struct._fields_}
    if unknown:
        raise TypeError(f"{struct.__name__} has no member {sorted(unknown)}")
    return struct(struct_size=ctypes.sizeof(struct), **members)


def field_pointers(actor, given, rows_of):
    """name -> device pointer of the per-row tensors given (None entries are left out), each checked against FIELDS; rows_of: the
    rows a tensor of each role must hold.  The result fills a batch struct by keyword: the member order is the struct's own."""
    ptr = {}
    for name, t in given.items():
        if t is not None:
            dtype, _, role = FIELDS[name]
            actor._check(t, dtype, rows_of[role] * per_row(actor, name), name)
            ptr[name] = t.data_ptr()
    return ptr


def flatten_batch(actor, batch):
    """(src, N, compact) of a collect(..., dist_inputs=True) batch: the per-row tensors flattened to N source rows, under the names
    grads_indexed takes, with 'obs' (rows) or 'obs_compact' (the compact record)."""
    a = actor
    if 'action_dist_inputs' not in batch:
        raise ValueError("the batch has no action_dist_inputs: collect(..., dist_inputs=True)")
    compact = 'obs' not in batch
    if compact and a.kind != _lib.MULTI:
        raise NotImplementedError("compact observation records exist for multi-agent observations only")
    src = {}
    for name, key in BATCH_KEYS.items():                       # [N, heads] / [N, logits] for the fields an actor sizes, [N] for the others
        src[name] = batch[key].reshape(-1, per_row(a, name)) if isinstance(FIELDS[name][1], str) else batch[key].reshape(-1)
    if not compact:
        src['obs'] = batch['obs'].reshape(-1, a.num_in)
    N = src['actions'].shape[0]
    if any(t.shape[0] != N for t in src.values()):
        raise ValueError("the batch's tensors disagree about the number of rows")
    if compact:
        src['obs_compact'] = batch['obs_compact'].reshape(-1, batch['obs_compact'].shape[-1])      # [T, E, words], contiguous: env t E + e
        if src['obs_compact'].shape[0] * a.U != N:
            raise ValueError("the batch's tensors disagree about the number of rows")
    return src, N, compact


def standardize(adv):
    """RLlib's standardisation of one learner's advantages: (a - mean) / max(1e-4, std), in the tensor's own precision."""
    return (adv - adv.mean()) / adv.std(unbiased=False).clamp_min(1e-4)


def select_rows(actor, src, N, compact, rows=None, num_active=None, check_rows=True):
    """The single-learner rule for which rows of a flattened batch a learner trains on, with their advantages standardised over the
    selected rows alone.  rows: distinct source rows (update()'s rows=); num_active: listed UEs (multi: the rows of the other slots
    are dropped; central: the kernel leaves the other heads out).  Returns (src, N, keep, kernel_active).  A rows batch is gathered
    at the selected rows (keep None).  The compact record is trained where it lies: src keeps every source row, keep holds the
    selected ones (None: all) and the standardised advantages stand in source order, where the index finds them."""
    a = actor
    kernel_active, keep = None, None
    if rows is not None:
        if num_active is not None:
            raise ValueError("rows and num_active exclude each other: leave the rows of unlisted slots out of rows")
        if not isinstance(rows, torch.Tensor) or rows.dim() != 1 or rows.numel() == 0 or rows.device != a.device or \
                rows.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"rows must be a non-empty 1-d int32 / int64 tensor on {a.device}")
        keep = rows.to(torch.int64)
        if check_rows:
            srt = keep.sort().values
            lo, hi, dup = torch.stack((srt[0], srt[-1], (srt[1:] == srt[:-1]).any().to(torch.int64))).tolist()      # one synchronisation
            if lo < 0 or hi >= N:
                raise ValueError(f"rows has entries outside the batch's {N} source rows")
            if dup:
                raise ValueError("rows has repeated entries: they must be distinct source rows")
    elif num_active is not None and int(num_active) < a.U:
        if a.kind == _lib.MULTI:
            keep = torch.nonzero(torch.arange(N, device=a.device) % a.U < int(num_active)).reshape(-1)
        else:
            kernel_active = int(num_active)
    if keep is not None:
        N = int(keep.numel())
        if not compact:
            src, keep = {k: t.index_select(0, keep) for k, t in src.items()}, None
    scattered = keep is not None
    adv = src['advantages'].index_select(0, keep) if scattered else src['advantages']
    adv = standardize(adv)
    if scattered:
        adv = torch.zeros_like(src['advantages']).index_copy_(0, keep, adv)
    return dict(src, advantages=adv), N, keep, kernel_active


def minibatch_plan(N, minibatch_rows, max_rows, micro_rows=None, grad_clip=None, noun="minibatches of {} rows", hint=""):
    """(mb, micro, accumulated): the rows of a minibatch (minibatch_rows, at most N; None: N), of a micro-batch -- the gather
    buffers' size -- and whether the minibatches go through the accumulators (micro_rows or grad_clip given)."""
    mb = N if minibatch_rows is None else min(int(minibatch_rows), N)
    if micro_rows is not None:
        micro = check_micro_rows(micro_rows, max_rows)
    elif mb > max_rows:
        raise ValueError(f"{noun.format(mb)} > max_rows {max_rows} of the learner{hint}")
    else:
        micro = mb
    if grad_clip is not None and not float(grad_clip) >= 0.0:
        raise ValueError(f"grad_clip {grad_clip!r} must be >= 0")
    return mb, min(micro, mb), micro_rows is not None or grad_clip is not None


def sgd_epochs(N, num_sgd_iter, seed, device):
    """Per SGD iteration one device permutation of N rows, from a generator seeded once."""
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    for _ in range(int(num_sgd_iter)):
        yield torch.randperm(N, generator=gen, device=device)


def minibatch_stats(N, mb, device):
    """(starts, stats): where the minibatches of an iteration begin, and their zeroed [minibatches, 5] statistics."""
    starts = list(range(0, N, mb))
    return starts, torch.zeros((len(starts), _lib.PPO_NUM_STATS), dtype=torch.float32, device=device)


def close_out(learners, means):
    """The end of an update: means is a float32 [len(learners), 5] device tensor, per learner the mean statistics of its last
    iteration's minibatches.  One transfer to the host (the update's one synchronisation); every learner's kl_coeff is adapted by
    RLlib's rule.  Returns one dict per learner: the statistics and the new kl_coeff."""
    outs = []
    for ln, mean in zip(learners, means.cpu().numpy()):
        out = {n: float(mean[i]) for i, n in enumerate(STATS)}
        ln.hyper['kl_coeff'] = adapt_kl_coeff(ln.hyper['kl_coeff'], out['kl'], ln.kl_target)
        out['kl_coeff'] = ln.hyper['kl_coeff']
        outs.append(out)
    return outs


class PPOLearner:
    """PPO on the device for the policy an FcnetActor runs; every update lands in the actor's own handle."""

    def __init__(self, actor, lr=5e-5, clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2, kl_target=0.01,
                 max_rows=65536, betas=(0.9, 0.999), eps=1e-8):
        self._h = None
        if not isinstance(actor, FcnetActor):
            raise ValueError("actor must be an FcnetActor")
        if actor.value_weights is None:
            raise ValueError("the actor has no value function (set_value): PPO needs one")
        if actor.value_shared:
            raise NotImplementedError("the shared value function (vf_share_layers=True) is not supported: the learner needs a value trunk of its own")
        self.actor, self.device, self._L = actor, actor.device, actor._L
        self.lr, self.kl_target = float(lr), float(kl_target)
        self.hyper = {'clip_param': float(clip_param), 'vf_clip_param': float(vf_clip_param), 'vf_loss_coeff': float(vf_loss_coeff),
                      'entropy_coeff': float(entropy_coeff), 'kl_coeff': float(kl_coeff)}
        self.max_rows = int(max_rows)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.shapes = {n: a.shape for n, a in join_weights(actor.weights, actor.value_weights).items()}
        host = {n: np.ascontiguousarray(a) for n, a in join_weights(actor.weights, actor.value_weights).items()}
        arr = _arrays_struct(host)
        cfg = _lib.DcompLearnerCfg(ctypes.sizeof(_lib.DcompLearnerCfg), 0, self.max_rows, self.betas[0], self.betas[1], self.eps, 0, ctypes.pointer(arr))
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._L.dcomp_learner_create(actor._h, ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self._mb = {}
        self._flat = None
        self.step = 0

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self._L.dcomp_learner_destroy(h)
            self._h = None

    # ------------------------------------------------------------------ the kernels
    def _fits(self, rows):
        if rows > self.max_rows:
            raise ValueError(f"{rows} rows > max_rows {self.max_rows} of the learner")
        return rows

    def _source_obs(self, source):
        """(obs tensor, obs_format, source rows) of a dict that holds 'obs' or 'obs_compact', after their checks."""
        a = self.actor
        if not isinstance(source, dict) or ('obs' in source) == ('obs_compact' in source):
            raise ValueError("source must be a dict that holds either 'obs' or 'obs_compact'")
        if 'obs' in source:
            obs, fmt = source['obs'], _lib.ACTOR_ROWS
            if not isinstance(obs, torch.Tensor) or obs.numel() == 0 or obs.numel() % a.num_in:
                raise ValueError(f"obs must hold a whole number of rows of {a.num_in} elements")
            n_src = obs.numel() // a.num_in
            a._check(obs, torch.float32, n_src * a.num_in, 'obs')
        else:
            obs, fmt = source['obs_compact'], _lib.ACTOR_COMPACT
            n_src = a._batch(obs, True)[1]                                     # (central: NotImplementedError)
        if n_src > 2 ** 31 - 1:
            raise ValueError(f"{n_src} source rows > 2^31 - 1")
        return obs, fmt, n_src

    def _hyper_struct(self):
        return _lib.DcompPpoHyper(ctypes.sizeof(_lib.DcompPpoHyper), *[self.hyper[n] for n in ('clip_param', 'vf_clip_param', 'vf_loss_coeff', 'entropy_coeff', 'kl_coeff')])

    def _rows(self, obs):
        return self._fits(self._source_obs({'obs': obs})[2])

    def _batch(self, obs, rows, num_active, fields):
        """dcomp_ppo_batch over checked tensors: a contiguous minibatch of `rows` rows, fields maps a per-row field to its tensor or None."""
        a = self.actor
        return fill(_lib.DcompPpoBatch, obs_format=_lib.ACTOR_ROWS, rows=rows, obs=obs.data_ptr(), num_active=a.U if num_active is None else int(num_active),
                    **field_pointers(a, fields, dict.fromkeys((INPUT, UPSTREAM, OUTPUT), rows)))

    def _sgd_source(self, source, index):
        """(obs tensor, obs_format, source rows, minibatch rows) of a flattened sample batch and an index, after their checks."""
        obs, fmt, n_src = self._source_obs(source)
        rows = n_src
        if index is not None:
            if not isinstance(index, torch.Tensor) or index.numel() == 0:
                raise ValueError("index must be a non-empty contiguous int32 device tensor")
            rows = index.numel()
            self.actor._check(index, torch.int32, rows, 'index')
        return obs, fmt, n_src, self._fits(rows)

    def _sgd_batch(self, where, source, index, num_active, wanted, outputs):
        """dcomp_sgd_batch over checked tensors: where = _sgd_source(); wanted names the per-row inputs taken from source (source_rows
        rows each), outputs maps a per-row output to its tensor or None (one row per minibatch position; the helper's earlier form, a
        (tensor, elements per row) pair, is still taken: the count is the field table's)."""
        a = self.actor
        obs, fmt, n_src, rows = where
        outputs = {n: t[0] if isinstance(t, tuple) else t for n, t in outputs.items()}
        ptr = field_pointers(a, {**{n: source.get(n) for n in wanted}, **outputs}, {INPUT: n_src, UPSTREAM: n_src, OUTPUT: rows})
        return fill(_lib.DcompSgdBatch, obs_format=fmt, rows=rows, source_rows=n_src, obs=obs.data_ptr(), index=index.data_ptr() if index is not None else None,
                    num_active=a.U if num_active is None else int(num_active), **ptr)

    def _stats(self, stats):
        if stats is None:
            stats = torch.zeros(_lib.PPO_NUM_STATS, dtype=torch.float32, device=self.device)
        self.actor._check(stats, torch.float32, _lib.PPO_NUM_STATS, 'stats')
        return stats

    def _submit(self, b, stats=None, into=None):
        """A checked batch struct, contiguous or indexed, to grads (into None: the statistics into `stats`, which is returned) or to
        accumulate (into = (acc, sums))."""
        entry = ('dcomp_sgd_' if isinstance(b, _lib.DcompSgdBatch) else 'dcomp_learner_') + ('grads' if into is None else 'accumulate')
        if into is None:
            stats = self._stats(stats)
            args = (ctypes.c_void_p(stats.data_ptr()),)
        else:
            args = self._accumulators(*into)
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._L, entry)(self._h, ctypes.byref(b), ctypes.byref(self._hyper_struct()), *args, self.actor._stream()))
        return stats

    def _evaluate(self, rows, batch_with):
        """evaluate / evaluate_indexed: the outputs allocated, the struct batch_with(outputs) builds over them, the launch."""
        a = self.actor
        out = {'logp': torch.empty((rows, a.heads), dtype=torch.float32, device=self.device),
               'entropy': torch.empty(rows, dtype=torch.float32, device=self.device), 'vf': torch.empty(rows, dtype=torch.float32, device=self.device)}
        b = batch_with(out)
        entry = 'dcomp_sgd_evaluate' if isinstance(b, _lib.DcompSgdBatch) else 'dcomp_learner_evaluate'
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._L, entry)(self._h, ctypes.byref(b), a._stream()))
        return out['logp'], out['entropy'], out['vf']

    def grads(self, obs, actions=None, old_logp=None, old_logits=None, advantages=None, value_targets=None, old_vf=None, *, num_active=None,
              logp=None, entropy=None, kl=None, vf=None, ratio=None, dlogits=None, dvalue=None, stats=None):
        """The loss statistics (a float32 [5] device tensor: total_loss, policy_loss, vf_loss, kl, entropy) and the gradients of all
        twelve arrays into the handle, from one (mini)batch of device tensors: obs float32 [rows, inputs], actions uint8 [rows,
        heads], old_logp [rows, heads], old_logits [rows, logits], advantages / value_targets / old_vf [rows].  logp ... ratio:
        optional per-row outputs.  dlogits [rows, logits] with dvalue [rows]: upstream gradients used instead of the loss's (the
        gradients are then plain sums over the rows, the statistics zero).  Nothing synchronises."""
        return self._submit(self._batch(obs, self._rows(obs), num_active, dict(
            actions=actions, old_logp=old_logp, old_logits=old_logits, advantages=advantages, value_targets=value_targets, old_vf=old_vf,
            logp=logp, entropy=entropy, kl=kl, vf=vf, ratio=ratio, dlogits=dlogits, dvalue=dvalue)), stats)

    def evaluate(self, obs, actions, *, num_active=None):
        """logp [rows, heads] of the GIVEN actions, the entropy [rows] and the value predictions [rows] under the current weights."""
        rows = self._rows(obs)
        return self._evaluate(rows, lambda out: self._batch(obs, rows, num_active, dict(out, actions=actions)))

    # ------------------------------------------------------------------ minibatches through a row index (include/dcomp_learner_indexed.h)
    def grads_indexed(self, source, index=None, *, num_active=None, logp=None, entropy=None, kl=None, vf=None, ratio=None, stats=None):
        """grads() on the rows `index` picks out of a whole sample batch, without gathering them: source is a dict of the flattened
        sample-batch tensors -- 'obs' float32 [source_rows, inputs] or 'obs_compact' int32 [envs, words] (multi: the record
        collect(compact=True) returns; source row s is slot s % U of env s // U), and actions, old_logp, old_logits, advantages,
        value_targets, old_vf (or dlogits with dvalue) with source_rows rows each.  index: a contiguous int32 device tensor of
        minibatch positions -> source rows (None: every source row in order).  logp ... ratio: optional per-row outputs, one per
        index entry.  The results are those of grads() on the gathered rows, bit for bit.  An index entry outside the sample batch is
        not read: its position contributes zeros and still counts in the mean.  multi: num_active must stay the env's slots -- leave
        the rows of unlisted slots out of the index.  Nothing synchronises."""
        return self._submit(self._sgd_batch(self._sgd_source(source, index), source, index, num_active, INPUTS + ('dlogits', 'dvalue'),
                                            dict(logp=logp, entropy=entropy, kl=kl, vf=vf, ratio=ratio)), stats)

    def evaluate_indexed(self, source, index=None, *, num_active=None):
        """evaluate() on the rows `index` picks out of source ('obs' or 'obs_compact', and 'actions'): logp [rows, heads], the entropy
        [rows] and the value predictions [rows], one row per index entry."""
        where = self._sgd_source(source, index)
        return self._evaluate(where[3], lambda out: self._sgd_batch(where, source, index, num_active, ('actions',), out))

    # ------------------------------------------------------------------ accumulated gradients (include/dcomp_learner_accum.h)
    @property
    def flat_size(self):
        """Elements of the flat gradient array: the twelve arrays one behind the other, in ARRAYS' order."""
        if self._flat is None:
            n = ctypes.c_int64()
            _lib.check(self._L.dcomp_learner_flat_size(self._h, ctypes.byref(n)))
            self._flat = int(n.value)
        return self._flat

    def new_accumulators(self):
        """(acc float32 [flat_size], sums float64 [8]) on the learner's device, zeroed: the running sums of one minibatch.  sums: the
        sums of the surrogate, kl, entropy and value loss over the counted rows, the counted rows, three reserved."""
        return (torch.zeros(self.flat_size, dtype=torch.float32, device=self.device),
                torch.zeros(_lib.ACCUM_SUMS, dtype=torch.float64, device=self.device))

    def _accumulators(self, acc, sums):
        self.actor._check(acc, torch.float32, self.flat_size, 'acc')
        self.actor._check(sums, torch.float64, _lib.ACCUM_SUMS, 'sums')
        return ctypes.c_void_p(acc.data_ptr()), ctypes.c_void_p(sums.data_ptr())

    def accumulate(self, obs, actions, old_logp, old_logits, advantages, value_targets, old_vf, acc, sums, *, num_active=None,
                   logp=None, entropy=None, kl=None, vf=None, ratio=None):
        """grads() up to the sums over the rows, which are ADDED to acc / sums (new_accumulators(); the caller zeroes them before a
        minibatch's first call) instead of being scaled into the handle: acc += the unnormalised gradient of these rows, sums += their
        loss sums and their count.  The handle's gradients are not written.  finish() turns the accumulated sums into the gradients
        apply() consumes.  While every call but the last has a multiple of the chunk unit (chunk_unit(): 2 048 rows) and the calls
        together have at most 262 144 rows, finish() gives the gradients of grads() on all rows at once, bit for bit.  Upstream
        gradients are not taken here: they are plain sums already."""
        self._submit(self._batch(obs, self._rows(obs), num_active, dict(
            actions=actions, old_logp=old_logp, old_logits=old_logits, advantages=advantages, value_targets=value_targets, old_vf=old_vf,
            logp=logp, entropy=entropy, kl=kl, vf=vf, ratio=ratio)), into=(acc, sums))

    def accumulate_indexed(self, source, index, acc, sums, *, num_active=None, logp=None, entropy=None, kl=None, vf=None, ratio=None):
        """accumulate() on the rows `index` picks out of a whole sample batch (grads_indexed's source and index)."""
        self._submit(self._sgd_batch(self._sgd_source(source, index), source, index, num_active, INPUTS,
                                     dict(logp=logp, entropy=entropy, kl=kl, vf=vf, ratio=ratio)), into=(acc, sums))

    def finish(self, acc, sums, grad_clip=None, stats=None, grad_norm=None):
        """The handle's gradients from accumulated sums: g = acc * float32(1 / sums[4]); with grad_clip (> 0) g is scaled by
        min(1, grad_clip / (norm + 1e-6)), norm the global L2 norm over all twelve arrays (torch.nn.utils.clip_grad_norm_,
        clip_reference()).  grad_norm: a float32 [1] device tensor that receives the norm of the unclipped g (also without grad_clip).
        acc and sums are read only.  Returns the five statistics (a float32 [5] device tensor, `stats` if given) formed from sums as
        grads() forms them.  Nothing synchronises."""
        a = self.actor
        clip = 0.0 if grad_clip is None else float(grad_clip)
        if not clip >= 0.0:
            raise ValueError(f"grad_clip {grad_clip!r} must be >= 0 (None or 0: no clipping)")
        pa, ps = self._accumulators(acc, sums)
        stats = self._stats(stats)
        if grad_norm is not None:
            a._check(grad_norm, torch.float32, 1, 'grad_norm')
        with torch.cuda.device(self.device):
            _lib.check(self._L.dcomp_learner_accum_finish(self._h, pa, ps, ctypes.byref(self._hyper_struct()), clip, ctypes.c_void_p(stats.data_ptr()),
                                                          ctypes.c_void_p(grad_norm.data_ptr()) if grad_norm is not None else None, a._stream()))
        return stats

    clip_reference = staticmethod(clip_reference)

    def apply(self, lr=None):
        """One Adam step on the gradients of the last grads() or finish(); the actor's next launch runs the new weights."""
        with torch.cuda.device(self.device):
            _lib.check(self._L.dcomp_learner_apply(self._h, float(self.lr if lr is None else lr), self.actor._stream()))

    # ------------------------------------------------------------------ host copies
    def read(self, which='weights'):
        """The twelve arrays of the master weights ('weights'), the gradients ('grads') or Adam's moments ('m', 'v') as numpy."""
        code = {'weights': _lib.LEARNER_WEIGHTS, 'grads': _lib.LEARNER_GRADS, 'm': _lib.LEARNER_ADAM_M, 'v': _lib.LEARNER_ADAM_V}[which]
        out = {n: np.empty(self.shapes[n], dtype=np.float32) for n in ARRAYS}
        step = ctypes.c_int64()
        with torch.cuda.device(self.device):
            _lib.check(self._L.dcomp_learner_read(self._h, code, ctypes.byref(_arrays_struct(out)), ctypes.byref(step), self.actor._stream()))
        self.step = int(step.value)
        return out

    def get_weights(self):
        """(weights, value_weights) as FcnetActor takes them; also refreshes actor.weights / actor.value_weights, which the
        actor's reference_* methods read."""
        w, vw = split_weights(self.read('weights'))
        self.actor.weights, self.actor.value_weights = w, vw
        return w, vw

    def to_rllib_weights(self, prefix='default_policy/'):
        return to_rllib_weights(self.read('weights'), prefix)

    def state_dict(self):
        return {'weights': self.read('weights'), 'm': self.read('m'), 'v': self.read('v'), 'step': self.step, 'kl_coeff': self.hyper['kl_coeff'], 'lr': self.lr}

    def load_state_dict(self, state):
        host = {}
        for k in ('weights', 'm', 'v'):
            host[k] = {n: np.ascontiguousarray(np.asarray(state[k][n], dtype=np.float32)) for n in ARRAYS}
            for n in ARRAYS:
                if host[k][n].shape != self.shapes[n]:
                    raise ValueError(f"{k}[{n!r}] has shape {host[k][n].shape}, expected {self.shapes[n]}")
        with torch.cuda.device(self.device):
            _lib.check(self._L.dcomp_learner_load_state(self._h, ctypes.byref(_arrays_struct(host['weights'])), ctypes.byref(_arrays_struct(host['m'])),
                                                        ctypes.byref(_arrays_struct(host['v'])), int(state['step']), self.actor._stream()))
        self.hyper['kl_coeff'], self.lr = float(state['kl_coeff']), float(state['lr'])
        self.actor.weights, self.actor.value_weights = split_weights(host['weights'])

    # ------------------------------------------------------------------ the training step
    def _gather_buffers(self, src, size):
        """The gather buffers of a rows batch, allocated once per size: one row per position of a (micro-)batch."""
        if size not in self._mb:
            self._mb = {size: {k: torch.empty((size,) + tuple(t.shape[1:]), dtype=t.dtype, device=self.device) for k, t in src.items()}}
        return self._mb[size]

    def submit_picks(self, src, compact, picks, size, num_active=None, stats=None, into=None):
        """One (micro-)batch of a flattened sample batch (src as flatten_batch() leaves it) to grads (into None) or to accumulate (into
        = (acc, sums)): picks are its source rows in order.  The compact record is trained where it lies -- picks (int32) is the row
        index of the indexed call; a rows batch is gathered into the buffers of `size` positions and goes through the contiguous call."""
        if compact:
            b = self._sgd_batch(self._sgd_source(src, picks), src, picks, None, INPUTS, {})
        else:
            view = {k: t[:int(picks.numel())] for k, t in self._gather_buffers(src, size).items()}
            for k in src:
                torch.index_select(src[k], 0, picks, out=view[k])
            obs = view.pop('obs')
            b = self._batch(obs, self._rows(obs), num_active, view)
        return self._submit(b, stats, into)

    def accumulate_minibatch(self, src, compact, picks, micro, acc, sums, num_active=None):
        """One minibatch of a flattened sample batch into acc / sums, `micro` positions at a time (submit_picks)."""
        for s in range(0, int(picks.numel()), micro):
            self.submit_picks(src, compact, picks[s:s + micro], micro, num_active, into=(acc, sums))

    def accumulated_step(self, src, compact, picks, micro, acc, sums, grad_clip, stats, num_active=None, lap=lambda name: None):
        """One minibatch of the accumulated path as phases: zeroed accumulators, accumulate per micro-batch, then (acc, SUM) and (sums,
        SUM) are yielded -- where the ranks of a data-parallel learner add theirs together; one learner just goes on -- then finish
        (1 / N, grad_clip; the statistics into `stats`) and apply.  lap(name) is called at the end of each of the four phases."""
        acc.zero_()
        sums.zero_()
        self.accumulate_minibatch(src, compact, picks, micro, acc, sums, num_active)
        lap('accumulate')
        yield acc, SUM
        yield sums, SUM
        lap('reduce')
        self.finish(acc, sums, grad_clip, stats=stats)
        lap('finish')
        self.apply()
        lap('apply')

    def update(self, batch, num_sgd_iter=30, minibatch_rows=None, seed=0, num_active=None, rows=None, check_rows=True, micro_rows=None,
               grad_clip=None):
        """PPO's SGD phase on one collect(..., dist_inputs=True) batch, observation rows or the compact record (compact=True): the
        batch is flattened to source rows, the advantages are standardised over the batch (RLlib: (a - mean) / max(1e-4, std)), and
        per iteration a seeded device permutation splits the rows into minibatches of minibatch_rows (default: the whole batch);
        each gets grads + apply.  A compact batch is trained where it lies: a minibatch is its slice of the permutation, handed to
        grads_indexed as the row index -- no observation row is ever written.  A rows batch is gathered into buffers allocated once
        and goes through grads: measured, the gather and contiguous reads beat scattered reads of whole rows at large batches
        (profiles/r11_learner_indexed.txt); both ways give the same bits.  Afterwards the mean KL of the last iteration is read (the
        one synchronisation) and kl_coeff adapted by RLlib's rule.  num_active: listed UEs where fewer than the env's slots (multi:
        the other rows are dropped before the split).  rows: an integer device tensor of distinct source rows of the flattened batch
        -- the learner then trains on exactly those rows: the advantages are standardised over them alone, the permutation runs over
        them only, and the result is that of update() on the batch gathered at rows, bit for bit (deepcomp_amd.policy_set hands each
        per-UE policy the rows of its slots this way); not together with num_active.  A collect(..., by_ue=True) batch of an env with UE arrival / departure is trained this way:
        rows=sampler.live_rows(batch), the rows whose UE acted and was still listed after the step -- every other row holds advantages
        = value_targets = 0 and must stay out of the mean and the standardisation.  rows are checked to be inside the batch and
        distinct (one sort and one synchronisation; check_rows=False skips it for rows the caller built itself).  Returns the last iteration's mean statistics
        and the new kl_coeff.

        micro_rows / grad_clip (both None: the path above, unchanged): a minibatch is then trained as zeroed accumulators, one
        accumulate per micro-batch of micro_rows positions (default: the whole minibatch), finish (1 / N of the minibatch, and the
        global-norm clip of RLlib's grad_clip) and apply.  micro_rows is a multiple of the chunk unit (2 048 rows) and at most
        max_rows; the workspaces and gather buffers are then sized by the micro-batch, and a minibatch may be larger than max_rows.
        Up to 262 144 rows per minibatch the new weights are those of the whole-minibatch path, bit for bit (without grad_clip)."""
        src, N, compact = flatten_batch(self.actor, batch)
        src, N, keep, kernel_active = select_rows(self.actor, src, N, compact, rows, num_active, check_rows)
        mb, micro, accumulated = minibatch_plan(N, minibatch_rows, self.max_rows, micro_rows, grad_clip)
        if accumulated:
            acc, sums = self.new_accumulators()
        starts, stats = minibatch_stats(N, mb, self.device)
        for perm in sgd_epochs(N, num_sgd_iter, seed, self.device):
            picks = perm if not compact else (perm if keep is None else keep.index_select(0, perm)).to(torch.int32)
            for i, s in enumerate(starts):
                if accumulated:
                    for _ in self.accumulated_step(src, compact, picks[s:s + mb], micro, acc, sums, grad_clip, stats[i], kernel_active):
                        pass                                               # (one learner: nothing to add together)
                else:
                    self.submit_picks(src, compact, picks[s:s + mb], mb, kernel_active, stats=stats[i])
                    self.apply()
        return close_out([self], stats.mean(0)[None])[0]
