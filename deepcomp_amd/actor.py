"""A trained fcnet actor on the device (include/dcomp.h: dcomp_actor_create / dcomp_actor_actions / dcomp_actor_actions_v).

What the reference does with a trained policy -- ``trainer.compute_action(obs, policy_id=...)`` per env and step
(util/simulation.py:347,375,512-541) -- for the whole batch in one HIP launch: the observation tensor the env kernel wrote (rows,
or the compact record) goes through RLlib's default fcnet (two hidden layers of one width, tanh or relu) on the matrix cores with
the activations kept on chip, and out comes the uint8 action tensor ``env.step`` takes:

    actor = FcnetActor.from_rllib_weights('multi', U, B, policy.get_weights())
    act = actor.act(env)                               # uint8 [E, U], feed straight into env.step(act)

``multi``: one decision row per (env, UE slot), the weights shared across UEs (DD-CoMP), one categorical head of B + 1 actions.
``central``: one row per env, U heads (MultiDiscrete, central.py:28).  D3-CoMP's per-UE networks are a set over such actors, run in
one launch: deepcomp_amd.policy_set.PerUEActor (a policy per UE slot) and PerIdActor (a policy per UE id, for envs whose UE list
changes).  Training is deepcomp_amd.learner.PPOLearner, on this actor's handle.

The value function of a PPO policy rides in the same launch once attached (``value_weights=`` / ``set_value``): RLlib's fcnet has it
as a trunk of its own (``fc_value_1``, ``fc_value_2``, ``value_out``: PPO's default, vf_share_layers=False) or as ``value_out`` on
the actor's second hidden layer (shared).  ``actions(..., vf=buf)`` then also writes the value predictions, ``value(obs)`` is the
value-only call (the bootstrap of a sample batch); deepcomp_amd.sampler collects whole PPO sample batches with them.

The arithmetic is the specification, and ``reference_logits`` spells it out in torch on the CPU (as agents.py does for the
heuristics): x = bf16(obs row); h1 = bf16(act(x W1 + b1)); h2 = bf16(act(h1 W2 + b2)); logits = h2 W3 + b3 -- bf16 products, f32
accumulation, bias and activation in f32.  Sampling is Gumbel-max over counter-based draws keyed by (seed, step, global decision
row, head, action), see ``gumbel_noise``: a batch split over calls or GPUs draws what the whole batch would.
"""
import ctypes

import numpy as np
import torch

from . import _lib

_NAMES = ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')
_VALUE_TRUNK, _VALUE_OUT = ('w1', 'b1', 'w2', 'b2'), ('wv', 'bv')
DRAW_TAG = 0x00AC7012


def _bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float32)


def layer_shapes(kind, num_ue, num_bs, hidden):
    """(inputs, heads, logits) and the shapes of the six weight arrays."""
    multi = kind in ('multi', _lib.MULTI)
    nin = 4 * num_bs + 1 if multi else num_ue * (2 * num_bs + 1)
    heads = 1 if multi else num_ue
    nout = heads * (num_bs + 1)
    return nin, heads, nout, {'w1': (nin, hidden), 'b1': (hidden,), 'w2': (hidden, hidden), 'b2': (hidden,), 'w3': (hidden, nout), 'b3': (nout,)}


def gumbel_noise(philox, seed, step, rows, heads, num_actions):
    """The kernel's Gumbel draws recomputed on the host: float64 [len(rows), heads, num_actions].  philox(ctr, key) -> 4 words is a
    Philox4x32-10 (the test suite passes oracle.philox4x32_10); rows are GLOBAL decision-row indices (row_base + local row)."""
    key = [int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF]
    words = np.zeros((len(rows), heads, 4 * ((num_actions + 3) // 4)), dtype=np.uint32)
    for i, row in enumerate(rows):
        for hd in range(heads):
            for blk in range((num_actions + 3) // 4):
                words[i, hd, 4 * blk:4 * blk + 4] = philox([int(row) & 0xFFFFFFFF, (hd << 16) | blk, int(step) & 0xFFFFFFFF, DRAW_TAG], key)
    w = words[..., :num_actions]
    u = ((w >> 8).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)        # the kernel's f32 expression ...
    u = np.minimum(u, np.float32(1.0 - 2.0 ** -24))                                    # ... kept below 1.0, where the draw would be infinite
    return -np.log(-np.log(u.astype(np.float64)))


class _ActorLaunch:
    """The launch side of an actor handle: the pointer, dtype and size checks and the one launch.  FcnetActor has it, and so has the
    per-UE set of such actors (deepcomp_amd.policy_set.PerUEActor), whose entry points take the same arguments.  A subclass provides
    kind, U, B, heads, num_logits, num_in, device, value_weights, _L and _h."""
    _ACTIONS, _ACTIONS_V = 'dcomp_actor_actions', 'dcomp_actor_actions_v'

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, t, dtype, numel, what):
        """The kernel gets raw pointers: a wrong dtype / device / size would read or write out of bounds on the device."""
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.device or not t.is_contiguous() or t.numel() != numel:
            raise ValueError(f"{what} must be a contiguous {dtype} tensor with {numel} elements on {self.device}")

    def actions(self, obs, *, compact=False, sample=True, seed=0, step=0, row_base=0, num_active=None, out=None, logits=None, logp=None,
                vf=None):
        """Actions for a batch of observations.  obs: float32 [E, U, 4B+1] (multi) / [E, U(2B+1)] (central), or with compact=True
        the int32 record [E, U(B+2)+2B] of env.step_compact.  Returns uint8 [E, U].  logits [rows, heads*(B+1)] / logp [rows, heads]
        (float32, optional) receive what the action was chosen from / the log-probability of the chosen action; vf [rows] (float32,
        optional, needs a value function) the value predictions, from the same launch."""
        return self._launch(obs, compact, sample, seed, step, row_base, num_active, out, logits, logp, vf, True)

    def value(self, obs, *, compact=False, out=None):
        """The value predictions alone (float32 [rows]): the bootstrap value of a sample batch's last observation.  The policy's
        head and the draws are skipped."""
        E, rows = self._batch(obs, compact)
        if out is None:
            out = torch.empty(rows, dtype=torch.float32, device=self.device)
        self._launch(obs, compact, False, 0, 0, 0, None, None, None, None, out, False)
        return out

    def _batch(self, obs, compact):
        """(envs, decision rows) of an observation tensor, after its pointer, dtype and size checks."""
        if compact:
            if self.kind != _lib.MULTI:
                raise NotImplementedError("compact observation records exist for multi-agent observations only")
            from .fragment import fragment_words
            per_env, dtype = fragment_words(self.U, self.B), torch.int32
        else:
            per_env, dtype = (self.U * self.num_in if self.kind == _lib.MULTI else self.num_in), torch.float32
        if not isinstance(obs, torch.Tensor) or obs.numel() == 0 or obs.numel() % per_env:
            raise ValueError(f"obs must hold a whole number of envs of {per_env} elements")
        E = obs.numel() // per_env
        self._check(obs, dtype, E * per_env, 'obs')
        return E, (E * self.U if self.kind == _lib.MULTI else E)

    def _checked_run(self, obs, compact, sample, seed, step, row_base, num_active, out, logits, logp, vf, policy):
        """Every check of a launch's tensors, and its dcomp_actor_run: (envs, the action tensor, the run)."""
        E, rows = self._batch(obs, compact)
        if policy:
            if out is None:
                out = torch.empty((E, self.U), dtype=torch.uint8, device=self.device)
            self._check(out, torch.uint8, E * self.U, 'out')
        if vf is not None:
            if self.value_weights is None:
                raise ValueError("the actor has no value function (set_value)")
            self._check(vf, torch.float32, rows, 'vf')
        if logits is not None:
            self._check(logits, torch.float32, rows * self.num_logits, 'logits')
        if logp is not None:
            self._check(logp, torch.float32, rows * self.heads, 'logp')
        run = _lib.DcompActorRun(ctypes.sizeof(_lib.DcompActorRun), _lib.ACTOR_COMPACT if compact else _lib.ACTOR_ROWS, E,
                                 self.U if num_active is None else int(num_active), 1 if sample else 0, int(step) & 0xFFFFFFFF,
                                 int(seed) & 0xFFFFFFFFFFFFFFFF, int(row_base),
                                 logits.data_ptr() if logits is not None else None, logp.data_ptr() if logp is not None else None)
        return E, out, run

    def _launch(self, obs, compact, sample, seed, step, row_base, num_active, out, logits, logp, vf, policy):
        _, out, run = self._checked_run(obs, compact, sample, seed, step, row_base, num_active, out, logits, logp, vf, policy)
        with torch.cuda.device(self.device):
            if vf is None:
                _lib.check(getattr(self._L, self._ACTIONS)(self._h, ctypes.byref(run), ctypes.c_void_p(obs.data_ptr()),
                                                       ctypes.c_void_p(out.data_ptr()), self._stream()))
            else:
                _lib.check(getattr(self._L, self._ACTIONS_V)(self._h, ctypes.byref(run), ctypes.c_void_p(obs.data_ptr()),
                                                         ctypes.c_void_p(out.data_ptr()) if policy else None,
                                                         ctypes.c_void_p(vf.data_ptr()), self._stream()))
        return out

    def act(self, env, sample=True, obs=None, compact=False, out=None, logp=None, vf=None, logits=None):
        """The actor's actions on env.obs (or on `obs`, e.g. the record env.step_compact wrote: compact=True) as the tensor
        env.step takes.  Draws are keyed by the env's seed, step = env.time + episode * episode_length and the GLOBAL decision row
        (env_id_base * U on a sharded env): reproducible, and independent of how the env axis is split over GPUs."""
        if env.kind != self.kind or env.U != self.U or env.B != self.B:
            raise ValueError("the env's kind / UE slots / stations differ from the actor's")
        rows_per_env = self.U if self.kind == _lib.MULTI else 1
        return self.actions(env.obs if obs is None else obs, compact=compact, sample=sample, seed=env.seed_value,
                            step=env.time + max(env.episode, 0) * env.episode_length, row_base=env.env_id_base * rows_per_env,
                            num_active=env.num_ue, out=out, logp=logp, vf=vf, logits=logits)


class FcnetActor(_ActorLaunch):
    """RLlib's default fcnet actor (two hidden layers, categorical heads) running as one HIP kernel."""

    def __init__(self, kind, num_ue, num_bs, weights, activation='tanh', device='cuda', value_weights=None):
        self.kind = _lib.MULTI if kind in ('multi', _lib.MULTI) else _lib.CENTRAL
        self.U, self.B = int(num_ue), int(num_bs)
        self.activation = activation
        if activation not in _lib.ACTIVATION:
            raise ValueError(f"activation {activation!r} is not one of {sorted(_lib.ACTIVATION)}")
        missing = [n for n in _NAMES if n not in weights]
        if missing:
            raise ValueError(f"weights lack {missing}")
        w = {n: np.ascontiguousarray(np.asarray(weights[n], dtype=np.float32)) for n in _NAMES}
        if w['w1'].ndim != 2:
            raise ValueError("w1 must be [inputs][hidden]")
        self.hidden = int(w['w1'].shape[1])
        self.num_in, self.heads, self.num_logits, shapes = layer_shapes(self.kind, self.U, self.B, self.hidden)
        for n in _NAMES:
            if w[n].shape != shapes[n]:
                raise ValueError(f"{n} has shape {w[n].shape}, expected {shapes[n]} ([in][out], the layout of a TF / RLlib kernel)")
        self.weights = w
        self._h = None
        L = _lib.load()
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError("deepcomp_amd runs on an AMD GPU (torch device 'cuda'); there is no CPU path")
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self._L = L
        fp = ctypes.POINTER(ctypes.c_float)
        cfg = _lib.DcompActorCfg(ctypes.sizeof(_lib.DcompActorCfg), self.kind, self.U, self.B, self.hidden, _lib.ACTIVATION[activation],
                                 *[w[n].ctypes.data_as(fp) for n in _NAMES])
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(L.dcomp_actor_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self.value_weights, self.value_shared = None, None
        if value_weights is not None:
            self.set_value(value_weights, shared='w1' not in value_weights)

    def set_value(self, weights, shared=False):
        """Attach the value function, once per actor.  shared=False: a trunk of its own, weights 'w1' [in][hidden], 'b1', 'w2', 'b2'
        (fc_value_1 / fc_value_2) and 'wv' [hidden], 'bv' [1] (value_out); shared=True (vf_share_layers): 'wv' and 'bv' only, on
        the actor's own second hidden layer."""
        names = _VALUE_OUT if shared else _VALUE_TRUNK + _VALUE_OUT
        missing = [n for n in names if n not in weights]
        if missing:
            raise ValueError(f"value weights lack {missing}")
        if shared and any(n in weights for n in _VALUE_TRUNK):
            raise ValueError("shared=True takes 'wv' and 'bv' only")
        w = {n: np.ascontiguousarray(np.asarray(weights[n], dtype=np.float32)) for n in names}
        w['wv'], w['bv'] = np.ascontiguousarray(w['wv'].reshape(-1)), np.ascontiguousarray(w['bv'].reshape(-1))
        H = self.hidden
        shapes = {'w1': (self.num_in, H), 'b1': (H,), 'w2': (H, H), 'b2': (H,), 'wv': (H,), 'bv': (1,)}
        for n in names:
            if w[n].shape != shapes[n]:
                raise ValueError(f"value {n} has shape {w[n].shape}, expected {shapes[n]}")
        fp = ctypes.POINTER(ctypes.c_float)
        ptr = lambda n: w[n].ctypes.data_as(fp) if n in w else None      # noqa: E731
        cfg = _lib.DcompActorValueCfg(ctypes.sizeof(_lib.DcompActorValueCfg), 1 if shared else 0, *[ptr(n) for n in _VALUE_TRUNK + _VALUE_OUT])
        with torch.cuda.device(self.device):
            _lib.check(self._L.dcomp_actor_set_value(self._h, ctypes.byref(cfg)))
        self.value_weights, self.value_shared = w, bool(shared)

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self._L.dcomp_actor_destroy(h)
            self._h = None

    # ------------------------------------------------------------------ construction
    @staticmethod
    def random_weights(kind, num_ue, num_bs, hidden=256, seed=0, bias_std=0.0):
        """Random-init weights (N(0, 1 / fan_in) kernels, N(0, bias_std) biases) for tools and tests."""
        g = torch.Generator().manual_seed(int(seed))
        _, _, _, shapes = layer_shapes(kind, num_ue, num_bs, hidden)
        out = {}
        for n in _NAMES:
            std = bias_std if n[0] == 'b' else shapes[n][0] ** -0.5
            out[n] = (torch.randn(shapes[n], generator=g) * std).numpy()
        return out

    @staticmethod
    def random_value_weights(kind, num_ue, num_bs, hidden=256, seed=0, bias_std=0.0, shared=False):
        """Random-init value weights (as random_weights; value_out N(0, 1 / hidden)) for tools and tests."""
        g = torch.Generator().manual_seed(int(seed) + 0x5EED)
        nin = layer_shapes(kind, num_ue, num_bs, hidden)[0]
        shapes = {'w1': (nin, hidden), 'b1': (hidden,), 'w2': (hidden, hidden), 'b2': (hidden,), 'wv': (hidden,), 'bv': (1,)}
        out = {}
        for n in (_VALUE_OUT if shared else _VALUE_TRUNK + _VALUE_OUT):
            std = bias_std if n[0] == 'b' else (hidden if n == 'wv' else shapes[n][0]) ** -0.5
            out[n] = (torch.randn(shapes[n], generator=g) * std).numpy()
        return out

    @classmethod
    def random(cls, kind, num_ue, num_bs, hidden=256, activation='tanh', seed=0, bias_std=0.0, device='cuda'):
        return cls(kind, num_ue, num_bs, cls.random_weights(kind, num_ue, num_bs, hidden, seed, bias_std), activation, device)

    @staticmethod
    def map_rllib_weights(weights):
        """RLlib's fcnet weight dict (``policy.get_weights()``: '<scope>/fc_1/kernel', '.../fc_1/bias', 'fc_2', 'fc_out'; kernels
        [in][out]) -> the six arrays.  The value branch (fc_value_*, value_out) is ignored."""
        want = {'fc_1/kernel': 'w1', 'fc_1/bias': 'b1', 'fc_2/kernel': 'w2', 'fc_2/bias': 'b2', 'fc_out/kernel': 'w3', 'fc_out/bias': 'b3'}
        out = {}
        for key, val in weights.items():
            k = key[:-2] if key.endswith(':0') else key
            for suffix, name in want.items():
                if k == suffix or k.endswith('/' + suffix):
                    if name in out:
                        raise ValueError(f"two entries for {suffix}")
                    out[name] = np.asarray(val, dtype=np.float32)
        missing = [s for s, n in want.items() if n not in out]
        if missing:
            raise ValueError(f"no entry for {missing}: not the weights of a two-layer fcnet")
        if any(k.endswith('fc_3/kernel') or k.endswith('fc_3/kernel:0') for k in weights):
            raise ValueError("more than two hidden layers")
        return out

    @staticmethod
    def map_rllib_value_weights(weights):
        """The value branch of RLlib's fcnet weight dict -> the value arrays of set_value: 'fc_value_1', 'fc_value_2' -> w1, b1, w2,
        b2 and 'value_out' (kernel [hidden][1]) -> wv [hidden], bv [1].  With vf_share_layers the dict has value_out only, and so
        has the result (set_value(..., shared=True))."""
        want = {'fc_value_1/kernel': 'w1', 'fc_value_1/bias': 'b1', 'fc_value_2/kernel': 'w2', 'fc_value_2/bias': 'b2',
                'value_out/kernel': 'wv', 'value_out/bias': 'bv'}
        out = {}
        for key, val in weights.items():
            k = key[:-2] if key.endswith(':0') else key
            for suffix, name in want.items():
                if k == suffix or k.endswith('/' + suffix):
                    if name in out:
                        raise ValueError(f"two entries for {suffix}")
                    out[name] = np.asarray(val, dtype=np.float32)
        if 'wv' not in out or 'bv' not in out:
            raise ValueError("no entry for value_out: the weights have no value branch")
        trunk = [n for n in _VALUE_TRUNK if n in out]
        if trunk and len(trunk) != len(_VALUE_TRUNK):
            raise ValueError(f"the value trunk is incomplete: only {trunk} of fc_value_1 / fc_value_2")
        if any(k.endswith('fc_value_3/kernel') or k.endswith('fc_value_3/kernel:0') for k in weights):
            raise ValueError("more than two hidden layers")
        out['wv'], out['bv'] = out['wv'].reshape(-1), out['bv'].reshape(-1)
        return out

    @classmethod
    def from_rllib_weights(cls, kind, num_ue, num_bs, weights, activation='tanh', device='cuda', with_value=False):
        return cls(kind, num_ue, num_bs, cls.map_rllib_weights(weights), activation, device,
                   value_weights=cls.map_rllib_value_weights(weights) if with_value else None)

    # ------------------------------------------------------------------ the specification
    @staticmethod
    def reference_logits_of(weights, obs_rows, activation='tanh', form='bf16'):
        """The arithmetic of the kernel in torch on the CPU.  obs_rows: [rows, inputs].  form='bf16': the specified chain (bf16
        operands, f32 accumulation, activations rounded to bf16) -> float32; form='float64': the same bf16-rounded weights and
        inputs in float64 with no activation rounding -- what the chain's error is measured against."""
        act = torch.tanh if activation == 'tanh' else torch.relu
        x = _bf16(torch.as_tensor(np.asarray(obs_rows, dtype=np.float32)).reshape(-1, weights['w1'].shape[0]))
        w = {n: torch.as_tensor(np.asarray(weights[n], dtype=np.float32)) for n in _NAMES}
        if form == 'float64':
            d = torch.float64
            h = act(x.to(d) @ _bf16(w['w1']).to(d) + w['b1'].to(d))
            h = act(h @ _bf16(w['w2']).to(d) + w['b2'].to(d))
            return h @ _bf16(w['w3']).to(d) + w['b3'].to(d)
        if form != 'bf16':
            raise ValueError("form is 'bf16' or 'float64'")
        h = _bf16(act(x @ _bf16(w['w1']) + w['b1']))
        h = _bf16(act(h @ _bf16(w['w2']) + w['b2']))
        return h @ _bf16(w['w3']) + w['b3']

    @staticmethod
    def reference_value_of(weights, value_weights, obs_rows, activation='tanh', form='bf16'):
        """The value's arithmetic in torch on the CPU, the twin of reference_logits_of: [rows].  value_weights with 'w1' ... 'b2': a
        trunk of its own; without: value_out on the actor's second hidden layer (weights' w1 ... b2)."""
        act = torch.tanh if activation == 'tanh' else torch.relu
        trunk = value_weights if 'w1' in value_weights else weights
        w = {n: torch.as_tensor(np.asarray(trunk[n], dtype=np.float32)) for n in _VALUE_TRUNK}
        wv = torch.as_tensor(np.asarray(value_weights['wv'], dtype=np.float32)).reshape(-1)
        bv = torch.as_tensor(np.asarray(value_weights['bv'], dtype=np.float32)).reshape(-1)[0]
        x = _bf16(torch.as_tensor(np.asarray(obs_rows, dtype=np.float32)).reshape(-1, w['w1'].shape[0]))
        if form == 'float64':
            d = torch.float64
            h = act(x.to(d) @ _bf16(w['w1']).to(d) + w['b1'].to(d))
            h = act(h @ _bf16(w['w2']).to(d) + w['b2'].to(d))
            return h @ _bf16(wv).to(d) + bv.to(d)
        if form != 'bf16':
            raise ValueError("form is 'bf16' or 'float64'")
        h = _bf16(act(x @ _bf16(w['w1']) + w['b1']))
        h = _bf16(act(h @ _bf16(w['w2']) + w['b2']))
        return h @ _bf16(wv) + bv

    def reference_value(self, obs_rows, form='bf16'):
        if self.value_weights is None:
            raise ValueError("the actor has no value function (set_value)")
        if torch.is_tensor(obs_rows):
            obs_rows = obs_rows.detach().cpu().numpy()
        return self.reference_value_of(self.weights, self.value_weights, obs_rows, self.activation, form)

    def reference_logits(self, obs_rows, form='bf16'):
        if torch.is_tensor(obs_rows):
            obs_rows = obs_rows.detach().cpu().numpy()
        return self.reference_logits_of(self.weights, obs_rows, self.activation, form)
