"""ctypes binding of libdcomp_hip.so (include/dcomp.h).  Fails loudly when the HIP extension is missing:
there is no CPU fallback in the product path."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DCOMP_LIB') or os.path.join(_HERE, 'csrc', 'libdcomp_hip.so')   # DCOMP_LIB: another build, e.g. a tools/ab/ab_lib.py variant

OK, EINVAL, EHIP, EACTION, ETAPE, EPOS, EUNSUPPORTED, EABI = 0, -1, -2, -3, -4, -5, -6, -7
ABI_VERSION = 3                 # include/dcomp.h DCOMP_ABI_VERSION: what the struct declarations below describe
CENTRAL, MULTI = 0, 1
REWARD = {'avg': 0, 'sum': 1, 'min': 2}
SHARING = {'resource-fair': 0, 'rate-fair': 1, 'max-cap': 2, 'proportional-fair': 3}
UTILITY = {'log': 0, 'step': 1}
RNG_TAPE, RNG_PHILOX = 0, 1
MAX_BS, MAX_UE = 64, 1024
SPECIAL_MAX_UE = 256             # up to here the specialised kernels; 257 ... 1 024 UEs per env: the generic kernel (csrc/dcomp_big.h)
MASK32_MAX_BS = 32              # up to here: one 32-bit connection mask per UE and the specialised kernels; beyond: state.conn_hi + the generic kernel

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_fp = ctypes.POINTER(ctypes.c_float)


class DcompCfg(ctypes.Structure):
    _fields_ = [('num_envs', ctypes.c_int32), ('num_ue', ctypes.c_int32), ('num_bs', ctypes.c_int32),
                ('map_w', ctypes.c_int32), ('map_h', ctypes.c_int32), ('env_kind', ctypes.c_int32),
                ('reward_agg', ctypes.c_int32), ('rng_mode', ctypes.c_int32), ('tape_depth', ctypes.c_int32),
                ('device', ctypes.c_int32), ('max_ues', ctypes.c_int32), ('seed', ctypes.c_uint64),
                ('env_id_base', ctypes.c_int64), ('bs_x', _dp), ('bs_y', _dp), ('bs_sharing', _ip),
                ('ue_util', _ip), ('ue_dr_req', _fp), ('ue_vel_lo', _ip), ('ue_vel_hi', _ip),
                ('ue_init_x', _ip), ('ue_init_y', _ip), ('ue_pause_duration', _ip), ('ue_border_buffer', _ip),
                ('ue_velocity', _dp)]


class DcompState(ctypes.Structure):
    _fields_ = [('pos', ctypes.c_void_p), ('mv', ctypes.c_void_p), ('conn', ctypes.c_void_p),
                ('ewma', ctypes.c_void_p), ('flags', ctypes.c_void_p), ('conn_since', ctypes.c_void_p),
                ('uid', ctypes.c_void_p), ('orig_consumed', ctypes.c_void_p), ('conn_hi', ctypes.c_void_p)]


class DcompOut(ctypes.Structure):
    _fields_ = [('obs', ctypes.c_void_p), ('reward', ctypes.c_void_p), ('sum_utility', ctypes.c_void_p),
                ('ue_dr', ctypes.c_void_p), ('ue_utility', ctypes.c_void_p), ('reward_before', ctypes.c_void_p),
                ('obs_compact', ctypes.c_void_p)]


class DcompTape(ctypes.Structure):
    _fields_ = [('pos0', ctypes.c_void_p), ('triples', ctypes.c_void_p), ('num_ids', ctypes.c_int32)]


class DcompRolloutOpts(ctypes.Structure):
    _fields_ = [('every_step', ctypes.c_int32), ('horizon', ctypes.c_int32), ('new_episode_draws', ctypes.c_int32),
                ('policy_loop', ctypes.c_int32), ('ev_n_remove', ctypes.c_void_p), ('ev_n_add', ctypes.c_void_p),
                ('ev_remove_idx', ctypes.c_void_p), ('ev_add_xy', ctypes.c_void_p)]


class DcompEvents(ctypes.Structure):
    _fields_ = [('n_remove', ctypes.c_int32), ('n_add', ctypes.c_int32), ('remove_idx', ctypes.c_void_p),
                ('add_xy', ctypes.c_void_p)]


class DcompPolicy(ctypes.Structure):
    _fields_ = [('policy', ctypes.c_int32), ('obs_kind', ctypes.c_int32), ('num_envs', ctypes.c_int32),
                ('num_ue', ctypes.c_int32), ('num_bs', ctypes.c_int32), ('num_active', ctypes.c_int32),
                ('epsilon', ctypes.c_float), ('cluster_mask', ctypes.c_void_p)]


POLICY = {'3gpp': 0, 'fullcomp': 1, 'dynamic': 2, 'cluster': 3}

ACTIVATION = {'tanh': 0, 'relu': 1}
ACTOR_ROWS, ACTOR_COMPACT = 0, 1
ACTOR_MAX_HIDDEN, ACTOR_MAX_IN, ACTOR_MAX_LOGITS = 256, 1024, 512


class DcompActorCfg(ctypes.Structure):
    _fields_ = [('struct_size', ctypes.c_int32), ('obs_kind', ctypes.c_int32), ('num_ue', ctypes.c_int32), ('num_bs', ctypes.c_int32),
                ('hidden', ctypes.c_int32), ('activation', ctypes.c_int32), ('w1', _fp), ('b1', _fp), ('w2', _fp), ('b2', _fp),
                ('w3', _fp), ('b3', _fp)]


class DcompActorRun(ctypes.Structure):
    _fields_ = [('struct_size', ctypes.c_int32), ('obs_format', ctypes.c_int32), ('num_envs', ctypes.c_int32),
                ('num_active', ctypes.c_int32), ('sample', ctypes.c_int32), ('step', ctypes.c_uint32), ('seed', ctypes.c_uint64),
                ('row_base', ctypes.c_int64), ('logits', ctypes.c_void_p), ('logp', ctypes.c_void_p)]


class DcompActorValueCfg(ctypes.Structure):
    _fields_ = [('struct_size', ctypes.c_int32), ('shared', ctypes.c_int32), ('w1', _fp), ('b1', _fp), ('w2', _fp), ('b2', _fp),
                ('wv', _fp), ('bv', _fp)]


class DcompGaeArgs(ctypes.Structure):
    _fields_ = [('struct_size', ctypes.c_int32), ('num_steps', ctypes.c_int32), ('num_rows', ctypes.c_int64),
                ('gamma', ctypes.c_float), ('lambda', ctypes.c_float), ('reward', ctypes.c_void_p), ('vf', ctypes.c_void_p),
                ('last_vf', ctypes.c_void_p), ('end', ctypes.c_void_p), ('advantages', ctypes.c_void_p),
                ('value_targets', ctypes.c_void_p)]


EXPORTS = ['dcomp_abi_version', 'dcomp_create_v', 'dcomp_create', 'dcomp_destroy', 'dcomp_state_sizes', 'dcomp_obs_dim', 'dcomp_reset', 'dcomp_step',
           'dcomp_step_dyn', 'dcomp_num_ue',
           'dcomp_rollout', 'dcomp_rollout_ex', 'dcomp_rollout_is_fused', 'dcomp_rollout_fused_for', 'dcomp_lanes_per_env', 'dcomp_needs_conn_hi', 'dcomp_step_kernel_name', 'dcomp_check', 'dcomp_time', 'dcomp_episode', 'dcomp_set_episode', 'dcomp_set_seed', 'dcomp_set_tape', 'dcomp_get_counters', 'dcomp_set_counters', 'dcomp_mt_draw_tape',
           'dcomp_connect_threshold', 'dcomp_connect_boundary_sq', 'dcomp_last_error', 'dcomp_version', 'dcomp_selftest', 'dcomp_heuristic_actions', 'dcomp_set_policy',
           'dcomp_fragment_words', 'dcomp_pack_fragment', 'dcomp_unpack_fragment',
           'dcomp_actor_create', 'dcomp_actor_destroy', 'dcomp_actor_actions',
           'dcomp_actor_set_value', 'dcomp_actor_actions_v', 'dcomp_gae']

# include/dcomp_learner.h: the PPO learner.  A list of its own: EXPORTS is what include/dcomp.h declares.
LEARNER_EXPORTS = ['dcomp_learner_create', 'dcomp_learner_destroy', 'dcomp_learner_grads', 'dcomp_learner_evaluate', 'dcomp_learner_apply',
                   'dcomp_learner_read', 'dcomp_learner_load_state']
LEARNER_ARRAYS = ('w1', 'b1', 'w2', 'b2', 'w3', 'b3', 'vw1', 'vb1', 'vw2', 'vb2', 'wv', 'bv')
LEARNER_WEIGHTS, LEARNER_GRADS, LEARNER_ADAM_M, LEARNER_ADAM_V = 0, 1, 2, 3
PPO_NUM_STATS = 5
PPO_STATS = ('total_loss', 'policy_loss', 'vf_loss', 'kl', 'entropy')


class DcompLearnerArrays(ctypes.Structure):
    _fields_ = [('struct_size', ctypes.c_int32), ('reserved', ctypes.c_int32)] + [(n, _fp) for n in LEARNER_ARRAYS]


class DcompLearnerCfg(ctypes.Structure):
    _fields_ = [('struct_size', ctypes.c_int32), ('value_shared', ctypes.c_int32), ('max_rows', ctypes.c_int64),
                ('beta1', ctypes.c_float), ('beta2', ctypes.c_float), ('eps', ctypes.c_float), ('reserved', ctypes.c_int32),
                ('weights', ctypes.POINTER(DcompLearnerArrays))]


class DcompPpoBatch(ctypes.Structure):
    _fields_ = [('struct_size', ctypes.c_int32), ('obs_format', ctypes.c_int32), ('rows', ctypes.c_int64),
                ('num_active', ctypes.c_int32), ('reserved', ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ('obs', 'actions', 'old_logp', 'old_logits', 'advantages', 'value_targets', 'old_vf',
                                               'logp', 'entropy', 'kl', 'vf', 'ratio', 'dlogits', 'dvalue')]


# include/dcomp_learner_indexed.h: minibatches through a row index into the whole sample batch, rows or compact record
SGD_EXPORTS = ['dcomp_sgd_grads', 'dcomp_sgd_evaluate']


class DcompSgdBatch(ctypes.Structure):
    _fields_ = [('struct_size', ctypes.c_int32), ('obs_format', ctypes.c_int32), ('rows', ctypes.c_int64), ('source_rows', ctypes.c_int64),
                ('index', ctypes.c_void_p), ('num_active', ctypes.c_int32), ('reserved', ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ('obs', 'actions', 'old_logp', 'old_logits', 'advantages', 'value_targets', 'old_vf',
                                               'dlogits', 'dvalue', 'logp', 'entropy', 'kl', 'vf', 'ratio')]


# include/dcomp_policy_set.h: one policy per UE slot over existing actor handles (D3-CoMP), one actor launch
SET_EXPORTS = ['dcomp_policy_set_create', 'dcomp_policy_set_destroy', 'dcomp_policy_set_actions', 'dcomp_policy_set_actions_v']


class DcompPolicySetCfg(ctypes.Structure):
    _fields_ = [('struct_size', ctypes.c_int32), ('num_policies', ctypes.c_int32), ('members', ctypes.POINTER(ctypes.c_void_p)),
                ('slot_policy', _ip)]


# include/dcomp_learner_group.h: the learners of a policy set trained in one launch round per minibatch round
GROUP_EXPORTS = ['dcomp_learner_group_create', 'dcomp_learner_group_destroy', 'dcomp_learner_group_grads', 'dcomp_learner_group_apply']


class DcompLearnerGroupCfg(ctypes.Structure):
    _fields_ = [('struct_size', ctypes.c_int32), ('num_learners', ctypes.c_int32), ('learners', ctypes.POINTER(ctypes.c_void_p))]


class DcompGroupBatch(ctypes.Structure):
    _fields_ = [('struct_size', ctypes.c_int32), ('obs_format', ctypes.c_int32), ('source_rows', ctypes.c_int64)] + \
               [(n, ctypes.c_void_p) for n in ('obs', 'actions', 'old_logp', 'old_logits', 'advantages', 'value_targets', 'old_vf', 'index')] + \
               [('index_stride', ctypes.c_int64), ('rows', ctypes.POINTER(ctypes.c_int64))]


# include/dcomp_learner_accum.h: the gradients as a running sum the caller owns (micro-batches, data-parallel ranks), then finish
ACCUM_EXPORTS = ['dcomp_learner_flat_size', 'dcomp_learner_accumulate', 'dcomp_sgd_accumulate', 'dcomp_learner_accum_finish']
ACCUM_SUMS = 8


# include/dcomp_learner_group_accum.h: the accumulators of all learners of a group, [P][flat] / [P][8], in one launch round
GROUP_ACCUM_EXPORTS = ['dcomp_learner_group_accumulate', 'dcomp_learner_group_accum_finish']


# include/dcomp_policy_set_uid.h: the set's launch keyed by UE id, for envs whose UE list changes during the episode
SET_UID_EXPORTS = ['dcomp_policy_set_actions_uid']


# include/dcomp_gae_uid.h: advantages that follow a UE through the slots of a dynamic env by its uid word
GAE_UID_EXPORTS = ['dcomp_gae_uid']


class DcompGaeUidArgs(ctypes.Structure):
    _fields_ = [('struct_size', ctypes.c_int32), ('num_steps', ctypes.c_int32), ('num_envs', ctypes.c_int32), ('num_slots', ctypes.c_int32),
                ('max_shift', ctypes.c_int32), ('gamma', ctypes.c_float), ('lambda', ctypes.c_float)] + \
               [(n, ctypes.c_void_p) for n in ('reward', 'vf', 'uid', 'uid_next', 'last_vf', 'end', 'advantages', 'value_targets', 'live')]


class DcompPpoHyper(ctypes.Structure):
    _fields_ = [('struct_size', ctypes.c_int32), ('clip_param', ctypes.c_float), ('vf_clip_param', ctypes.c_float),
                ('vf_loss_coeff', ctypes.c_float), ('entropy_coeff', ctypes.c_float), ('kl_coeff', ctypes.c_float)]


_lib = None


class DcompError(RuntimeError):
    pass


def load():
    """Load the HIP extension; raise (never fall back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build the HIP extension first (python -m deepcomp_amd.build). "
                          "deepcomp_amd has no CPU fallback.")
    # PyTorch-ROCm bundles its own libamdhip64.so.7: import it first so that this library binds to the SAME HIP
    # runtime (device pointers and streams are shared with torch); loading ours first would pull in /opt/rocm's copy.
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.dcomp_create.argtypes = [ctypes.POINTER(DcompCfg), ctypes.POINTER(vp)]        # the ABI-1 symbol: refuses (include/dcomp.h, ABI guard)
    if hasattr(L, 'dcomp_create_v'):
        L.dcomp_create_v.argtypes = [i32] + [ctypes.c_size_t] * 4 + [ctypes.POINTER(DcompCfg), ctypes.POINTER(vp)]
    L.dcomp_destroy.argtypes = [vp]
    L.dcomp_state_sizes.argtypes = [vp] + [ctypes.POINTER(ctypes.c_size_t)] * 6
    L.dcomp_obs_dim.argtypes = [vp, _ip, _ip]
    L.dcomp_reset.argtypes = [vp, ctypes.POINTER(DcompState), ctypes.POINTER(DcompTape), ctypes.POINTER(DcompOut), vp]
    L.dcomp_step.argtypes = [vp, ctypes.POINTER(DcompState), vp, ctypes.POINTER(DcompOut), vp]
    L.dcomp_step_dyn.argtypes = [vp, ctypes.POINTER(DcompState), vp, ctypes.POINTER(DcompOut), ctypes.POINTER(DcompEvents), vp]
    L.dcomp_num_ue.argtypes = [vp]
    L.dcomp_rollout.argtypes = [vp, ctypes.POINTER(DcompState), vp, i32, ctypes.POINTER(DcompOut), vp]
    if os.environ.get('DCOMP_LIB') and not hasattr(L, 'dcomp_rollout_ex'):     # a timing variant built from older sources
        EXPORTS[:] = [n for n in EXPORTS if hasattr(L, n)]
        L.dcomp_rollout_ex = L.dcomp_rollout_is_fused = lambda *a: EUNSUPPORTED
    else:
        L.dcomp_rollout_ex.argtypes = [vp, ctypes.POINTER(DcompState), vp, i32, ctypes.POINTER(DcompOut), ctypes.POINTER(DcompRolloutOpts), vp]
        L.dcomp_rollout_is_fused.argtypes = [vp]
        if hasattr(L, 'dcomp_rollout_fused_for'):
            L.dcomp_rollout_fused_for.argtypes = [vp, i32, i32, i32]
        if hasattr(L, 'dcomp_lanes_per_env'):
            L.dcomp_lanes_per_env.argtypes = [vp]
        if hasattr(L, 'dcomp_needs_conn_hi'):
            L.dcomp_needs_conn_hi.argtypes = [vp]
        if hasattr(L, 'dcomp_step_kernel_name'):
            L.dcomp_step_kernel_name.argtypes = [vp, ctypes.c_char_p, i32]
    L.dcomp_check.argtypes = [vp, ctypes.POINTER(DcompState), vp]
    L.dcomp_time.argtypes = [vp]
    L.dcomp_episode.argtypes = [vp]
    L.dcomp_episode.restype = i64
    L.dcomp_set_episode.argtypes = [vp, i64]
    if hasattr(L, 'dcomp_set_seed'):
        L.dcomp_set_seed.argtypes = [vp, ctypes.c_uint64]
        L.dcomp_set_tape.argtypes = [vp, ctypes.POINTER(DcompTape), i32]
    L.dcomp_get_counters.argtypes = [vp, ctypes.POINTER(i64)]
    L.dcomp_set_counters.argtypes = [vp, ctypes.POINTER(i64)]
    L.dcomp_mt_draw_tape.argtypes = [ctypes.POINTER(DcompCfg), ctypes.POINTER(i64), i32, i32, vp, vp]
    L.dcomp_connect_threshold.restype = ctypes.c_double
    if hasattr(L, 'dcomp_connect_boundary_sq'):
        L.dcomp_connect_boundary_sq.restype = ctypes.c_double
    L.dcomp_last_error.restype = ctypes.c_char_p
    L.dcomp_version.restype = ctypes.c_char_p
    L.dcomp_selftest.argtypes = [i32, i32, vp, vp, vp, i64, vp]
    if hasattr(L, 'dcomp_heuristic_actions'):
        L.dcomp_heuristic_actions.argtypes = [ctypes.POINTER(DcompPolicy), vp, vp, vp]
    if hasattr(L, 'dcomp_set_policy'):
        L.dcomp_set_policy.argtypes = [vp, ctypes.POINTER(DcompPolicy), vp]
    if hasattr(L, 'dcomp_pack_fragment'):
        L.dcomp_fragment_words.argtypes = [i32, i32]
        L.dcomp_pack_fragment.argtypes = [vp, i64, i32, i32, vp, vp, vp]
        L.dcomp_unpack_fragment.argtypes = [vp, i64, i32, i32, vp, vp]
    if hasattr(L, 'dcomp_actor_create'):
        L.dcomp_actor_create.argtypes = [ctypes.POINTER(DcompActorCfg), ctypes.POINTER(vp)]
        L.dcomp_actor_destroy.argtypes = [vp]
        L.dcomp_actor_actions.argtypes = [vp, ctypes.POINTER(DcompActorRun), vp, vp, vp]
    if hasattr(L, 'dcomp_actor_set_value'):
        L.dcomp_actor_set_value.argtypes = [vp, ctypes.POINTER(DcompActorValueCfg)]
        L.dcomp_actor_actions_v.argtypes = [vp, ctypes.POINTER(DcompActorRun), vp, vp, vp, vp]
        L.dcomp_gae.argtypes = [ctypes.POINTER(DcompGaeArgs), vp]
    if os.environ.get('DCOMP_LIB'):              # timing variants built from older sources lack the newest entry points
        EXPORTS[:] = [n for n in EXPORTS if hasattr(L, n)]
    if hasattr(L, 'dcomp_learner_create') or not os.environ.get('DCOMP_LIB'):
        ap = ctypes.POINTER(DcompLearnerArrays)
        L.dcomp_learner_create.argtypes = [vp, ctypes.POINTER(DcompLearnerCfg), ctypes.POINTER(vp)]
        L.dcomp_learner_destroy.argtypes = [vp]
        L.dcomp_learner_grads.argtypes = [vp, ctypes.POINTER(DcompPpoBatch), ctypes.POINTER(DcompPpoHyper), vp, vp]
        L.dcomp_learner_evaluate.argtypes = [vp, ctypes.POINTER(DcompPpoBatch), vp]
        L.dcomp_learner_apply.argtypes = [vp, ctypes.c_float, vp]
        L.dcomp_learner_read.argtypes = [vp, i32, ap, ctypes.POINTER(i64), vp]
        L.dcomp_learner_load_state.argtypes = [vp, ap, ap, ap, i64, vp]
        for name in LEARNER_EXPORTS:
            getattr(L, name)
    if hasattr(L, 'dcomp_sgd_grads') or not os.environ.get('DCOMP_LIB'):
        L.dcomp_sgd_grads.argtypes = [vp, ctypes.POINTER(DcompSgdBatch), ctypes.POINTER(DcompPpoHyper), vp, vp]
        L.dcomp_sgd_evaluate.argtypes = [vp, ctypes.POINTER(DcompSgdBatch), vp]
        for name in SGD_EXPORTS:
            getattr(L, name)
    if hasattr(L, 'dcomp_policy_set_create') or not os.environ.get('DCOMP_LIB'):
        L.dcomp_policy_set_create.argtypes = [ctypes.POINTER(DcompPolicySetCfg), ctypes.POINTER(vp)]
        L.dcomp_policy_set_destroy.argtypes = [vp]
        L.dcomp_policy_set_actions.argtypes = [vp, ctypes.POINTER(DcompActorRun), vp, vp, vp]
        L.dcomp_policy_set_actions_v.argtypes = [vp, ctypes.POINTER(DcompActorRun), vp, vp, vp, vp]
        for name in SET_EXPORTS:
            getattr(L, name)
    if hasattr(L, 'dcomp_learner_group_create') or not os.environ.get('DCOMP_LIB'):
        L.dcomp_learner_group_create.argtypes = [ctypes.POINTER(DcompLearnerGroupCfg), ctypes.POINTER(vp)]
        L.dcomp_learner_group_destroy.argtypes = [vp]
        L.dcomp_learner_group_grads.argtypes = [vp, ctypes.POINTER(DcompGroupBatch), ctypes.POINTER(DcompPpoHyper), vp, vp]
        L.dcomp_learner_group_apply.argtypes = [vp, _fp, _ip, vp]
        for name in GROUP_EXPORTS:
            getattr(L, name)
    if hasattr(L, 'dcomp_learner_accumulate') or not os.environ.get('DCOMP_LIB'):
        L.dcomp_learner_flat_size.argtypes = [vp, ctypes.POINTER(i64)]
        L.dcomp_learner_accumulate.argtypes = [vp, ctypes.POINTER(DcompPpoBatch), ctypes.POINTER(DcompPpoHyper), vp, vp, vp]
        L.dcomp_sgd_accumulate.argtypes = [vp, ctypes.POINTER(DcompSgdBatch), ctypes.POINTER(DcompPpoHyper), vp, vp, vp]
        L.dcomp_learner_accum_finish.argtypes = [vp, vp, vp, ctypes.POINTER(DcompPpoHyper), ctypes.c_float, vp, vp, vp]
        for name in ACCUM_EXPORTS:
            getattr(L, name)
    if hasattr(L, 'dcomp_learner_group_accumulate') or not os.environ.get('DCOMP_LIB'):
        L.dcomp_learner_group_accumulate.argtypes = [vp, ctypes.POINTER(DcompGroupBatch), ctypes.POINTER(DcompPpoHyper), vp, vp, vp]
        L.dcomp_learner_group_accum_finish.argtypes = [vp, vp, vp, ctypes.POINTER(DcompPpoHyper), _fp, _ip, vp, vp, vp]
        for name in GROUP_ACCUM_EXPORTS:
            getattr(L, name)
    if hasattr(L, 'dcomp_gae_uid') or not os.environ.get('DCOMP_LIB'):
        L.dcomp_gae_uid.argtypes = [ctypes.POINTER(DcompGaeUidArgs), vp]
        for name in GAE_UID_EXPORTS:
            getattr(L, name)
    if hasattr(L, 'dcomp_policy_set_actions_uid') or not os.environ.get('DCOMP_LIB'):
        L.dcomp_policy_set_actions_uid.argtypes = [vp, ctypes.POINTER(DcompActorRun), vp, vp, vp, vp, vp]
        for name in SET_UID_EXPORTS:
            getattr(L, name)
    for name in EXPORTS:
        getattr(L, name)
    _lib = L
    return L


def last_error():
    return load().dcomp_last_error().decode()


def create(cfg, handle):
    """dcomp_create_v with the sizes of THIS module's struct declarations: a library built from other headers refuses (DCOMP_EABI)
    instead of reading past a struct."""
    L = load()
    if not hasattr(L, 'dcomp_create_v'):            # DCOMP_LIB timing variants built from ABI-1 sources
        return L.dcomp_create(ctypes.byref(cfg), ctypes.byref(handle))
    return L.dcomp_create_v(ABI_VERSION, ctypes.sizeof(DcompCfg), ctypes.sizeof(DcompState), ctypes.sizeof(DcompOut),
                            ctypes.sizeof(DcompRolloutOpts), ctypes.byref(cfg), ctypes.byref(handle))


def check(rc):
    """Map a negative return code to the exception the reference raises in the same situation."""
    if rc == OK:
        return
    msg = last_error()
    if rc in (EACTION, EPOS):
        raise AssertionError(msg)          # base.py:238, central.py:61, movement.py:165
    if rc == EUNSUPPORTED:
        raise NotImplementedError(msg)     # user.py:92, central.py:73
    if rc == EINVAL:
        raise ValueError(msg)
    if rc == EABI:
        raise ImportError(msg)             # binding and library were built from different headers
    raise DcompError(f"dcomp error {rc}: {msg}")
