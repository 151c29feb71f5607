/* dcomp_learner.h -- the PPO learner of the fcnet policy a dcomp_actor runs (dcomp.h: dcomp_actor_create / dcomp_actor_set_value):
 * loss, backward pass and Adam on the device, on the train batch deepcomp_amd.sampler.collect leaves in HBM.
 *
 * The arithmetic is the specification; deepcomp_amd/learner.py spells it out on the CPU (ppo_loss_reference, adam_reference):
 *   forward   the actor's chain: x = bf16(row); h1 = bf16(act(x W1 + b1)); h2 = bf16(act(h1 W2 + b2)); logits = h2 W3 + b3, and
 *             the value trunk of its own the same way (f32 accumulation, bias and activation in f32)
 *   loss      RLlib's ppo_surrogate_loss per decision row in f32: ratio = exp(logp - old logp), the clipped surrogate, KL(old || new)
 *             from old_logits, the entropy, the clipped value loss; the mean over the counted rows
 *   backward  dlogits / dvalue in f32, rounded to bf16 where they become matrix operands; dA2 = bf16((W3 dlogits) * act'(h2)),
 *             dA1 likewise (act' from the stored bf16 h: tanh 1 - h^2, relu h > 0); dW = sum over rows of a (x) d with bf16 a, d
 *             and f32 sums over fixed row chunks, reduced in a fixed order; db = the f32 column sums of the bf16 d; 1 / N once, in
 *             f32, after the sum over rows
 *   Adam      torch.optim.Adam's update as f32 operations each rounded on its own; the bias corrections come from the host in double
 * The same batch and weights give bit-identical gradients and statistics on every run: no floating-point atomics, and the row
 * split depends on the row count alone.
 *
 * Supported: DCOMP_MULTI and DCOMP_CENTRAL, tanh and relu, any hidden width the actor takes, a value trunk of its own
 * (vf_share_layers=False, PPO's default).  The shared value (dcomp_actor_value_cfg.shared = 1) and the compact record as learner
 * input are refused with DCOMP_EUNSUPPORTED by the calls here, which take a contiguous minibatch of rows; dcomp_learner_indexed.h has
 * the calls that pick a minibatch through a row index out of a whole sample batch, rows or compact record.
 *
 * Every struct carries its own size as its first field (anything else -> DCOMP_EABI); DCOMP_ABI_VERSION is unaffected.  Errors are
 * reported through dcomp_last_error().  Everything is validated on the host before the first HIP call. */
#ifndef DCOMP_LEARNER_H
#define DCOMP_LEARNER_H

#include "dcomp_types.h"

#ifndef DCOMP_EABI
#define DCOMP_EABI (-7)        /* as in dcomp.h: caller and library disagree about a struct size */
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dcomp_learner dcomp_learner;

#define DCOMP_PPO_NUM_STATS 5      /* stats_dev: total_loss, policy_loss (= -mean surrogate), vf_loss, kl, entropy */
enum { DCOMP_LEARNER_WEIGHTS = 0, DCOMP_LEARNER_GRADS = 1, DCOMP_LEARNER_ADAM_M = 2, DCOMP_LEARNER_ADAM_V = 3 };

/* The twelve f32 arrays of the policy and of its value trunk, each in the natural [in][out] layout of a TF / RLlib kernel. */
typedef struct dcomp_learner_arrays {
    int32_t struct_size;          /* sizeof(dcomp_learner_arrays) of the caller */
    int32_t reserved;             /* 0 */
    float *w1, *b1, *w2, *b2, *w3, *b3;            /* the policy: [inputs][hidden], [hidden], [hidden][hidden], [hidden], [hidden][logits], [logits] */
    float *vw1, *vb1, *vw2, *vb2, *wv, *bv;        /* the value trunk: as the policy's, then value_out [hidden], [1] */
} dcomp_learner_arrays;

typedef struct dcomp_learner_cfg {
    int32_t struct_size;          /* sizeof(dcomp_learner_cfg) of the caller */
    int32_t value_shared;         /* must be 0: the value function is a trunk of its own (1 -> DCOMP_EUNSUPPORTED) */
    int64_t max_rows;             /* decision rows of the largest (mini)batch; every workspace is sized by it */
    float beta1, beta2, eps;      /* Adam's (torch.optim.Adam: 0.9, 0.999, 1e-8) */
    int32_t reserved;             /* 0 */
    const dcomp_learner_arrays *weights;           /* HOST f32 master weights: what the actor and its value function were built from */
} dcomp_learner_cfg;

/* One (mini)batch, every pointer a device pointer.  rows are decision rows as in dcomp_actor_actions: DCOMP_MULTI one per (env, UE
 * slot), the slot of row i being i % num_ue; DCOMP_CENTRAL one per env.  num_active as in dcomp_actor_run: a multi row whose slot is
 * >= num_active contributes nothing and is not counted in the mean (its inputs are not read); central heads >= num_active are
 * left out of logp, kl and the entropy. */
typedef struct dcomp_ppo_batch {
    int32_t struct_size;          /* sizeof(dcomp_ppo_batch) of the caller */
    int32_t obs_format;           /* DCOMP_ACTOR_ROWS (DCOMP_ACTOR_COMPACT -> DCOMP_EUNSUPPORTED) */
    int64_t rows;
    int32_t num_active;
    int32_t reserved;             /* 0 */
    const float *obs;             /* [rows][inputs] */
    const uint8_t *actions;       /* [rows][heads] */
    const float *old_logp;        /* [rows][heads]: action_logp of the sample batch */
    const float *old_logits;      /* [rows][logits]: action_dist_inputs of the sample batch */
    const float *advantages;      /* [rows] */
    const float *value_targets;   /* [rows] */
    const float *old_vf;          /* [rows]: vf_preds of the sample batch */
    /* optional per-row outputs (NULL: not written) */
    float *logp;                  /* [rows][heads]: log-probability of the given action under the current weights */
    float *entropy;               /* [rows]: summed over the heads */
    float *kl;                    /* [rows]: summed over the heads */
    float *vf;                    /* [rows] */
    float *ratio;                 /* [rows] */
    /* optional upstream gradients, both or neither: used INSTEAD of the PPO loss's (actions ... old_vf may then be NULL, the
     * statistics are zero and no 1 / N is applied: gradients are plain sums over the rows) */
    const float *dlogits;         /* [rows][logits] */
    const float *dvalue;          /* [rows] */
} dcomp_ppo_batch;

typedef struct dcomp_ppo_hyper {
    int32_t struct_size;          /* sizeof(dcomp_ppo_hyper) of the caller */
    float clip_param;             /* RLlib: 0.3 */
    float vf_clip_param;          /* 10 */
    float vf_loss_coeff;          /* 1 */
    float entropy_coeff;          /* 0 */
    float kl_coeff;               /* 0.2 */
} dcomp_ppo_hyper;

/* dcomp_learner_create: a learner on the actor `a` (which needs dcomp_actor_set_value with shared = 0 first, and must outlive the
 * learner).  Uploads the master weights, allocates everything the other calls need, and writes the packed bf16 weights of the
 * actor handle from the masters (bit-identical to what dcomp_actor_create / dcomp_actor_set_value pack from the same arrays). */
int dcomp_learner_create(dcomp_actor *a, const dcomp_learner_cfg *cfg, dcomp_learner **out);
int dcomp_learner_destroy(dcomp_learner *l);

/* Loss statistics -> stats_dev[DCOMP_PPO_NUM_STATS] (device) and the gradients of all twelve arrays -> the handle.  Enqueues on
 * `stream` and allocates nothing. */
int dcomp_learner_grads(dcomp_learner *l, const dcomp_ppo_batch *batch, const dcomp_ppo_hyper *hyper, float *stats_dev, void *stream);

/* The forward pass alone on given actions: batch.logp / entropy / vf (at least one non-NULL) from obs and actions; the handle's
 * gradients are left alone.  old_* , advantages and value_targets are not read. */
int dcomp_learner_evaluate(dcomp_learner *l, const dcomp_ppo_batch *batch, void *stream);

/* One Adam step on the handle's gradients (step count + 1), then the actor handle's packed bf16 weights are rewritten in the same
 * launch: the actor's next launch on `stream` runs the new weights, with no host copy and no synchronisation. */
int dcomp_learner_apply(dcomp_learner *l, float lr, void *stream);

/* Copy master weights, gradients or moments (DCOMP_LEARNER_*) to the HOST arrays of dst (NULL members are skipped), after
 * synchronising with `stream`.  *step (may be NULL) receives the number of Adam steps taken. */
int dcomp_learner_read(dcomp_learner *l, int32_t which, const dcomp_learner_arrays *dst, int64_t *step, void *stream);

/* Checkpoint / resume: master weights, both moments (every member non-NULL, HOST) and the step count go back into the handle, and
 * the actor's packed weights are rewritten from the masters. */
int dcomp_learner_load_state(dcomp_learner *l, const dcomp_learner_arrays *weights, const dcomp_learner_arrays *adam_m,
                             const dcomp_learner_arrays *adam_v, int64_t step, void *stream);

#ifdef __cplusplus
}
#endif
#endif
