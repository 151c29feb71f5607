/* dcomp_learner_indexed.h -- the PPO learner's minibatches picked through a row index out of a whole sample batch (dcomp_learner.h
 * has the learner itself: create, apply, read, load_state, and the calls on a contiguous minibatch).
 *
 * PPO's SGD phase walks a shuffled sample batch in minibatches.  dcomp_learner_grads takes a contiguous minibatch, so its caller
 * gathers seven tensors per minibatch; here the kernel reads every per-row input of minibatch position i at SOURCE ROW index[i] of
 * the sample batch where it lies.  That is also what makes the compact record (DCOMP_ACTOR_COMPACT, dcomp_out.obs_compact /
 * dcomp_pack_fragment) a learner input: a record holds a whole env and cannot be gathered row by row, but input k of source row s is
 * decoded from the record of env s / num_ue, slot s % num_ue, by the rule dcomp_actor_actions reads it with.  A sample batch
 * collected as records trains without an observation row ever being written.
 *
 * The arithmetic is dcomp_learner_grads' on the gathered rows, bit for bit: the same values are staged at the same positions, and
 * the workspaces, the row split of the weight gradients and the order of every sum depend on `rows` alone.
 *
 * An index entry outside [0, source_rows) is never dereferenced: the position is computed on zeros with zero deltas like a row
 * beyond the batch, its per-row outputs are 0, and it still counts in the 1 / N of the mean.  A bad index gives wrong numbers,
 * never a fault.
 *
 * Struct sizes, errors and validation as in dcomp_learner.h: everything is checked on the host before the first HIP call. */
#ifndef DCOMP_LEARNER_INDEXED_H
#define DCOMP_LEARNER_INDEXED_H

#include "dcomp_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One minibatch of `rows` positions out of a sample batch of `source_rows` decision rows, every pointer a device pointer.  Decision
 * rows are those of dcomp_ppo_batch: DCOMP_MULTI one per (env, UE slot), row s being slot s % num_ue of env s / num_ue (a sample
 * batch [T][E][U] flattened: env t E + e); DCOMP_CENTRAL one per env.
 * num_active: DCOMP_CENTRAL as in dcomp_ppo_batch (heads >= num_active are left out of logp, kl and the entropy).  DCOMP_MULTI: must
 * equal num_ue -- rows of unlisted slots are left out by not listing them in the index, and every position counts in 1 / N. */
typedef struct dcomp_sgd_batch {
    int32_t struct_size;          /* sizeof(dcomp_sgd_batch) of the caller */
    int32_t obs_format;           /* DCOMP_ACTOR_ROWS | DCOMP_ACTOR_COMPACT (DCOMP_MULTI only) */
    int64_t rows;                 /* minibatch positions, <= max_rows of the handle */
    int64_t source_rows;          /* decision rows of the sample batch the pointers address, <= 2^31 - 1 */
    const int32_t *index;         /* [rows]; NULL: position i reads source row i (then rows <= source_rows) */
    int32_t num_active;
    int32_t reserved;             /* 0 */
    const void *obs;              /* [source_rows][inputs] f32, or the records of source_rows / num_ue envs (a multiple of num_ue) */
    const uint8_t *actions;       /* [source_rows][heads] */
    const float *old_logp;        /* [source_rows][heads] */
    const float *old_logits;      /* [source_rows][logits] */
    const float *advantages;      /* [source_rows] */
    const float *value_targets;   /* [source_rows] */
    const float *old_vf;          /* [source_rows] */
    /* optional upstream gradients, both or neither, as in dcomp_ppo_batch */
    const float *dlogits;         /* [source_rows][logits] */
    const float *dvalue;          /* [source_rows] */
    /* optional per-row outputs (NULL: not written), at the minibatch POSITION */
    float *logp;                  /* [rows][heads] */
    float *entropy;               /* [rows] */
    float *kl;                    /* [rows] */
    float *vf;                    /* [rows] */
    float *ratio;                 /* [rows] */
} dcomp_sgd_batch;

/* dcomp_learner_grads on the rows the index picks: statistics -> stats_dev[DCOMP_PPO_NUM_STATS], gradients -> the handle.  Enqueues
 * on `stream`, allocates nothing, does not synchronise. */
int dcomp_sgd_grads(dcomp_learner *l, const dcomp_sgd_batch *batch, const dcomp_ppo_hyper *hyper, float *stats_dev, void *stream);

/* dcomp_learner_evaluate on the rows the index picks: batch.logp / entropy / vf (at least one non-NULL). */
int dcomp_sgd_evaluate(dcomp_learner *l, const dcomp_sgd_batch *batch, void *stream);

#ifdef __cplusplus
}
#endif
#endif
