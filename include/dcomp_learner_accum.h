/* dcomp_learner_accum.h -- the PPO learner's gradients as a running sum the caller owns (dcomp_learner.h has the learner itself;
 * dcomp_learner_indexed.h the minibatches picked through a row index).
 *
 * dcomp_learner_grads sums its f32 partials per fixed row chunk in chunk order, applies 1 / N once and writes the handle's gradients.
 * Here the running sum stays in a buffer of the caller's and is NOT scaled, so that
 *   micro-batches of one minibatch accumulate into it (a minibatch larger than the handle's max_rows),
 *   the ranks of a data-parallel learner add theirs together (an all-reduce of acc and sums between accumulate and finish),
 *   and dcomp_learner_accum_finish applies 1 / N of the GLOBAL row count once, clips by the global norm when asked to, and leaves
 *   the gradients where dcomp_learner_apply reads them.
 * When every call but the last has a multiple of the whole batch's chunk rows, and the whole batch has at most 262 144 rows (one
 * chunk = 2 048 rows), the f32 additions are those of dcomp_learner_grads on the whole batch in the same order: the gradients are
 * bit-identical.  Beyond that the two differ by f32 re-association only.  No floating-point atomics anywhere: every order is fixed
 * and repeats are bit-identical.
 *
 * Struct sizes, errors and validation as in dcomp_learner.h: everything is checked on the host before the first HIP call; every call
 * only enqueues on `stream`, allocates nothing and does not synchronise. */
#ifndef DCOMP_LEARNER_ACCUM_H
#define DCOMP_LEARNER_ACCUM_H

#include "dcomp_learner_indexed.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCOMP_ACCUM_SUMS 8   /* doubles: sum surrogate, sum kl, sum entropy, sum vf loss (the four of the per-tile workspace, same signs),
                                counted rows, three reserved (left 0) */

/* *floats = the elements of the handle's flat gradient array: the twelve arrays of dcomp_learner_arrays one behind the other. */
int dcomp_learner_flat_size(const dcomp_learner *l, int64_t *floats);

/* dcomp_learner_grads / dcomp_sgd_grads up to the chunk partials, then: acc[e] = acc[e] + part_0[e] + part_1[e] + ... added one at a
 * time in chunk order in f32 (s = acc[e]; for c: s += part[c]), NOT scaled; sums[0..3] += the batch's four loss sums (double),
 * sums[4] += the rows that count.  The handle's gradients and statistics are not written.  acc_dev [flat_size] f32 and sums_dev
 * [DCOMP_ACCUM_SUMS] f64 are the caller's, zeroed by the caller before a minibatch's first call.  Every check of the grads calls is
 * made; upstream gradients (batch.dlogits / dvalue) are refused with DCOMP_EINVAL: they are plain sums already. */
int dcomp_learner_accumulate(dcomp_learner *l, const dcomp_ppo_batch *batch, const dcomp_ppo_hyper *hyper, float *acc_dev, double *sums_dev,
                             void *stream);
int dcomp_sgd_accumulate(dcomp_learner *l, const dcomp_sgd_batch *batch, const dcomp_ppo_hyper *hyper, float *acc_dev, double *sums_dev,
                         void *stream);

/* g[e] = acc[e] * (float)(1.0 / sums[4]) -> the handle's gradients (what dcomp_learner_apply consumes); the five statistics from
 * sums as dcomp_learner_grads forms them from its totals -> stats_dev (may be NULL; hyper gives the three loss coefficients).
 * grad_clip > 0: the global L2 norm of g over all twelve arrays, accumulated in double in a fixed order, -> *grad_norm_dev (f32, may
 * be NULL), and g *= (float)min(1.0, grad_clip / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_).  grad_clip == 0: no clipping (the
 * norm is still written when asked for); < 0 or NaN: DCOMP_EINVAL.  Reads acc and sums, leaves both unchanged (it can be called
 * again). */
int dcomp_learner_accum_finish(dcomp_learner *l, const float *acc_dev, const double *sums_dev, const dcomp_ppo_hyper *hyper, float grad_clip,
                               float *stats_dev, float *grad_norm_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif
