/* dcomp_learner_group_accum.h -- the accumulated gradients (dcomp_learner_accum.h) of all learners of a group (dcomp_learner_group.h)
 * in one launch round: micro-batches, grad_clip and data-parallel ranks for a per-UE policy set (dcomp_policy_set.h: D3-CoMP).
 *
 * Through the per-member calls a micro-batch round of P policies is 3 P launches (dcomp_sgd_accumulate), a finish 2 P
 * (dcomp_learner_accum_finish), and a data-parallel set all-reduces P gradients per minibatch.  Here the accumulators of all members
 * are ONE buffer each -- acc_dev [P][flat] f32 and sums_dev [P][DCOMP_ACCUM_SUMS] f64, member p's slice at acc_dev + p flat and
 * sums_dev + DCOMP_ACCUM_SUMS p, flat = dcomp_learner_flat_size of a member (the members have one shape: one number) -- so a micro-batch
 * round is three launches per DCOMP_GROUP_SLICE policies, a finish two, and the ranks meet twice per minibatch whatever P is.
 *
 * What a member's slices and its handle hold afterwards is BIT-IDENTICAL to what the per-member calls leave there: the running sum is
 * carried in, the chunk partials are added in chunk order, the four loss sums in the same 256 ranges, the count is rows[p]; the norm
 * partials go through the member's own workspace in the same fixed order.  So grouped and per-member calls mix freely, and the
 * chunk-aligned guarantee of dcomp_learner_accum.h holds per member.  No floating-point atomics: a thread owns its entry of acc, one
 * thread per policy owns that policy's sums.
 *
 * Struct sizes, errors and validation as in dcomp_learner.h: everything is checked on the host before the first HIP call; a call only
 * enqueues on `stream`, allocates nothing and does not synchronise.
 *
 * dcomp_learner_group_accumulate checks in this order: NULL group / batch / hyper / acc_dev / sums_dev (DCOMP_EINVAL); batch.struct_size
 * (DCOMP_EABI); NULL batch.rows / batch.index; then per member in order: rows[p] outside [0, max_rows of p], rows[p] > index_stride, and
 * for rows[p] > 0 every check dcomp_learner_group_grads makes of that member's call (hyper[p].struct_size: DCOMP_EABI); every rows[p]
 * == 0; the device.
 * dcomp_learner_group_accum_finish: NULL group / acc_dev / sums_dev / hyper (DCOMP_EINVAL); then per ACTIVE member in order:
 * hyper[p].struct_size (DCOMP_EABI), grad_clip[p] negative or NaN (DCOMP_EINVAL); no active member (DCOMP_EINVAL); the device. */
#ifndef DCOMP_LEARNER_GROUP_ACCUM_H
#define DCOMP_LEARNER_GROUP_ACCUM_H

#include "dcomp_learner_group.h"
#include "dcomp_learner_accum.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dcomp_sgd_accumulate for every member with rows[p] > 0 (batch as dcomp_learner_group_grads takes it), on that member's slices of
 * acc_dev / sums_dev: acc += the chunk partials in chunk order, unscaled; sums[0..3] += the four loss sums, sums[4] += rows[p].  The
 * handles' gradients and statistics are not written.  A member with rows[p] == 0 sits the call out: its slices are not touched.  At
 * least one member must be active.  hyper: a HOST array of P structs.  The caller zeroes the slices before a minibatch's first call. */
int dcomp_learner_group_accumulate(dcomp_learner_group *g, const dcomp_group_batch *batch, const dcomp_ppo_hyper *hyper, float *acc_dev,
                                   double *sums_dev, void *stream);

/* dcomp_learner_accum_finish for every member p with active[p] != 0 (active = NULL: all): g = acc * (float)(1 / sums[4]) into the
 * member's handle, the five statistics from sums with hyper[p]'s coefficients into stats_dev[p] (stats_dev [P][DCOMP_PPO_NUM_STATS],
 * may be NULL), the global L2 norm of the member's g into grad_norm_dev[p] (f32 [P], may be NULL), and g scaled by
 * min(1, grad_clip[p] / (norm + 1e-6)) where grad_clip[p] > 0.  grad_clip: a HOST array [P], NULL or 0: no clipping (the norm is still
 * written when asked for); negative or NaN: DCOMP_EINVAL.  An inactive member keeps its gradients, its row of stats_dev and its entry
 * of grad_norm_dev.  acc_dev and sums_dev are read only (the call can be repeated). */
int dcomp_learner_group_accum_finish(dcomp_learner_group *g, const float *acc_dev, const double *sums_dev, const dcomp_ppo_hyper *hyper,
                                     const float *grad_clip, const int32_t *active, float *stats_dev, float *grad_norm_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif
