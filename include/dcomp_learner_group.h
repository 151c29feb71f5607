/* dcomp_learner_group.h -- the PPO learners of a per-UE policy set (dcomp_policy_set.h: D3-CoMP) trained together: ONE launch round
 * per minibatch round for all P policies, where P dcomp_sgd_grads + dcomp_learner_apply calls are 4 P launches.
 *
 * A group is a list of existing dcomp_learner handles (dcomp_learner.h) of one shape.  dcomp_learner_group_grads does for every
 * member what dcomp_sgd_grads (dcomp_learner_indexed.h) does for one: policy p's minibatch is rows[p] positions, position i reading
 * source row index[p index_stride + i] of ONE shared sample batch (the policies' rows are disjoint subsets of it), with policy p's
 * hyper-parameters; its gradients go to member p's handle and its statistics to stats_dev[p].  dcomp_learner_group_apply is
 * dcomp_learner_apply for every active member with its own lr and its own step count.  Both are four kernels with the policy as a
 * grid dimension (forward + loss + backward, weight gradients, reduce; Adam), launched once per DCOMP_GROUP_SLICE policies: the
 * per-call values of a policy (rows, hyper-parameters, Adam's scalars) travel in the kernel arguments, so a call allocates nothing,
 * copies nothing and does not synchronise.
 *
 * What a member's handle holds afterwards is BIT-IDENTICAL to what the per-learner calls leave there: the arithmetic of a policy is
 * unchanged, its row split and the order of every sum depend on rows[p] alone, and Adam's bias corrections come from the host in
 * double, per member.  So group calls and per-learner calls on a member can be mixed freely: apply advances the member's own step
 * count, and dcomp_learner_read / dcomp_learner_load_state see the member as ever.
 *
 * The group copies NO weights and owns one small device table (per member: its net, workspaces and array descriptions, written at
 * create).  The learners (and their actors) must outlive the group and stay on its device.
 *
 * A policy with rows[p] = 0 sits a call out: its gradients and its row of stats_dev are left untouched.  An index entry outside
 * [0, source_rows) behaves as in dcomp_sgd_grads: never dereferenced, zeros, counted in 1 / N.  There are no per-row outputs and no
 * upstream gradients here; the per-learner calls keep those.
 *
 * Struct sizes, errors (dcomp_last_error()) and validation as in dcomp_learner.h: everything is checked on the host before the first
 * HIP call.  dcomp_learner_group_create checks in this order: NULL cfg / out / learners (DCOMP_EINVAL); struct_size (DCOMP_EABI);
 * num_learners outside 1 ... DCOMP_MAX_UE, a NULL or repeated learner (DCOMP_EINVAL); learners that disagree in shape, activation or
 * device (DCOMP_EINVAL); DCOMP_CENTRAL learners (DCOMP_EUNSUPPORTED: a central policy is one network). */
#ifndef DCOMP_LEARNER_GROUP_H
#define DCOMP_LEARNER_GROUP_H

#include "dcomp_learner_indexed.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCOMP_GROUP_SLICE 64       /* policies per launch: a larger group goes as ceil(P / DCOMP_GROUP_SLICE) launch rounds */

typedef struct dcomp_learner_group dcomp_learner_group;

typedef struct dcomp_learner_group_cfg {
    int32_t struct_size;             /* sizeof(dcomp_learner_group_cfg) of the caller */
    int32_t num_learners;            /* P, 1 ... DCOMP_MAX_UE */
    dcomp_learner *const *learners;  /* P distinct handles on distinct actors: DCOMP_MULTI, same num_ue / num_bs / hidden / activation / device */
} dcomp_learner_group_cfg;

/* dcomp_sgd_batch for P learners over one source batch; every pointer but `rows` a device pointer. */
typedef struct dcomp_group_batch {
    int32_t struct_size;          /* sizeof(dcomp_group_batch) of the caller */
    int32_t obs_format;           /* DCOMP_ACTOR_ROWS | DCOMP_ACTOR_COMPACT */
    int64_t source_rows;          /* decision rows of the sample batch the pointers address, <= 2^31 - 1 */
    const void *obs;              /* [source_rows][inputs] f32, or the records of source_rows / num_ue envs */
    const uint8_t *actions;       /* [source_rows] */
    const float *old_logp;        /* [source_rows] */
    const float *old_logits;      /* [source_rows][logits] */
    const float *advantages;      /* [source_rows] */
    const float *value_targets;   /* [source_rows] */
    const float *old_vf;          /* [source_rows] */
    const int32_t *index;         /* [P][index_stride]: policy p's positions -> source rows */
    int64_t index_stride;
    const int64_t *rows;          /* HOST [P]: policy p's minibatch positions, 0 ... min(max_rows of p, index_stride); 0: p sits this call out */
} dcomp_group_batch;

int dcomp_learner_group_create(const dcomp_learner_group_cfg *cfg, dcomp_learner_group **out);
int dcomp_learner_group_destroy(dcomp_learner_group *g);

/* dcomp_sgd_grads for every policy with rows[p] > 0: hyper is a HOST array of P structs (kl_coeff adapts per policy), stats_dev a
 * device array [P][DCOMP_PPO_NUM_STATS].  At least one policy must be active.  Enqueues on `stream`, allocates nothing, does not
 * synchronise. */
int dcomp_learner_group_grads(dcomp_learner_group *g, const dcomp_group_batch *batch, const dcomp_ppo_hyper *hyper, float *stats_dev, void *stream);

/* dcomp_learner_apply for every member p with active[p] != 0 (active = NULL: all): one Adam step with lr[p] on the member's
 * gradients, step count + 1, the member's actor rewritten.  lr and active are HOST arrays [P]. */
int dcomp_learner_group_apply(dcomp_learner_group *g, const float *lr, const int32_t *active, void *stream);

#ifdef __cplusplus
}
#endif
#endif
