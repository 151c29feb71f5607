/* dcomp_policy_set.h -- one policy network per UE (D3-CoMP, --separate-agent-nns: env_setup.py:295 keys the policy map by UE) run in
 * ONE actor launch: a set over existing dcomp_actor handles (dcomp.h: dcomp_actor_create / dcomp_actor_set_value).
 *
 * A set maps every UE slot u of a DCOMP_MULTI env to one of its P member handles (slot_policy).  dcomp_policy_set_actions[_v] does
 * what dcomp_actor_actions[_v] does -- same dcomp_actor_run, same observation formats, same [E][U] outputs at the same addresses,
 * same draws (keyed by row_base + row) -- with the row of slot u going through the weights of member slot_policy[u].  A row's results
 * are bit-identical to those of its member's own launch over the same batch.
 *
 * The set copies NO weights: it holds one small device table with, per slot, the pointers into its member's packed device images.
 * dcomp_learner_apply / dcomp_learner_load_state on a member rewrite those images in place, so the set's next launch on the stream
 * runs the new weights with no call in between.  The members must outlive the set, and stay on its device.
 *
 * The table is written at create from the trunks the members have THEN.  Attach value functions (dcomp_actor_set_value, once per
 * handle) BEFORE creating the set: the set records its members' value form, and once a member's differs from it every
 * dcomp_policy_set_actions[_v] call fails with DCOMP_EINVAL on the host -- create a new set over the members instead.
 *
 * Struct sizes, errors (dcomp_last_error()) and validation as in dcomp.h: everything is checked on the host before the first HIP
 * call.  dcomp_policy_set_create checks in this order: what needs no dereference of a member (NULL cfg / out / members: DCOMP_EINVAL;
 * struct_size: DCOMP_EABI; num_policies outside 1 ... DCOMP_MAX_UE, a NULL member: DCOMP_EINVAL); that the members agree (DCOMP_EINVAL);
 * forms that agree but are not supported -- DCOMP_CENTRAL members (one network by construction), a shared value function
 * (dcomp_actor_value_cfg.shared = 1) -- DCOMP_EUNSUPPORTED; the range of slot_policy (DCOMP_EINVAL).
 *
 * Envs whose UE list changes during the episode (dcomp_step_dyn) shift their slots when a UE leaves, so a slot is not one UE there:
 * dcomp_policy_set_uid.h has the launch on this handle that picks a row's member by the UE id in the env's uid word instead. */
#ifndef DCOMP_POLICY_SET_H
#define DCOMP_POLICY_SET_H

#include "dcomp_types.h"

#ifndef DCOMP_EABI
#define DCOMP_EABI (-7)        /* as in dcomp.h: caller and library disagree about a struct size */
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dcomp_policy_set dcomp_policy_set;

typedef struct dcomp_policy_set_cfg {
    int32_t struct_size;             /* sizeof(dcomp_policy_set_cfg) of the caller */
    int32_t num_policies;            /* P >= 1 */
    dcomp_actor *const *members;     /* P handles, all: DCOMP_MULTI, same num_ue / num_bs / hidden / activation / device,
                                        same value form: none, or a trunk of its own (shared = 0) */
    const int32_t *slot_policy;      /* [num_ue], entries in [0, P): the policy of UE slot u.  NULL: slot u -> u % P */
} dcomp_policy_set_cfg;

int dcomp_policy_set_create(const dcomp_policy_set_cfg *cfg, dcomp_policy_set **out);
int dcomp_policy_set_destroy(dcomp_policy_set *s);

/* dcomp_actor_actions / dcomp_actor_actions_v over the set: one launch, only enqueues on `stream`, allocates nothing.  _v needs
 * members with a value function; action == NULL is the value-only call (run.logits and run.logp must be NULL). */
int dcomp_policy_set_actions  (dcomp_policy_set *s, const dcomp_actor_run *run, const void *obs, uint8_t *action, void *stream);
int dcomp_policy_set_actions_v(dcomp_policy_set *s, const dcomp_actor_run *run, const void *obs, uint8_t *action, float *vf, void *stream);

#ifdef __cplusplus
}
#endif
#endif
