/* dcomp_policy_set_uid.h -- a policy set (dcomp_policy_set.h) keyed by UE ID: the launch for envs whose UE list changes during the
 * episode (dcomp_step_dyn), where slots shift when a UE leaves and a slot is not one UE.  The reference's --separate-agent-nns keys its
 * policy map by ue.id and creates a policy for every UE the episode will ever see (get_num_diff_ues()); here that is a set of P members,
 * member p being the policy of the UE with id p + 1, launched with the env's uid words (dcomp_state.uid, dcomp_gae_uid.h: the UE's 1-based
 * id, bit 15 set when it arrived during the episode, 0 for a dead slot).
 *
 * dcomp_policy_set_actions_uid is ONE more entry point on the dcomp_policy_set handle.  The row at (env, slot) goes through member
 * id - 1 with id = uid[env][slot] & 0x7FFF; bit 15 does not enter the choice, and neither does the set's slot_policy.  Everything else
 * is the shared launch's: a live row's outputs land at the addresses dcomp_actor_actions[_v] has them, its draws are keyed by seed, step,
 * row_base + env U + slot, head and action -- so its action, logp, logits and vf are, bit for bit, those of its member's own
 * dcomp_actor_actions[_v] launch over the same batch (a row is one column of the B operand, as for the slot-keyed set).
 *
 * Slots whose word is 0 and slots whose id exceeds P get action 0 and 0.0f in every optional output.  Every entry of every output passed
 * in is written exactly once by the call and nothing outside them; no value at such a row of obs, NaN included, reaches any output.
 *
 * What the kernel assumes of the words (it is what dcomp_step_dyn writes): the non-zero words of an env's row are distinct and a prefix
 * of it.  Words that break this give wrong numbers (a row written twice or not at all), never a fault: whatever they hold, every index
 * stays inside the env's own row and inside [0, P) -- dcomp_gae_uid.h's promise.
 *
 * One launch; it only enqueues on `stream` and allocates nothing (the handle got a second device table at create, [P][2] trunks in
 * member order).  Both observation formats, sample 0 and 1, every width and activation of the members; the value form is 0 or 1.
 * Checked on the host before the first HIP call, in dcomp_policy_set_actions_v's order (vf == NULL is the call without a value and
 * needs no value function), and after those: uid == NULL; run.num_active != num_ue (the uid words say which slots are listed);
 * action == NULL && vf == NULL (all DCOMP_EINVAL).  As for every call on the set, members must have got their value functions before
 * the set was created. */
#ifndef DCOMP_POLICY_SET_UID_H
#define DCOMP_POLICY_SET_UID_H

#include "dcomp_policy_set.h"

#ifdef __cplusplus
extern "C" {
#endif

int dcomp_policy_set_actions_uid(dcomp_policy_set *s, const dcomp_actor_run *run, const void *obs,
                                 const uint16_t *uid,   /* device [E][U]: dcomp_state.uid, the layout obs stands in */
                                 uint8_t *action,       /* [E][U]; NULL: the value-only call (run.logits / run.logp NULL) */
                                 float *vf,             /* [E*U] or NULL; needs members with a value trunk of their own */
                                 void *stream);

#ifdef __cplusplus
}
#endif
#endif
