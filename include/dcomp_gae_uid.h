/* dcomp_gae_uid.h -- generalised advantage estimation that follows a UE through the slots of an env whose UE list changes during
 * the episode (dcomp.h has dcomp_gae, the estimator of a static layout: a column there is one trajectory).
 *
 * What a dynamic multi-agent env writes (dcomp_step_dyn; csrc/dcomp_dyn.h).  An env has U = max_ues slots, slot s being position s
 * of the reference's ue_list.  dcomp_state.uid holds one 16-bit word per slot: the UE's 1-based id, bit 15 set when the UE arrived
 * during the episode, 0 for a dead slot.  A step applies the actions in the layout it finds, then the events -- a departure is
 * ue_list.pop(i): the slots behind i move up by one; an arrival appends -- then the rates, the reward and the observation.  So with
 * uid[t] the words BEFORE step t and uid_next[t] the words AFTER it (and before a reset at the horizon):
 *     obs[t], actions[t], vf[t]   are in the layout of uid[t],
 *     reward[t], the next obs     are in the layout of uid_next[t],
 * and inside an episode uid[t + 1] = uid_next[t].
 *
 * What is computed, the `end` convention of dcomp_gae per UE.  Row (t, e, s) COUNTS (live = 1) iff its word w = uid[t][e][s] is not 0
 * and occurs in uid_next[t][e][.], at slot s': the UE acted and was still listed after the step.  A counted row's reward is
 * reward[t][e][s'] and its successor is row (t + 1, e, s').  With (nv, A) = (vf, advantage) of the successor,
 *     d = (reward + gamma nv) - vf[t][e][s];  A' = d + (gamma lambda) A;  advantages = A';  value_targets = A' + vf[t][e][s]
 * as f32 operations each rounded on its own, in this order (dcomp_gae's).  (nv, A) = (0, 0) where end[t] is set and where the
 * successor does not count (the UE departs in step t + 1); at t = T - 1 without end, (nv, A) = (last_vf[e][s'], 0).  The row of the
 * step in which a UE departs does not count (it has an action, but neither a reward nor a next observation), and the reward an
 * arriving UE gets before its first action is dropped.  On a static layout -- every row of uid and uid_next holding the same distinct
 * non-zero words -- the advantages and value targets are dcomp_gae's, bit for bit, and live is 1 everywhere.
 *
 * What the kernel assumes of a trace (it is what dcomp_step_dyn writes), per env and step:
 *   - the non-zero words of a row are a prefix of it (live slots first) and distinct;
 *   - survivors keep their order from uid[t] to uid_next[t], so a UE at slot s is found at a slot s' in [s - k, s], k being the
 *     departures of the step;
 *   - max_shift >= 0: no step has more than max_shift departures (the search looks at s, s - 1, ..., s - max_shift only);
 *     max_shift < 0: unknown, the whole prefix s, s - 1, ..., 0 is searched.
 * A trace that breaks these gives wrong numbers, never a fault: every index stays inside the env's own row.
 *
 * Every output word is written: positions that do not count get advantages = value_targets = 0.0f and live = 0.  No value at a dead
 * or unmatched position -- a reward nobody's s' points at, vf or last_vf of a row that does not count, NaN included -- influences
 * any output.  The outputs must not overlap the inputs.
 *
 * The struct carries its own size as its first field (anything else -> DCOMP_EABI).  Everything is checked on the host before the
 * first HIP call, in dcomp_gae's order: NULL args; struct_size; NULL reward / vf / uid / uid_next / advantages / value_targets / live;
 * num_steps < 1; num_envs < 1; num_slots outside 1 ... DCOMP_MAX_UE; 2^40 elements or more (all DCOMP_EINVAL but the size).  The call
 * only enqueues on `stream`, allocates nothing and does not synchronise. */
#ifndef DCOMP_GAE_UID_H
#define DCOMP_GAE_UID_H

#include "dcomp_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef DCOMP_EABI
#define DCOMP_EABI (-7)        /* as in dcomp.h: caller and library disagree about a struct size */
#endif

/* Every pointer is a DEVICE pointer. */
typedef struct dcomp_gae_uid_args {
    int32_t struct_size;          /* sizeof(dcomp_gae_uid_args) of the caller */
    int32_t num_steps;            /* T >= 1 */
    int32_t num_envs;             /* E >= 1 */
    int32_t num_slots;            /* U, 1 ... DCOMP_MAX_UE; T E U < 2^40 */
    int32_t max_shift;            /* largest departure count of any step; < 0: unknown, search the whole prefix */
    float gamma, lambda;
    const float *reward;          /* [T][E][U], in the layout of uid_next[t] */
    const float *vf;              /* [T][E][U] value predictions, in the layout of uid[t] */
    const uint16_t *uid;          /* [T][E][U] the words before step t */
    const uint16_t *uid_next;     /* [T][E][U] the words after step t (before a reset at the horizon) */
    const float *last_vf;         /* optional [E][U], in the layout of uid_next[T-1]: value of the observation after step T-1 (NULL = 0) */
    const uint8_t *end;           /* optional [T]: 1 = step t was the last of its episode; NULL = none */
    float *advantages;            /* [T][E][U] */
    float *value_targets;         /* [T][E][U] */
    uint8_t *live;                /* [T][E][U] 1 = the row counts */
} dcomp_gae_uid_args;

int dcomp_gae_uid(const dcomp_gae_uid_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif
