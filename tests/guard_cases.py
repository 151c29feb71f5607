"""The kernel families tests/test_guard_bands_gpu.py runs behind guard bands (round 17), as a table in the shape of
test_threshold_gpu.FAMILIES, plus what each row claims about itself -- checked without a GPU by tests/test_guard_cpu.py.

Every E is chosen so that the last wavefront or workgroup is partly filled (E x lanes per env is no multiple of 64, or E is no multiple
of the envs a workgroup holds) and, where the shape allows it, so that E x U x row floats is no multiple of four: the end of the
observation then falls inside a 16-byte line.  No family needs more than 7 envs; T is 4 steps (the fused rollout of the short-row shapes
needs at least 4), 5 where UEs arrive and depart so that a slot dies after having been live (ARRIVAL: time 3).
"""
from collections import namedtuple

from tests import threshold_cases as tc
from tests.threshold_cases import ARRIVAL

PHASES = (0, 4, 8, 12)          # bytes into a 16-byte line at which a float / int32 output starts

# sharing: 'mixed' (the reference's cycle; no max-cap station: the tight and wide kernels take no other) or 'maxcap' (a cycle with max-cap
# stations: conn_since exists and is written).  mode: 'step' | 'dyn' | 'rollout' (rollout() must be ONE launch) | 'rollout_steps' (must not).
# lanes: lanes an env occupies; epb: envs per workgroup (256-lane workgroups on the specialised kernels, 64 // U envs per wavefront when packed
# tightly; max(64, lanes) lanes on the generic one).
Case = namedtuple('Case', 'name kind U B E env mode tag sharing lanes epb')

CASES = [
    Case('narrow_32x10', 'multi', 32, 10, 3, {}, 'step', 'step_kernel<10, 32', 'mixed', 32, 8),            # StageGeo<10>::NPASS = 2
    Case('narrow_16x32', 'central', 16, 32, 5, {}, 'step', 'step_kernel<32, 16', 'maxcap', 16, 16),        # five staging windows per wave
    Case('narrow_10x5', 'central', 10, 5, 5, {}, 'step', 'step_kernel<5, 16', 'mixed', 16, 16),            # the one-window form
    Case('tight_10x5', 'multi', 10, 5, 7, {'DCOMP_TIGHT': '1'}, 'step', 'step_kernel_tight<5', 'mixed', 10, 24),
    Case('tight_5x32', 'central', 5, 32, 7, {'DCOMP_TIGHT': '1'}, 'step', 'step_kernel_tight<32', 'mixed', 5, 48),
    Case('wide_128x32', 'multi', 128, 32, 3, {}, 'step', 'step_kernel_wide<32', 'mixed', 128, 2),
    Case('wide_128x32_pad24000', 'multi', 128, 32, 3, {'DCOMP_WIDE_PAD_LDS': '24000'}, 'step', 'step_kernel_wide<32', 'mixed', 128, 2),
    Case('dyn_6x24', 'multi', 6, 24, 5, {}, 'dyn', 'step_kernel_dyn', 'maxcap', 8, 32),
    Case('big_32x40', 'multi', 32, 40, 3, {}, 'step', 'big_kernel', 'maxcap', 32, 2),
    Case('big_16x64', 'central', 16, 64, 5, {}, 'step', 'big_kernel', 'mixed', 16, 4),
    Case('big_forced_32x10', 'multi', 32, 10, 3, {'DCOMP_FORCE_BIG': '1'}, 'step', 'big_kernel', 'mixed', 32, 2),
    Case('big_row_x4_0_10x40', 'multi', 10, 40, 5, {'DCOMP_BIG_ROW_X4': '0'}, 'step', 'big_kernel', 'mixed', 16, 4),
    Case('big_row_x4_1_10x40', 'multi', 10, 40, 5, {'DCOMP_BIG_ROW_X4': '1'}, 'step', 'big_kernel', 'mixed', 16, 4),
    Case('big_dyn_6x40', 'multi', 6, 40, 5, {}, 'dyn', 'big_kernel', 'maxcap', 8, 8),
    Case('rollout_10x5', 'central', 10, 5, 5, {}, 'rollout', None, 'mixed', 16, 16),
    Case('rollout_32x10', 'multi', 32, 10, 3, {}, 'rollout', None, 'maxcap', 32, 8),
    Case('rollout_tight_10x5', 'central', 10, 5, 7, {'DCOMP_TIGHT': '1'}, 'rollout', 'step_kernel_tight<5', 'mixed', 10, 24),
    Case('big_rollout_12x40', 'multi', 12, 40, 3, {}, 'rollout', 'big_kernel', 'maxcap', 16, 4),
    Case('big_rollout_forced_10x5', 'central', 10, 5, 3, {'DCOMP_FORCE_BIG': '1'}, 'rollout', 'big_kernel', 'mixed', 16, 4),
    Case('big_rollout_steps_12x40', 'multi', 12, 40, 3, {'DCOMP_NO_FUSED_BIG': '1'}, 'rollout_steps', 'big_kernel', 'mixed', 16, 4),
]
IDS = [c.name for c in CASES]

# Units of a buffer that a call is documented (include/dcomp_types.h) not to write: (case name | '*', surface, buffer) -> (unit indices, reason).
# There is none.  obs, obs_compact and reward can have none.
ALLOW = {}


def slots(case):
    """UE slots per env: the list, or max_ues of the arrival schedule."""
    return tc.slots(case.U, case.mode)


def steps(case):
    return 5 if case.mode == 'dyn' else 4


def obs_floats(case):
    """Floats of one env's observation."""
    M = slots(case)
    return M * (4 * case.B + 1) if case.kind == 'multi' else M * (2 * case.B + 1)


def compact_words(case):
    """int32 words of one env's compact record (multi-agent only): U (B + 2) + 2B, one more word per UE above 32 stations."""
    M = slots(case)
    return M * (case.B + (3 if case.B > 32 else 2)) + 2 * case.B


def partly_filled(case):
    """The last wavefront or workgroup of the launch is partly filled."""
    return (case.E * case.lanes) % 64 != 0 or case.E % case.epb != 0


def shape_allows_ragged_end(case):
    """Some E <= 7 makes E x (floats per env) no multiple of four."""
    return obs_floats(case) % 4 != 0


def ragged_end(case):
    return (case.E * obs_floats(case)) % 4 != 0


def sharing_list(case):
    if case.sharing == 'mixed':
        return None
    cycle = ('resource-fair', 'max-cap', 'rate-fair', 'max-cap', 'proportional-fair')
    return [cycle[b % len(cycle)] for b in range(case.B)]


__all__ = ['ARRIVAL', 'PHASES', 'CASES', 'IDS', 'ALLOW', 'Case']
