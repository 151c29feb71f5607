"""The shapes of the grouped learner tests (tests/test_learner_group_*.py, tests/test_learner_group_accum_*.py) as tables: the CPU
tests show what they reach (which cell a shape reaches is the library's answer, tests/fcnet_cases.py), the GPU tests run them.
Tables only; nothing here touches the device."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_HEADER = os.path.join(REPO, 'include', 'dcomp_learner_group.h')
CHUNK = 2048

# The grouped cases of the GPU tests: (U, B, hidden, activation, E, T, slot_policy, compact).  Each is the smallest shape that reaches
# its cell; every one trains with minibatches of 64 rows per policy.
GROUP_CASES = {
    'a-rows': (5, 3, 32, 'tanh', 70, 5, [0, 1, 1, 0, 1], False),         # the uneven split: 700 against 1 050 rows
    'a-compact': (5, 3, 32, 'tanh', 70, 5, [0, 1, 1, 0, 1], True),
    'b-compact': (3, 36, 64, 'relu', 33, 2, [0, 1, 2], True),            # 36 stations: two connection words, two staging chunks; <2, 1>
    'c-rows': (4, 10, 256, 'tanh', 40, 2, [0, 1, 2, 3], False),          # the widest instantiation; <2, 4>, bias<4>
    'h128-b5': (4, 5, 128, 'tanh', 40, 2, [0, 1, 0, 1], False),          # one input tile, four output tiles: <1, 4>
    'h128-b10': (4, 10, 128, 'relu', 40, 2, [0, 1, 0, 1], True),         # two input tiles: <2, 4>
    'h32-relu': (5, 3, 32, 'relu', 70, 2, [0, 1, 1, 0, 1], True),
    'h64-tanh': (5, 3, 64, 'tanh', 70, 2, [0, 1, 1, 0, 1], False),       # dW2 / dW3 through <2, 1>
    'h256-relu': (4, 10, 256, 'relu', 40, 2, [0, 1, 2, 3], True),
}
UNEVEN = ('a-rows', 'a-compact')


def group_slice():
    """DCOMP_GROUP_SLICE as the header has it."""
    return int(re.search(r'#define\s+DCOMP_GROUP_SLICE\s+(\d+)', open(GROUP_HEADER).read()).group(1))


# The shapes of the grouped accumulated GPU tests: (U, B, hidden, E, T, slot_policy).
CALL = (5, 3, 32, 70, 13, [0, 1, 2, 0, 1])            # GROUP_CASES['a-rows']'s shape with T raised: 4 550 source rows for indices of 4 500
CALL_ROWS = [4500, 2250, 0]                           # 3 and 2 weight-gradient chunks; the third member sits the calls out
FINISH = {32: (4, 5, 32, 40, 2, [0, 1, 2, 3]), 64: (4, 5, 64, 40, 2, [0, 1, 2, 3])}
UPDATE = (4, 5, 32, 100, 23, [0, 0, 1, 2])            # 4 600 / 2 300 / 2 300 rows per policy, max_rows 2 048
LOCK = (4, 5, 32, 32, 8, [0, 1, 0, 1])                # per rank: 32 envs, 512 rows per policy
LOCK4 = (4, 5, 32, 32, 8, [0, 1, 2, 3])
# (n_of per policy, minibatch_rows, max_rows, micro_rows, grad_clip) of every grouped update the GPU tests run
PLANS = {
    'whole-batch': ([4600, 2300, 2300], None, 2048, 2048, 0.5),
    'two-rounds': ([4600, 2300, 2300], 3000, 2048, 2048, 0.5),
    'no-clip': ([4600, 2300, 2300], 3000, 2048, 2048, None),
    'clip-only': ([4600, 2300, 2300], 3000, 4600, None, 0.5),
    'mix': ([4600, 2300, 2300], 2048, 2048, None, 1.0),
    'lock-1': ([512, 512], 256, 2048, None, 5.0),
    'lock-2': ([512, 512], 128, 2048, None, 5.0),
    'idle-policy': ([4600, 0, 2300], 3000, 2048, 2048, None),
    'plain': ([700, 1050], 64, 64, None, None),
}
