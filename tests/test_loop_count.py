"""CPU: the instruction budget of the N = 16 ADMM iteration (tools/loop_count.py).

The production kernel's innermost loop is compiled to gfx950 assembly with the Makefile's
flags and counted per class.  One ADMM iteration of one instance is its instruction count on
a single in-order wave, so the count is pinned: no scratch or global
access inside the loop, the FP64 arithmetic of round 6 (every operation follows the oracle's
order, so its count does not move), and no more instructions in all than the round-7 trim
left.  The compile takes about 20 s."""
import os
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

# round 6 (the parent of the trim): 635 instructions, 318 of them FP64 VALU -- 315 FP64
# operations, a clamp's v_max_f64 / v_min_f64 pair counted once (profiles/r07_loop_count_parent.txt)
FP64_OPS = 315
FP64_VALU = 318
# after the trim (profiles/r07_loop_count.txt): as compiled, and after asmpass/nop_elide.py
TOTAL_MAX = 614
TOTAL_ELIDED_MAX = 596


@pytest.fixture(scope="module")
def loop16():
    import loop_count
    return loop_count.measure(16)


def test_loop_has_no_scratch_or_global_access(loop16):
    assert loop16["scratch_global"] == 0, loop16


def test_fp64_count_is_round_6s(loop16):
    assert loop16["fp64_ops"] == FP64_OPS, loop16
    assert loop16["fp64_valu"] == FP64_VALU, loop16


def test_total_is_not_above_the_recorded_figure(loop16):
    print(loop16)
    assert loop16["total"] <= TOTAL_MAX, loop16
    assert loop16["after_nop_elide"] <= TOTAL_ELIDED_MAX, loop16
