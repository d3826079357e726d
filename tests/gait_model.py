"""The gait stage restated in numpy (include/mpcq.h "gait transitions", mpcq_gait.hip): one call
of `roll` is one call of the kernel for every robot of a batch.  All quantities are small
integers in doubles or int32, so every comparison against the kernel is exact equality.

Where the issue's prose leaves a choice, this file decides, and the kernel follows:
  - `last` for index 0 is row 19 (the reference's gait[index - 1] wraps, as the planner's roll);
  - a NaN speed leaves `want` alone in every case, also while want < 0 (no band is assigned);
  - the terminator row of a library cycle is all zero, like the rows after it;
  - a table without a zero row is not written at all, and neither is its state row, not even
    the sanitised values or a selection.
"""
import math
from types import SimpleNamespace

import numpy as np

GAIT_MAX = 8
MANUAL, BY_SPEED = 0, 1
YAW_WEIGHT = 0.2421053541332781  # sqrt(0.19**2 + 0.15005**2), as the header's literal


def params(**kw):
    p = SimpleNamespace(n_gaits=0, select=MANUAL, align=1, reserved0=0, thresholds=[math.inf] * 7, hysteresis=0.0,
                        yaw_weight=YAW_WEIGHT, reserved=[0.0] * 5)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        if k == "thresholds":
            v = list(v) + [math.inf] * (7 - len(v))
        setattr(p, k, v)
    return p


def new_state(B):
    st = np.zeros((B, 4), np.int32)
    st[:, :2] = -1
    return st


def check_cycle(cy):
    """None, or (row, field) of the first broken library rule."""
    cy = np.asarray(cy, np.float64)
    rows = 0
    while rows < 20 and cy[rows, 0] != 0.0:
        c = cy[rows, 0]
        if not (1 <= c <= 64) or c != int(c):
            return rows, "count"
        for q in range(4):
            if cy[rows, 1 + q] not in (0.0, 1.0):
                return rows, "contact"
        rows += 1
    if rows < 1:
        return 0, "count"
    if rows > 19:
        return 19, "count"
    rest = cy[rows:].ravel().view(np.uint64)
    if rest.any():
        e = int(np.flatnonzero(rest)[0])
        return rows + e // 5, "contact" if e % 5 else "count"
    return None


def period(cy):
    return int(np.asarray(cy)[:, 0].sum())


def cycle_step(cy, phase):
    """(contacts of step `phase` of the cycle, whether it is the first step of its row)."""
    start = 0
    for r in range(20):
        c = int(cy[r, 0])
        if c == 0:
            break
        if phase < start + c:
            return cy[r, 1:].copy(), phase == start
        start += c
    raise IndexError(phase)


def select(p, want, v_ref):
    """Step 1 for one robot: the new `want`."""
    n = p.n_gaits
    s = math.sqrt(v_ref[0] * v_ref[0] + v_ref[1] * v_ref[1]) + p.yaw_weight * abs(v_ref[5])
    th, hy = p.thresholds, p.hysteresis
    if want < 0:
        if s == s:
            want = sum(1 for i in range(n - 1) if s >= th[i])
        return want
    up = False
    while want < n - 1 and s > th[want] + hy:
        want += 1
        up = True
    if not up:
        while want > 0 and s < th[want - 1] - hy:
            want -= 1
    return want


def roll_one(p, cycles, v_ref, gait, st):
    """One robot, in place: gait (20, 5) doubles, st (4,) int32.  Returns whether it wrote."""
    n = p.n_gaits
    want, active, phase, switches = (int(v) for v in st)
    if active < -1 or active >= n:
        active = -1
    if want < -1 or want >= n:
        want = -1
    if p.select == BY_SPEED:
        want = select(p, want, v_ref)
    zero = np.flatnonzero(gait[:, 0] == 0.0)
    if zero.size == 0:
        return False
    index = int(zero[0])
    last = (index + 19) % 20
    if active >= 0:
        phase %= period(cycles[active])
    if want >= 0 and want != active:
        if active >= 0:
            boundary = cycle_step(cycles[active], phase)[1]
        else:
            boundary = (not np.array_equal(gait[0, 1:], gait[last, 1:])) or index == 1
        if boundary or p.align == 0:
            active, phase = want, 0
            switches = (switches + 1 + 2 ** 31) % 2 ** 32 - 2 ** 31  # int32 wrap
    if active >= 0:
        new = cycle_step(cycles[active], phase)[0]
        phase = (phase + 1) % period(cycles[active])
    else:
        new = gait[0, 1:].copy()
    if np.array_equal(gait[last, 1:], new):
        gait[last, 0] += 1.0
    else:
        gait[index, 0] = 1.0
        gait[index, 1:] = new
    if gait[0, 0] > 1.0:
        gait[0, 0] -= 1.0
    else:
        gait[:-1] = gait[1:].copy()
        gait[19] = 0.0
    st[:] = (want, active, phase, switches)
    return True


def roll(p, cycles, v_ref, gait, state):
    """The batch, in place: gait (B, 20, 5), state (B, 4) int32, v_ref (B, 6) or None (MANUAL)."""
    cycles = np.asarray(cycles, np.float64)
    for b in range(gait.shape[0]):
        roll_one(p, cycles, None if v_ref is None else v_ref[b], gait[b], state[b])
    return gait, state
