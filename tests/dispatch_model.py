"""Host model of the dispatch-order layer (csrc/mpcq_order.hip, the session's order_kernel in
csrc/mpcq_session.hip, the suspension rule of the engine's ADMM loop), shared by
test_dispatch_model.py (CPU) and test_gpu_dispatch.py (GPU).

Integer-exact restatements in plain Python / numpy, written from the kernels' comments and
from MPC.py's construct_gait rule (MPC.py:646-650), not from the kernels' code: one element at
a time, no scans, no waves.  The kernels must reproduce them exactly; only the order inside a
bucket of the session's order is left open (documented as arbitrary).
"""
import math

import numpy as np

SLOTS = 251        # class table slots: the bitmap of contact masks modulo this prime
BUCKETS = 256      # cost / key buckets
ITER_SHIFT = 4     # a cost bucket is 16 iterations wide


# ------------------------------------------------------------------ gait class
def class_bitmap(fs) -> int:
    """The set of contact masks the phases of one fsteps table (20,13) use, as a 16-bit
    bitmap (bit m set: some phase has mask m).  construct_gait: the table ends at the first
    row whose duration is 0.0; foot q (bit q of the mask) is in contact unless its x
    (column 1 + 3 q) is NaN or == 0.0.  None: no terminating row (BAD_GAIT)."""
    key = 0
    for j in range(20):
        if fs[j, 0] == 0.0:
            return key
        mask = 0
        for q in range(4):
            x = fs[j, 1 + 3 * q]
            if not (math.isnan(x) or x == 0.0):
                mask |= 1 << q
        key |= 1 << mask
    return None


def class_slot(fs) -> int:
    key = class_bitmap(fs)
    return 0 if key is None else key % SLOTS


def class_slots(fsteps) -> np.ndarray:
    return np.array([class_slot(f) for f in np.asarray(fsteps, dtype=np.float64)], np.int32)


def class_costs(tab_sum, tab_cnt) -> list:
    """The cost bucket of every slot: (sum // cnt) >> 4, at most 255; a slot the table has
    not seen takes the mean over all seen slots (total sum // total count); 0 before any
    launch."""
    s = [int(v) for v in tab_sum]
    n = [int(v) for v in tab_cnt]
    tot_s = sum(a for a, c in zip(s, n) if c)
    tot_n = sum(c for c in n if c)
    unseen = tot_s // tot_n if tot_n else 0
    return [min((a // c if c else unseen) >> ITER_SHIFT, BUCKETS - 1) for a, c in zip(s, n)]


def stable_order(buckets) -> np.ndarray:
    """Stable counting sort: the highest bucket first, input order kept inside a bucket."""
    buckets = [int(b) for b in buckets]
    out = []
    for q in range(BUCKETS - 1, -1, -1):
        out.extend(i for i, b in enumerate(buckets) if b == q)
    assert len(out) == len(buckets)
    return np.array(out, np.int32)


def stable_order_fast(buckets) -> np.ndarray:
    """The same permutation for large batches (numpy's stable sort on the negated bucket);
    test_dispatch_model.py checks it against stable_order."""
    return np.argsort(-np.asarray(buckets, np.int64), kind="stable").astype(np.int32)


def class_order(cls, tab_sum, tab_cnt) -> np.ndarray:
    cost = class_costs(tab_sum, tab_cnt)
    return stable_order_fast([cost[c] for c in cls])


def class_learn(tab_sum, tab_cnt, cls, iters):
    """The table after a launch: every instance with iters > 0 adds its count to its slot."""
    s = [int(v) for v in tab_sum]
    n = [int(v) for v in tab_cnt]
    for c, it in zip(cls, iters):
        if it > 0:
            s[int(c)] += int(it)
            n[int(c)] += 1
    return np.array(s, np.uint64), np.array(n, np.uint64)


# ------------------------------------------------------------------ suspended list
def key_bucket(v: float) -> int:
    """floor(8 log2 v) + 128 in 0..255 (1/8 octave, keys from 2^-16 to 2^16); a key that is
    not > 0, or NaN: 0."""
    if not v > 0.0:
        return 0
    if math.isinf(v):
        return BUCKETS - 1
    e = math.floor(8.0 * math.log2(v)) + 128
    return max(0, min(BUCKETS - 1, e))


def key_edge_distance(v: float) -> float:
    """|8 log2 v - nearest integer| (inf for keys whose bucket no rounding can move)."""
    if not v > 0.0 or math.isinf(v):
        return math.inf
    e = 8.0 * math.log2(v)
    return abs(e - round(e))


def is_pow2(v: float) -> bool:
    return v > 0.0 and not math.isinf(v) and math.frexp(v)[0] == 0.5


def suspended_list(prev, n, status, key, code) -> np.ndarray:
    """Of prev[0..n) (None: 0..n-1) the instances whose status is ``code``, the largest key
    bucket first, prev's order inside a bucket."""
    ids = [int(i) for i in (range(n) if prev is None else prev[:n])]
    sus = [i for i in ids if status[i] == code]
    b = [key_bucket(float(key[i][0])) for i in sus]
    o = stable_order(b)
    return np.array([sus[j] for j in o], np.int32)


# ------------------------------------------------------------------ session order
def iters_bucket(it: int) -> int:
    """Buckets of 16 iterations, a negative count as 0, at most 255."""
    return min(max(int(it), 0) >> ITER_SHIFT, BUCKETS - 1)


# ------------------------------------------------------------------ slices
def suspend_bound(slice_iters: int, check: int = 25, adapt: int = 100, max_iter: int = 4000) -> int:
    """The largest final iteration count an instance of a sliced solve can have without
    having been suspended.

    The ADMM loop runs in segments that end where a termination check or an adaptive-rho step
    is due (iteration counts that are multiples of ``check`` or ``adapt``) or at max_iter.  A
    cold instance is suspended at the first segment end k >= slice_iters -- except that a
    segment end where rho is updated leaves the loop to refactorise before it looks at the
    slice, and the instance then runs on to the next segment end.  Rho updates happen only at
    multiples of ``adapt``, so the bound is the first segment end >= slice_iters that is not
    one: the slice plus the gap to the next segment end, plus one more segment when that end
    can update rho.  An instance that was not suspended stopped at or before it; one whose
    final count is larger was.  (A suspended instance has run >= slice_iters iterations, so no
    listed instance ends below the slice.)"""
    assert slice_iters >= 1
    for k in range(slice_iters, max_iter):
        may_update_rho = adapt > 0 and k % adapt == 0
        if check > 0 and k % check == 0 and not may_update_rho:
            return k
    return max_iter


# ------------------------------------------------------------------ shared test inputs
def table(rows, rest=None, swing=float("nan")):
    """An fsteps table (20,13) from rows of (duration, mask): foot q of a row is in contact
    (a non-zero foothold) where bit q of the mask is set, else ``swing``.  The rows after the
    listed ones have duration 0 (the first of them terminates the table) and, with ``rest``,
    that mask -- which no reader of the table may count."""
    fs = np.full((20, 13), np.nan)
    fs[:, 0] = 0.0
    for j in range(20):
        if j < len(rows):
            d, m = rows[j]
            fs[j, 0] = d
        elif rest is not None:
            m = rest
        else:
            continue
        for q in range(4):
            if m >> q & 1:
                fs[j, 1 + 3 * q:4 + 3 * q] = (0.19 - 0.05 * q, -0.15 + 0.02 * j, 0.0)
            else:
                fs[j, 1 + 3 * q:4 + 3 * q] = (swing, 0.3, 0.0)
    return fs


def slot_cases():
    """Hand-built tables for the class-slot test: a list of (name, fsteps (20,13), bitmap or
    None for a table without terminator), the bitmap worked out by hand here."""
    out = []
    for m in range(1, 16):  # every non-empty mask alone
        out.append((f"mask{m}", table([(16, m)]), 1 << m))
    # mixed combinations; the masks after the terminator differ and must not count
    out.append(("trot", table([(1, 15), (7, 9), (1, 15), (7, 6)], rest=5), 1 << 15 | 1 << 9 | 1 << 6))
    out.append(("1..7", table([(2, m) for m in range(1, 8)], rest=15), 0xfe))
    out.append(("8..15", table([(2, m) for m in range(8, 16)], rest=1), 0xff00))
    out.append(("all15", table([(1, m) for m in range(1, 16)] + [(1, 3)]), 0xfffe))
    out.append(("odd", table([(3, m) for m in (1, 3, 5, 7, 9, 11, 13, 15)]), 0xaaaa))
    out.append(("repeat", table([(1, 12), (1, 12), (5, 3), (1, 12)]), 1 << 12 | 1 << 3))
    # a foothold with x exactly 0.0 (and -0.0) counts as swing: mask 15 reads as 14 / 13
    fs = table([(16, 15)])
    fs[0, 1] = 0.0
    out.append(("x==0", fs, 1 << 14))
    fs = table([(8, 15), (8, 15)])
    fs[1, 4] = -0.0
    out.append(("x==-0", fs, 1 << 15 | 1 << 13))
    # NaN x with finite y, z: swing; a finite x with NaN y, z: contact
    fs = table([(16, 6)])
    fs[0, 2:4] = np.nan
    fs[0, 5:7] = np.nan
    out.append(("nan-yz", fs, 1 << 6))
    # swing feet written as 0.0 instead of NaN, and a flying phase (mask 0)
    out.append(("swing0", table([(4, 9), (4, 6)], swing=0.0), 1 << 9 | 1 << 6))
    out.append(("flying", table([(3, 15), (2, 0), (3, 15)]), 1 << 15 | 1 << 0))
    # the terminator at row 0 (an empty table: slot 0) and at row 19; a -0.0 terminator
    out.append(("term0", table([], rest=15), 0))
    out.append(("term19", table([(1, 1 + j % 4) for j in range(19)]), 1 << 1 | 1 << 2 | 1 << 3 | 1 << 4))
    fs = table([(4, 7), (4, 11)], rest=2)
    fs[2, 0] = -0.0
    out.append(("term-0", fs, 1 << 7 | 1 << 11))
    # no terminator: 20 phases (BAD_GAIT): slot 0 whatever the masks
    out.append(("noterm", table([(1, 1 + j % 15) for j in range(20)]), None))
    # a NaN duration is no terminator: the row counts, the table goes on
    fs = table([(4, 2), (4, 4), (4, 8)])
    fs[1, 0] = np.nan
    out.append(("nan-dur", fs, 1 << 2 | 1 << 4 | 1 << 8))
    # collisions modulo 251: {0} = 1 and {2..7} = 252; {1, 2} = 6 and {0, 8} = 257
    out.append(("coll-a1", table([(16, 0)]), 1))
    out.append(("coll-a2", table([(2, m) for m in range(2, 8)]), 252))
    out.append(("coll-b1", table([(8, 1), (8, 2)]), 6))
    out.append(("coll-b2", table([(8, 0), (8, 8)]), 257))
    return out


def suspended_keys(n: int, seed: int) -> np.ndarray:
    """Keys for the suspended-list test: the special values first (as far as n allows, in a
    seeded shuffle), then 2^((k + u) / 8) with u in [0.05, 0.95] -- no key but an exact power
    of two within 0.05 of a bucket edge in 8 log2 v, so a last-bit difference between the
    device's log2 and the host's cannot move a bucket (check_key_edges).  2^15.875, the lower
    edge of the last bucket, is no power of two: it is bracketed at 2^(15.875 -+ 1/64)."""
    rng = np.random.default_rng(seed)
    special = [0.0, -0.0, -3.5, float("nan"), float("inf"), -float("inf"), 1e30, 2.0 ** -17, 2.0 ** -16, 1.0,
               2.0 ** (15.875 - 1 / 64), 2.0 ** (15.875 + 1 / 64), 2.0 ** 16, 2.0 ** -16 * 1.01, 2.0 ** -17 * 1.9,
               1e-300, 5e-324, 1.7e308, 0.9, 1.1]
    k = rng.integers(-160, 160, n)   # beyond 2^-16 .. 2^16 on both sides
    u = rng.uniform(0.05, 0.95, n)
    key = 2.0 ** ((k + u) / 8.0)
    m = min(n, len(special))
    pos = rng.permutation(n)[:m]
    key[pos] = rng.permutation(special)[:m] if m < len(special) else special
    return key


def check_key_edges(keys, tol: float = 1e-9):
    """No key other than an exact power of two within ``tol`` of a bucket edge."""
    for v in keys:
        v = float(v)
        assert is_pow2(v) or key_edge_distance(v) > tol, v
