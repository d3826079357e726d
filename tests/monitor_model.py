"""Host model of the episode monitor (csrc/mpcq_monitor.hip): the same float64 operations in
the same order, no contraction (numpy has none), so every output is bit-equal to the kernel's.

step(...) is one tick for a batch; the accumulators live in a dict as mpcq.monitor.new_state
lays them out (ep (B, 8), ep_ticks (B,), episodes (B,), last (B, 16), totals (8,) uint64) and are
updated in place."""
import numpy as np

NONFINITE, TILT, HEIGHT, SOLVER, TIMEOUT = 1, 2, 4, 8, 16
BITS = (NONFINITE, TILT, HEIGHT, SOLVER, TIMEOUT)
OK_STATUS = (1, 2, -2)  # SOLVED, SOLVED_INACCURATE, MAX_ITER_REACHED: the retrieve's test
TRACE = 16
DEFAULTS = dict(max_tilt=0.5, min_height=0.10, max_ticks=0)


def new_state(B):
    ep = np.zeros((B, 8))
    ep[:, 4] = np.inf
    return dict(ep=ep, ep_ticks=np.zeros(B, np.int32), episodes=np.zeros(B, np.int32),
                last=np.zeros((B, 16)), totals=np.zeros(8, np.uint64))


def copy_state(acc):
    return {k: v.copy() for k, v in acc.items()}


def done_bits(q_w, status, ticks, max_tilt, min_height, max_ticks):
    """The done bits of one tick; ticks = the episode's tick count with this tick in."""
    q_w = np.asarray(q_w, np.float64)
    done = np.zeros(q_w.shape[0], np.int32)
    with np.errstate(invalid="ignore"):
        done |= np.where(~np.isfinite(q_w).all(axis=1), NONFINITE, 0).astype(np.int32)
        ar, ap = np.abs(q_w[:, 3]), np.abs(q_w[:, 4])
        done |= np.where((ar > max_tilt) | (ap > max_tilt), TILT, 0).astype(np.int32)  # false on NaN
        done |= np.where(q_w[:, 2] < min_height, HEIGHT, 0).astype(np.int32)
    done |= np.where(~np.isin(status, OK_STATUS), SOLVER, 0).astype(np.int32)
    if max_ticks > 0:
        done |= np.where(ticks >= max_ticks, TIMEOUT, 0).astype(np.int32)
    return done


def step(q_w, status, iters, f0, cost, state, v_ref, acc, max_tilt=0.5, min_height=0.10, max_ticks=0):
    """One tick.  Returns (done (B,) int32, trace (B, 16)); acc is updated in place."""
    q_w = np.asarray(q_w, np.float64)
    B = q_w.shape[0]
    status = np.asarray(status, np.int32)
    iters = np.asarray(iters, np.int32)
    f0 = np.asarray(f0, np.float64)
    cost = np.asarray(cost, np.float64)
    state = np.asarray(state, np.float64)
    v_ref = np.broadcast_to(np.asarray(v_ref, np.float64), (B, 6))
    ep = acc["ep"].copy()
    ticks = acc["ep_ticks"] + np.int32(1)
    done = done_bits(q_w, status, ticks, max_tilt, min_height, max_ticks)
    with np.errstate(invalid="ignore", over="ignore"):
        c = cost[:, 0].copy()
        for e in range(1, 13):  # left to right
            c = c + cost[:, e]
        ff = f0[:, 0] * f0[:, 0]
        for e in range(1, 12):
            ff = ff + f0[:, e] * f0[:, e]
        d0 = state[:, 6] - v_ref[:, 0]
        d1 = state[:, 7] - v_ref[:, 1]
        d2 = state[:, 11] - v_ref[:, 5]
        verr = (d0 * d0 + d1 * d1) + d2 * d2
        ok = (done & SOLVER) == 0
        ep[:, 0] = np.where(ok, ep[:, 0] + c, ep[:, 0])
        ep[:, 1] = np.where(ok, ep[:, 1] + ff, ep[:, 1])
        ep[:, 5] = np.where(ok, ep[:, 5] + verr, ep[:, 5])
        ep[:, 2] = ep[:, 2] + iters.astype(np.float64)
        fin = (done & NONFINITE) == 0
        ar, ap = np.abs(q_w[:, 3]), np.abs(q_w[:, 4])
        t = np.where(ar > ap, ar, ap)
        ep[:, 3] = np.where(fin & (t > ep[:, 3]), t, ep[:, 3])
        ep[:, 4] = np.where(fin & (q_w[:, 2] < ep[:, 4]), q_w[:, 2], ep[:, 4])
    ep[:, 6] = 0.0
    ep[:, 7] = 0.0
    trace = np.zeros((B, TRACE))
    trace[:, 0:6] = q_w
    trace[:, 6] = done
    trace[:, 7] = status
    trace[:, 8] = iters
    trace[:, 9] = ticks
    trace[:, 10] = c
    trace[:, 11] = ff
    d = done != 0
    row = np.concatenate([ep, ticks[:, None].astype(np.float64), done[:, None].astype(np.float64), q_w], axis=1)
    acc["last"][d] = row[d]
    acc["episodes"][d] += 1
    ep[d] = 0.0
    ep[d, 4] = np.inf
    acc["ep"][:] = ep
    acc["ep_ticks"][:] = np.where(d, 0, ticks)
    tot = acc["totals"]
    tot[0] += np.uint64(B)
    tot[1] += np.uint64(int(d.sum()))
    for i, bit in enumerate(BITS):
        tot[2 + i] += np.uint64(int(((done & bit) != 0).sum()))
    return done, trace


def reset(acc, mask):
    """An explicit mpcq_session_reset: the masked robots' running episode is discarded."""
    m = np.asarray(mask) != 0
    acc["ep"][m] = 0.0
    acc["ep"][m, 4] = np.inf
    acc["ep_ticks"][m] = 0


def same(a, b):
    """Bit equality of two arrays, any NaN equal to any NaN (and so -0.0 != 0.0)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.int64)[~na], np.ascontiguousarray(b).view(np.int64)[~na]))
