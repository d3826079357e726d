"""Host model of the scenario stage (include/mpcq.h, "scenarios"): an independent scalar
restatement, Python integers and floats, one robot at a time.  It shares no code with
mpcq/scenario.py (the vectorised numpy statement the package ships) nor with the kernel; the
tests hold all three to each other bit for bit.

Python's float is the IEEE double, its int / int division is correctly rounded, and nothing here
contracts a multiply and an add: the kernel's operations one by one."""
from types import SimpleNamespace

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
STREAM_CONSTANTS, STREAM_COMMANDS, STREAM_PUSHES = 0, 1, 2
ROBOT_DTYPE = np.dtype([("mass", np.float64), ("gI", np.float64, (3, 3)), ("mu", np.float64),
                        ("fz_max", np.float64), ("reserved", np.float64, (4,))])


def params(**kw):
    """mpcq_default_scenario_params with overrides, as a plain namespace."""
    p = SimpleNamespace(seed=0, v_lo=[1.0, 0.0, 0.0], v_hi=[1.0, 0.0, 0.0], wrench_lo=[0.0] * 6, wrench_hi=[0.0] * 6,
                        push_prob=1.0, mass_scale_lo=1.0, mass_scale_hi=1.0, mu_lo=0.9, mu_hi=0.9, commands=1,
                        cmd_start=48, cmd_ramp=175, cmd_period=0, pushes=0, push_first=0, push_period=0,
                        push_jitter=0, push_ticks=10, push_flip=0, robots=0, reserved=[0] * 5)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, list(v) if isinstance(getattr(p, k), list) else v)
    return p


def philox(counter, key):
    """Philox4x32-10: counter 4 words, key 2 words -> 4 words."""
    c0, c1, c2, c3 = (int(x) & MASK for x in counter)
    k0, k1 = (int(x) & MASK for x in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def draw(p, b, epoch, index, stream):
    seed = int(p.seed)
    return philox((b, epoch, index, stream), (seed & MASK, seed >> 32))


def u(wa, wb):
    return (float(wa >> 5) * 67108864.0 + float(wb >> 6)) * 2.0 ** -53


def rng(lo, hi, x):
    d = float(hi) - float(lo)
    m = d * x
    return float(lo) + m


def draw_int(a, n, w):
    return a + ((w * n) >> 32)


def prob(w, pr):
    return float(w) * 2.0 ** -32 < pr


def constants(p, b, epoch):
    w = draw(p, b, epoch, 0, STREAM_CONSTANTS)
    return rng(p.mass_scale_lo, p.mass_scale_hi, u(w[0], w[1])), rng(p.mu_lo, p.mu_hi, u(w[2], w[3]))


def target(p, b, epoch, j):
    a = draw(p, b, epoch, 2 * j, STREAM_COMMANDS)
    c = draw(p, b, epoch, 2 * j + 1, STREAM_COMMANDS)
    return [rng(p.v_lo[0], p.v_hi[0], u(a[0], a[1])), rng(p.v_lo[1], p.v_hi[1], u(a[2], a[3])),
            rng(p.v_lo[2], p.v_hi[2], u(c[0], c[1]))]


def alpha(p, tau):
    """(segment j, the segment's tick t, alpha) of the episode's tick tau."""
    j = tau // p.cmd_period if p.cmd_period > 0 else 0
    t = tau - j * p.cmd_period - (p.cmd_start if j == 0 else 0)
    if p.cmd_ramp > 0:
        a = t / p.cmd_ramp
        a = 0.0 if a < 0.0 else 1.0 if a > 1.0 else a
    else:
        a = 1.0 if t >= 0 else 0.0
    return j, t, a


def command(p, b, epoch, tau):
    if not p.commands:
        return [0.0] * 6
    j, _, a = alpha(p, tau)
    tg = target(p, b, epoch, j)
    pv = target(p, b, epoch, j - 1) if j > 0 else [0.0, 0.0, 0.0]
    v = []
    for e in range(3):
        if a == 1.0:
            v.append(tg[e])
        elif a == 0.0:
            v.append(pv[e])
        else:
            d = tg[e] - pv[e]
            m = d * a
            v.append(pv[e] + m)
    return [v[0], v[1], 0.0, 0.0, 0.0, v[2]]


def window(p, b, epoch, tau):
    """The push window tau falls into, or None before push_first: dict(j, jitter, occurs, s,
    bits, active)."""
    if not p.pushes or tau < p.push_first:
        return None
    j = (tau - p.push_first) // p.push_period if p.push_period > 0 else 0
    h = draw(p, b, epoch, 4 * j, STREAM_PUSHES)
    jitter = draw_int(0, p.push_jitter + 1, h[0])
    occurs = prob(h[1], p.push_prob)
    s = p.push_first + j * p.push_period + jitter
    return dict(j=j, jitter=jitter, occurs=occurs, s=s, bits=h[2] & p.push_flip,
                active=occurs and s <= tau < s + p.push_ticks)


def push(p, b, epoch, tau):
    """(the push [6], active)."""
    w = window(p, b, epoch, tau)
    if w is None or not w["active"]:
        return [0.0] * 6, False
    out = []
    for i in range(6):
        d = draw(p, b, epoch, 4 * w["j"] + 1 + i // 2, STREAM_PUSHES)
        x = rng(p.wrench_lo[i], p.wrench_hi[i], u(d[0], d[1]) if i % 2 == 0 else u(d[2], d[3]))
        out.append(-x if (w["bits"] >> i) & 1 else x)
    return out, True


def new_state(B):
    return dict(epoch=np.zeros(B, np.int32), tick=np.zeros(B, np.int32), robots=np.zeros(B, ROBOT_DTYPE),
                draw=np.zeros((B, 8)))


def robot_row(p, base_row, ms, mu):
    """The row of CV_ROBOTS: base_row (a ROBOT_DTYPE scalar) under the bits of p.robots."""
    r = np.zeros((), ROBOT_DTYPE)
    r["mass"] = float(base_row["mass"]) * ms if p.robots & 1 else float(base_row["mass"])
    g = np.array(base_row["gI"], np.float64).reshape(9)
    r["gI"] = np.array([float(x) * ms if p.robots & 1 else float(x) for x in g]).reshape(3, 3)
    r["mu"] = mu if p.robots & 2 else float(base_row["mu"])
    r["fz_max"] = float(base_row["fz_max"])
    r["reserved"] = base_row["reserved"]
    return r


def step(p, st, first, all_first, base, wrench_in=None, init=False):
    """One call of the kernel over every robot of the state ``st`` (new_state), updated in
    place: first (B,) or None, base (B,) ROBOT_DTYPE, wrench_in (B, 6) or None.  init: the
    launch of mpcq_session_enable_scenario (the stored epoch's constants, tau not advanced).
    Returns v_ref, push, wrench_out (B, 6) and the robot-ticks' (epoch, tau, is_first)."""
    B = st["epoch"].shape[0]
    v_ref, pu, wo = np.zeros((B, 6)), np.zeros((B, 6)), np.zeros((B, 6))
    seen = []
    for b in range(B):
        is_first = bool(init or all_first or (first is not None and first[b] != 0))
        epoch, tau = int(st["epoch"][b]), int(st["tick"][b])
        if is_first and not init:
            epoch, tau = epoch + 1, 0
        if is_first:
            ms, mu = constants(p, b, epoch)
            st["robots"][b] = robot_row(p, base[b], ms, mu)
            st["draw"][b] = [ms, mu, float(epoch), 0.0, 0.0, 0.0, 0.0, 0.0]
        v_ref[b] = command(p, b, epoch, tau)
        w, active = push(p, b, epoch, tau)
        pu[b] = w
        for e in range(6):
            wi = 0.0 if wrench_in is None else float(wrench_in[b, e])
            wo[b, e] = wi + w[e] if active else wi
        st["epoch"][b] = epoch
        if not init:
            st["tick"][b] = tau + 1
        seen.append((epoch, tau, is_first))
    return v_ref, pu, wo, seen
