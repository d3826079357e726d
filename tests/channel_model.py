"""Host model of the channel's two stages (include/mpcq.h, "channel"): a numpy restatement,
stateful over ticks, vectorised over robots, in the kernels' operation order.  It has its own
Philox and its own draw shapes: it shares no code with mpcq/channel.py (the statement of the draws
the package ships) nor with the kernels; the tests hold all three to each other bit for bit.

numpy's float64 operations are the IEEE double's, one rounding each, and nothing here contracts a
multiply and an add.  Rows move by assignment, so -0.0 and NaN travel as bits."""
from types import SimpleNamespace

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK, S32 = np.uint64(0xFFFFFFFF), np.uint64(32)
S_NOISE, S_HOLD, S_FORCE, S_BIAS, S_GAIN = 0x100, 0x110, 0x120, 0x200, 0x210
MAX_DELAY, MAX_LATENCY = 8, 4
F_INIT = np.array([0.0, 0.0, 8.0] * 4)
SQRT3 = 1.7320508075688772
FIELDS = ("seed", "delay", "latency", "hold_prob", "sigma", "bias", "f_sigma", "f_gain", "reserved")


def params(src=None, **kw):
    """mpcq_default_channel_params (all zero) with overrides, as a plain namespace; ``src``: an
    object with the struct's fields (a ctypes ChannelParams) to start from."""
    p = SimpleNamespace(seed=0, delay=0, latency=0, hold_prob=0.0, sigma=[0.0] * 12, bias=[0.0] * 12,
                        f_sigma=[0.0] * 3, f_gain=0.0, reserved=[0] * 2)
    if src is not None:
        for k in FIELDS:
            v = getattr(src, k)
            setattr(p, k, list(v) if hasattr(v, "__len__") else v)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        cur = getattr(p, k)
        if isinstance(cur, list):
            v = [float(v)] * len(cur) if not hasattr(v, "__len__") else [float(x) for x in v]
            assert len(v) == len(cur), k
        setattr(p, k, v)
    return p


def _words(x):
    return (np.asarray(x).astype(np.int64) & np.int64(0xFFFFFFFF)).astype(np.uint64)


def philox(p, b, epoch, c2, stream):
    """Philox4x32-10 of the counter (b, epoch, c2, stream) under the channel's seed: four uint64
    arrays of 32-bit words (the inputs broadcast)."""
    seed = int(p.seed)
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_words(x) for x in (b, epoch, c2, stream, seed & 0xFFFFFFFF, seed >> 32)))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def n(w):
    """The centred sum of the four words at unit variance."""
    s = (w[0] + w[1] + w[2] + w[3]).astype(np.int64) - np.int64(8589934590)
    return s.astype(np.float64) * np.float64(SQRT3 * 2.0 ** -32)


def u(wa, wb):
    return ((wa >> np.uint64(5)).astype(np.float64) * 67108864.0 + (wb >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53


def sym(w):
    return 2.0 * u(w[0], w[1]) - 1.0


def new_state(B):
    """The six arrays as the first enable leaves them: zero, every robot waiting to be primed."""
    st = dict(clock=np.zeros((B, 2), np.int32), obs=np.zeros((B, 12)), f_cmd=np.zeros((B, 12)),
              draw=np.zeros((B, 16)), s_ring=np.zeros((B, MAX_DELAY, 12)), f_ring=np.zeros((B, MAX_LATENCY, 12)))
    st["clock"][:, 1] = -1
    return st


def arm(st, mask=None):
    """mpcq_session_enable_channel's launch: every non-negative stored tau to its complement."""
    t = st["clock"][:, 1]
    sel = t >= 0 if mask is None else (t >= 0) & (np.asarray(mask) != 0)
    t[sel] = ~t[sel]


def observe(p, st, truth, first=None, all_first=False):
    """The observe stage of one tick on the state ``st`` (in place); returns obs (B, 12)."""
    truth = np.asarray(truth, np.float64)
    B = truth.shape[0]
    b = np.arange(B)
    first = np.full(B, bool(all_first)) | (np.zeros(B, bool) if first is None else np.asarray(first) != 0)
    epoch, stored = st["clock"][:, 0].copy(), st["clock"][:, 1].copy()
    init = first | (stored < 0)
    tau = np.where(stored < 0, ~stored, stored)
    epoch = np.where(first, epoch + 1, epoch).astype(np.int32)
    tau = np.where(first, 0, tau).astype(np.int32)
    if init.any():
        i12, q4 = np.arange(12), np.arange(4)
        bias = np.array(p.bias, np.float64) * sym(philox(p, b[:, None], epoch[:, None], 0, S_BIAS + i12))
        gain = 1.0 + np.float64(p.f_gain) * sym(philox(p, b[:, None], epoch[:, None], 0, S_GAIN + q4))
        gain[:, 0] = np.where(first, gain[:, 0], -gain[:, 0])  # not first: the force ring is pending
        st["draw"][init, :12] = bias[init]
        st["draw"][init, 12:] = gain[init]
        st["s_ring"][init] = truth[init][:, None, :]
        st["f_ring"][first] = F_INIT
    delayed = truth.copy()
    if p.delay > 0:
        rows = np.nonzero(~init)[0]
        slot = tau[rows] % p.delay
        delayed[rows] = st["s_ring"][rows, slot]
        st["s_ring"][rows, slot] = truth[rows]
    o = delayed.copy()
    for i in range(12):
        if p.bias[i] != 0.0:
            o[:, i] = o[:, i] + st["draw"][:, i]
        if p.sigma[i] != 0.0:
            o[:, i] = o[:, i] + np.float64(p.sigma[i]) * n(philox(p, b, epoch, tau, S_NOISE + i))
    if p.hold_prob > 0.0:
        w1 = philox(p, b, epoch, tau, S_HOLD)[1]
        hold = ~init & (w1.astype(np.float64) * 2.0 ** -32 < np.float64(p.hold_prob))
        o[hold] = st["obs"][hold]
    st["obs"][:] = o
    st["clock"][:, 0] = epoch
    st["clock"][:, 1] = tau + 1
    return o.copy()


def actuate(p, st, f0):
    """The actuate stage of the same tick (after observe); returns f_cmd (B, 12)."""
    f0 = np.asarray(f0, np.float64)
    B = f0.shape[0]
    b = np.arange(B)
    epoch, stored = st["clock"][:, 0], st["clock"][:, 1]
    tau = np.where(stored > 0, stored - 1, 0)
    g0 = st["draw"][:, 12].copy()
    pending = g0 < 0.0
    gain = st["draw"][:, 12:].copy()
    gain[:, 0] = np.where(pending, -g0, g0)
    cmd = f0.copy()
    st["f_ring"][pending] = f0[pending][:, None, :]
    st["draw"][pending, 12] = -g0[pending]
    if p.latency > 0:
        rows = np.nonzero(~pending)[0]
        slot = tau[rows] % p.latency
        cmd[rows] = st["f_ring"][rows, slot]
        st["f_ring"][rows, slot] = f0[rows]
    v = cmd.copy()
    if p.f_gain != 0.0:
        v = cmd * np.repeat(gain, 3, axis=1)
    for j in range(12):
        if p.f_sigma[j % 3] != 0.0:
            v[:, j] = v[:, j] + np.float64(p.f_sigma[j % 3]) * n(philox(p, b, epoch, tau, S_FORCE + j))
    st["f_cmd"][:] = v
    return v.copy()


def bits(a):
    """An array's bit patterns, for equality that tells -0.0 from 0.0 and takes NaN as a value."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a
