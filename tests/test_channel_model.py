"""CPU: the channel's draws and the host model of its two stages (tests/channel_model.py) --
the draw shapes' bounds and moments, the model against the package's statement of the draws
(mpcq/channel.py), and the behaviour the header states: pass-through, delay, latency, holds,
restarts, priming, and that every field acts."""
import numpy as np
import pytest

import channel_model as CM

SEEDS = (1, 0x123456789ABCDEF)
LIM = 2.0 * np.sqrt(3.0)


def _ctypes(p):
    import mpcq
    return mpcq.default_channel_params(**{k: getattr(p, k) for k in CM.FIELDS})


def _same(a, b):
    return np.array_equal(CM.bits(a), CM.bits(b))


# ---------------------------------------------------------------------- draws
@pytest.mark.parametrize("seed", SEEDS)
def test_normal_draw_bounds_and_moments(seed):
    """Conditions on the generator, from the precision of the format and the sample size: with
    49,152 unit-variance draws the mean's standard error is 0.0045 and the variance's 0.0060
    (Irwin-Hall of order 4: excess kurtosis -0.3), so +-0.02 and 1 +- 0.03 are more than 4
    standard errors.  Observed: means -0.010 .. -0.003, variances 0.990 .. 1.005, max |n| 3.27."""
    import mpcq
    p = mpcq.default_channel_params(seed=seed)
    # robots 0..4095 x 12 components at (epoch 0, tau 0); robot 3, epoch 2, component 0, tau 0..49151
    a = mpcq.channel.normal(p, np.arange(4096)[:, None], 0, 0, mpcq.channel.STREAM_NOISE + np.arange(12))
    b = mpcq.channel.normal(p, 3, 2, np.arange(49152), mpcq.channel.STREAM_NOISE)
    for x in (a, b):
        assert x.size == 49152 and x.dtype == np.float64
        assert np.abs(x).max() <= LIM
        assert abs(x.mean()) <= 0.02, x.mean()
        assert abs(x.var() - 1.0) <= 0.03, x.var()
    # the model's own generator and shapes give the same bits
    m = CM.params(seed=seed)
    assert _same(a, CM.n(CM.philox(m, np.arange(4096)[:, None], 0, 0, CM.S_NOISE + np.arange(12))))
    assert _same(b, CM.n(CM.philox(m, 3, 2, np.arange(49152), CM.S_NOISE)))


def test_normal_draw_extremes():
    """The shape itself: all-zero words give -2 sqrt(3) (1 - 2^-32), all-ones words the opposite."""
    z = tuple(np.array([v], np.uint64) for v in (0, 0, 0, 0))
    o = tuple(np.array([0xFFFFFFFF], np.uint64) for _ in range(4))
    assert CM.n(z)[0] == -CM.n(o)[0] and abs(CM.n(z)[0]) <= LIM and abs(CM.n(z)[0]) > LIM * (1 - 1e-9)
    assert CM.sym(z)[0] == -1.0 and -1.0 <= CM.sym(o)[0] < 1.0


@pytest.mark.parametrize("seed", SEEDS)
def test_episode_draws_against_the_package(seed):
    import mpcq
    amp = [0.0, 0.5, 1.0, 2.0] * 3
    p = mpcq.default_channel_params(seed=seed, bias=amp, f_gain=0.25, hold_prob=0.3)
    m = CM.params(p)
    r, e = np.arange(300)[:, None], np.arange(4)[None, :]
    bias, gain = mpcq.channel.bias(p, r, e), mpcq.channel.gain(p, r, e)
    assert bias.shape == (300, 4, 12) and gain.shape == (300, 4, 4)
    s = CM.sym(CM.philox(m, r[..., None], e[..., None], 0, CM.S_BIAS + np.arange(12)))
    assert (s >= -1.0).all() and (s < 1.0).all()
    assert _same(bias, np.array(amp) * s)
    assert _same(gain, 1.0 + 0.25 * CM.sym(CM.philox(m, r[..., None], e[..., None], 0, CM.S_GAIN + np.arange(4))))
    assert (gain > 0.75 - 1e-15).all() and (gain < 1.25).all() and gain.std() > 0.1
    assert (np.abs(bias) <= np.array(amp)).all() and (bias[..., 0] == 0.0).all()
    h = mpcq.channel.held(p, r, 1, np.arange(50)[None, :])
    w1 = CM.philox(m, r, 1, np.arange(50)[None, :], CM.S_HOLD)[1]
    assert np.array_equal(h, w1.astype(np.float64) * 2.0 ** -32 < 0.3)
    assert 0.27 < h.mean() < 0.33  # 15,000 decisions at 0.3: +-8 standard errors


# ---------------------------------------------------------------------- the model's behaviour
def _truths(B, T, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T, B, 12)), rng.standard_normal((T, B, 12)) * 10.0


def _run(p, truths, forces, st=None, first=None):
    """T ticks of both stages; first: {tick: mask}.  Tick 0 is a first tick for every robot."""
    st = CM.new_state(truths.shape[1]) if st is None else st
    obs, cmd = [], []
    for t in range(truths.shape[0]):
        obs.append(CM.observe(p, st, truths[t], first=(first or {}).get(t), all_first=t == 0))
        cmd.append(CM.actuate(p, st, forces[t]))
    return np.array(obs), np.array(cmd), st


def test_zero_channel_is_a_bitwise_pass_through():
    tr, f0 = _truths(5, 4)
    tr[1, 2, :] = -0.0
    tr[2, 3, 4:9] = np.nan
    f0[1, 0, :] = -0.0
    f0[3, 4, 2] = np.nan
    obs, cmd, st = _run(CM.params(seed=7), tr, f0)
    assert _same(obs, tr) and _same(cmd, f0)
    assert st["clock"].tolist() == [[1, 4]] * 5
    assert np.array_equal(st["draw"], np.tile([0.0] * 12 + [1.0] * 4, (5, 1)))  # (a zero bias: 0 * sym, either sign)


@pytest.mark.parametrize("d", (1, 3, 8))
def test_delay_alone(d):
    tr, f0 = _truths(3, 20)
    obs, cmd, _ = _run(CM.params(delay=d), tr, f0)
    for tau in range(20):
        assert _same(obs[tau], tr[max(tau - d, 0)]), tau
    assert _same(cmd, f0)


@pytest.mark.parametrize("lat", (1, 4))
def test_latency_alone(lat):
    tr, f0 = _truths(3, 12)
    obs, cmd, _ = _run(CM.params(latency=lat), tr, f0)
    for tau in range(12):
        assert _same(cmd[tau], np.tile(CM.F_INIT, (3, 1)) if tau < lat else f0[tau - lat]), tau
    assert _same(obs, tr)


def test_holds_repeat_the_previous_observation():
    import mpcq
    tr, f0 = _truths(40, 15)
    p = CM.params(seed=5, hold_prob=0.4)
    obs, _, _ = _run(p, tr, f0)
    held = mpcq.channel.held(_ctypes(p), np.arange(40)[None, :], 1, np.arange(15)[:, None])
    held[0] = False  # a first tick never holds
    assert 0.25 < held[1:].mean() < 0.55
    for t in range(15):
        want = np.where(held[t][:, None], obs[t - 1] if t else tr[0], tr[t])
        assert _same(obs[t], want), t
    obs1, _, _ = _run(CM.params(seed=5, hold_prob=1.0), tr, f0)
    assert all(_same(obs1[t], tr[0]) for t in range(15))  # every non-first tick holds
    # with a delay the ring advances under a held tick
    p2 = CM.params(seed=5, hold_prob=0.4, delay=2)
    obs2, _, _ = _run(p2, tr, f0)
    for t in range(1, 15):
        want = np.where(held[t][:, None], obs2[t - 1], tr[max(t - 2, 0)])
        assert _same(obs2[t], want), t


MIXED = dict(seed=11, delay=2, latency=1, hold_prob=0.3, sigma=[0.0, 0.01, 0.02] * 4, bias=[0.05, 0.0, 0.1] * 4,
             f_sigma=[0.5, 0.0, 1.0], f_gain=0.2)


def test_a_first_flag_restarts_that_robot_only():
    tr, f0 = _truths(6, 12, seed=3)
    p = CM.params(**MIXED)
    mask = np.array([0, 1, 0, 0, 1, 0])
    obs_a, cmd_a, st_a = _run(p, tr, f0)
    obs_b, cmd_b, st_b = _run(p, tr, f0, first={7: mask})
    keep = mask == 0
    assert _same(obs_a[:, keep], obs_b[:, keep]) and _same(cmd_a[:, keep], cmd_b[:, keep])
    for k in st_a:
        assert _same(st_a[k][keep], st_b[k][keep]), k
    assert st_b["clock"].tolist() == [[2, 5] if m else [1, 12] for m in mask]
    r = np.nonzero(mask)[0]
    # a new epoch: other bias and gains, the state ring refilled, the initial result back in force
    assert not np.array_equal(st_a["draw"][r], st_b["draw"][r])
    b2 = p.bias * CM.sym(CM.philox(p, r[:, None], 2, 0, CM.S_BIAS + np.arange(12)))
    assert _same(st_b["draw"][r, :12], b2)
    n7 = CM.n(CM.philox(p, r[:, None], 2, 0, CM.S_NOISE + np.arange(12)))
    want7 = tr[7][r].copy()
    for i in range(12):
        if p.bias[i] != 0.0:
            want7[:, i] = want7[:, i] + b2[:, i]
        if p.sigma[i] != 0.0:
            want7[:, i] = want7[:, i] + p.sigma[i] * n7[:, i]
    assert _same(obs_b[7][r], want7)
    g2 = st_b["draw"][r, 12:]
    f7 = CM.n(CM.philox(p, r[:, None], 2, 0, CM.S_FORCE + np.arange(12)))
    fs = np.tile(p.f_sigma, 4)
    want = CM.F_INIT * np.repeat(g2, 3, axis=1)
    assert _same(cmd_b[7][r], np.where(fs != 0.0, want + fs * f7, want))


def test_priming_in_mid_run():
    """Armed robots refill their rings at the next observe, keep epoch and tau, and take the
    tick's own f0 into the force ring; the others go on."""
    tr, f0 = _truths(4, 10, seed=4)
    p = CM.params(delay=3, latency=2)
    st = CM.new_state(4)
    for t in range(5):
        CM.observe(p, st, tr[t], all_first=t == 0)
        CM.actuate(p, st, f0[t])
    CM.arm(st, mask=[1, 0, 0, 1])
    assert st["clock"][:, 1].tolist() == [~5, 5, 5, ~5]
    for t in range(5, 10):
        o = CM.observe(p, st, tr[t])
        c = CM.actuate(p, st, f0[t])
        assert _same(o[[1, 2]], tr[t - 3][[1, 2]]) and _same(c[[1, 2]], f0[t - 2][[1, 2]])
        assert _same(o[[0, 3]], tr[max(t - 3, 5)][[0, 3]]) and _same(c[[0, 3]], f0[max(t - 2, 5)][[0, 3]])
    assert st["clock"].tolist() == [[1, 10]] * 4 and (st["draw"][:, 12] == 1.0).all()
    # a fresh group primes on its first observe without a first flag: epoch 0, tau 0
    st = CM.new_state(2)
    o = CM.observe(p, st, tr[0][:2])
    assert _same(o, tr[0][:2]) and st["clock"].tolist() == [[0, 1]] * 2 and (st["draw"][:, 12] == -1.0).all()
    c = CM.actuate(p, st, f0[0][:2])
    assert _same(c, f0[0][:2]) and (st["draw"][:, 12] == 1.0).all() and _same(st["f_ring"], np.repeat(f0[0][:2, None], 4, 1))


@pytest.mark.parametrize("field", [k for k in MIXED if k != "seed"] + ["seed"])
def test_every_field_acts(field):
    """Putting any one nonzero field of the mixed case back to zero changes the output (the
    seed: to another value)."""
    tr, f0 = _truths(8, 12, seed=6)
    obs_a, cmd_a, _ = _run(CM.params(**MIXED), tr, f0)
    zero = dict(MIXED)
    zero[field] = [0.0] * len(MIXED[field]) if isinstance(MIXED[field], list) else 0
    obs_b, cmd_b, _ = _run(CM.params(**zero), tr, f0)
    which = {"delay": "obs", "hold_prob": "obs", "sigma": "obs", "bias": "obs", "latency": "cmd", "f_sigma": "cmd",
             "f_gain": "cmd", "seed": "both"}[field]
    if which in ("obs", "both"):
        assert not _same(obs_a, obs_b)
    else:
        assert _same(obs_a, obs_b)
    if which in ("cmd", "both"):
        assert not _same(cmd_a, cmd_b)
    else:
        assert _same(cmd_a, cmd_b)
    # component by component: an amplitude set to zero silences exactly its components
    if field in ("sigma", "bias"):
        half = dict(MIXED)
        half[field] = [0.0 if i == 2 else v for i, v in enumerate(MIXED[field])]
        obs_c, _, _ = _run(CM.params(**half), tr, f0)
        diff = (CM.bits(obs_a) != CM.bits(obs_c)).any(axis=(0, 1))
        assert diff.tolist() == [i == 2 for i in range(12)]
