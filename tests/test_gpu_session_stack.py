"""GPU: a session with all nine optional stages and the four tables on, checked launch by launch on
the inputs its own tick read (tests/session_stack.py holds the chain and says what each launch
must have read).

The session: N = 16, B = 7 (odd: an empty half in the last planner wave; 4 + 3 for the 16-lane
stages; a tail of the swing kernel's 16 robots per wave), mixed trot / bound tables, per-robot
model and plant robots, weights, a user disturbance table, a wrench on robot 1, swing, plant,
monitor (episodes of 13 ticks), scenario (commands, pushes, robots), channel (delay 2, latency 1,
noise, bias, held frames, leg gains), estimator, compensating disturb stage, gait transitions with
requests ahead of a few ticks; robot 5's table loses its terminator before tick 17.  40 ticks:
more than two gait periods, three episodes.  The test resets the robots the monitor marks itself
(test_auto_reset_is_the_callers_reset: that is auto-reset), after reading every array, so no array
is overwritten before it is read and every (robot, tick) is checked.

Bit equality everywhere, except the plant's states against the numpy model (session_stack.PLANT_TOL
= test_gpu_plant.TOL; against Plant.step on the robots without a wrench: bits).  SV_ORDER is
compared as a permutation: the order inside a bucket is arbitrary by design.

Companions on fresh sessions: the auto-reset twin (every array after every tick), ``run`` in one
call per stretch between two interventions of the schedule (final arrays and the trace), and the
same chain at N = 48 (one robot per planner wave; the engine's S^-1 / R^-1 Q in the workspace).
"""
import numpy as np
import pytest

import session_stack as SS
from monitor_model import same

pytestmark = pytest.mark.gpu

N, B, T = 16, 7, 40
BAD = 5  # the robot that loses its gait terminator


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


def _explicit(mpcq, oracle, eng, cfg, ticks):
    """The session with the test's own resets, every tick checked.  Returns the chain and, per
    tick, every array as the tick and its reset leave it."""
    history = []
    with SS.open_stack(mpcq, eng, cfg, auto_reset=0) as sess:
        chain = SS.Chain(mpcq, oracle, eng, sess, cfg)
        for k in range(ticks):
            SS.before_tick(mpcq, sess, cfg, k)
            b4 = SS.read_all(mpcq, sess)
            sess.tick(None)
            now = SS.read_all(mpcq, sess)
            chain.check(k, b4, now)
            done = now["MV_DONE"] != 0
            if done.any():
                sess.reset(done)
                chain.after_reset(done)
                now = SS.read_all(mpcq, sess)
            history.append(now)
    return chain, history


class _Stack:
    """The 40-tick run on its engine, made and checked by the first test that asks for it; the
    companions compare their sessions with its history (and fail with it if it failed)."""

    def __init__(self, mpcq, oracle, eng):
        self.mpcq, self.oracle, self.eng = mpcq, oracle, eng
        self.cfg = SS.config(mpcq, N, B, bad_gait=BAD)
        self.out = self.err = None

    def get(self):
        if self.err is not None:
            raise self.err
        if self.out is None:
            try:
                self.out = _explicit(self.mpcq, self.oracle, self.eng, self.cfg, T)
            except BaseException as e:
                self.err = e
                raise
        return (self.cfg, self.eng) + self.out


@pytest.fixture(scope="module")
def stack(mpcq, oracle):
    with mpcq.Engine(N) as eng:
        yield _Stack(mpcq, oracle, eng)


def test_every_launch_on_its_own_inputs(mpcq, stack):
    cfg, eng, chain, history = stack.get()
    s = chain.seen
    print(f"stack N={N} B={B} T={T}: plant states against the numpy model {chain.worst_plant:.2e} (bound "
          f"{SS.PLANT_TOL:.0e}); met {s}")
    # the run has power: it cannot pass by doing nothing
    assert s["first_late"] > 0          # a first flag at a tick k > 0
    assert s["held"] > 0                # a frame held by the channel
    assert s["pushed"] > 0              # a tick with a push
    assert s["switched"] > 0            # an active gait changed
    assert s["bad_gait"] > 0 and s["warm_solved"] > 0
    assert s["dist_differs"] > 0        # DV_DIST non-zero and not the user's table
    assert s["plant_bits"] > 0 and s["failed_plant"] > 0
    episodes = history[-1]["MV_EPISODES"]
    assert (episodes >= 3).all(), episodes  # three episodes of 13 ticks in 40
    assert history[-1]["CV_ROBOTS"].tobytes() != cfg["plant_robots"].tobytes()  # the scenario's robots differ


def test_inputs_have_power_on_the_host(mpcq):
    """What can be settled without a device: the scenario pushes, the channel holds a frame."""
    sc = mpcq.default_scenario_params(**SS.SCENARIO)
    ch = mpcq.default_channel_params(**SS.CHANNEL)
    robots, ticks = np.arange(B)[:, None], np.arange(SS.MAX_TICKS)[None, :]
    _, active = mpcq.scenario.push(sc, robots, 0, ticks)
    assert active.any()
    assert mpcq.channel.held(ch, robots, 0, ticks[:, 3:]).any()
    assert SS.MAX_TICKS < T


def test_auto_reset_twin(mpcq, stack):
    cfg, eng, chain, history = stack.get()
    with SS.open_stack(mpcq, eng, cfg, auto_reset=1) as twin:
        for k in range(T):
            SS.before_tick(mpcq, twin, cfg, k)
            twin.tick(None)
            SS.same_reads(SS.read_all(mpcq, twin), history[k], ("auto-reset twin", k))


def test_run_twin(mpcq, stack):
    cfg, eng, chain, history = stack.get()
    cuts = [0] + [t for t in SS.intervention_ticks(cfg) if 0 < t < T] + [T]
    rows = []
    with SS.open_stack(mpcq, eng, cfg, auto_reset=1) as twin:
        for a, b in zip(cuts[:-1], cuts[1:]):
            SS.before_tick(mpcq, twin, cfg, a)
            rows.append(twin.run(None, b - a, trace=True))
        SS.same_reads(SS.read_all(mpcq, twin), history[-1], "run twin")
        assert twin.k == T
    trace = np.concatenate(rows)
    assert trace.shape == (T, B, mpcq.TRACE) and same(trace, np.stack(chain.trace))


def test_a_horizon_above_32(mpcq, oracle):
    """N = 48 (three periods of the 16-step cycles), B = 3, 6 ticks, no bad-gait robot."""
    n, b, ticks = 48, 3, 6
    cfg = SS.config(mpcq, n, b)
    with mpcq.Engine(n) as eng:
        chain, history = _explicit(mpcq, oracle, eng, cfg, ticks)
    print(f"stack N={n} B={b} T={ticks}: plant states against the numpy model {chain.worst_plant:.2e}; met {chain.seen}")
    assert chain.seen["switched"] > 0 and chain.seen["warm_solved"] > 0 and chain.seen["dist_differs"] > 0
    assert set(chain.seen["statuses"]) <= {1, 2, -2}, chain.seen["statuses"]
