"""CPU: the monitor's host model (tests/monitor_model.py) on hand-computed cases -- the model is
what the GPU tests hold the kernel to, so its own rules are pinned here against include/mpcq.h."""
import numpy as np

import monitor_model as MM

STAND = np.array([0.0, 0.0, 0.2, 0.0, 0.0, 0.0])


def _tick(q_w, status=1, iters=10, f0=None, cost=None, state=None, v_ref=None, acc=None, **kw):
    q_w = np.atleast_2d(np.asarray(q_w, np.float64))
    B = q_w.shape[0]
    acc = MM.new_state(B) if acc is None else acc
    f0 = np.zeros((B, 12)) if f0 is None else np.broadcast_to(np.asarray(f0, np.float64), (B, 12))
    cost = np.zeros((B, 13)) if cost is None else np.broadcast_to(np.asarray(cost, np.float64), (B, 13))
    state = np.zeros((B, 12)) if state is None else np.broadcast_to(np.asarray(state, np.float64), (B, 12))
    v_ref = np.zeros(6) if v_ref is None else v_ref
    done, trace = MM.step(q_w, np.broadcast_to(np.int32(status), (B,)), np.broadcast_to(np.int32(iters), (B,)),
                          f0, cost, state, v_ref, acc, **kw)
    return done, trace, acc


def _pose(**kw):
    q = STAND.copy()
    for k, v in kw.items():
        q["x y z roll pitch yaw".split().index(k)] = v
    return q


def test_each_bit_alone_and_several_together():
    kw = dict(max_tilt=0.5, min_height=0.1, max_ticks=0)
    poses = [STAND, _pose(roll=0.6), _pose(pitch=-0.6), _pose(z=0.05), _pose(x=np.inf), _pose(roll=0.7, z=0.0)]
    done, _, _ = _tick(poses, **kw)
    assert done.tolist() == [0, MM.TILT, MM.TILT, MM.HEIGHT, MM.NONFINITE, MM.TILT | MM.HEIGHT]
    for st, want in ((1, 0), (2, 0), (-2, 0), (3, MM.SOLVER), (4, MM.SOLVER), (-3, MM.SOLVER), (-4, MM.SOLVER),
                     (-10, MM.SOLVER), (-11, MM.SOLVER), (-12, MM.SOLVER), (-13, MM.SOLVER), (0, MM.SOLVER)):
        done, _, _ = _tick(STAND, status=st, **kw)
        assert done.tolist() == [want], st
    # an infinite roll is non-finite and beyond the tilt; a failed solve on a fallen robot: both
    done, _, _ = _tick([_pose(roll=np.inf), _pose(z=0.01)], status=-3, **kw)
    assert done.tolist() == [MM.NONFINITE | MM.TILT | MM.SOLVER, MM.HEIGHT | MM.SOLVER]
    done, _, _ = _tick(_pose(z=-np.inf), **kw)
    assert done.tolist() == [MM.NONFINITE | MM.HEIGHT]
    # thresholds switched off
    done, _, _ = _tick([_pose(roll=3.0), _pose(z=-5.0)], max_tilt=np.inf, min_height=-np.inf)
    assert done.tolist() == [0, 0]


def test_a_threshold_met_exactly_is_not_done():
    poses = [_pose(roll=0.5), _pose(pitch=-0.5), _pose(z=0.1), _pose(roll=np.nextafter(0.5, 1.0)),
             _pose(z=np.nextafter(0.1, 0.0))]
    done, _, _ = _tick(poses, max_tilt=0.5, min_height=0.1)
    assert done.tolist() == [0, 0, 0, MM.TILT, MM.HEIGHT]


def test_a_nan_pose_is_nonfinite_only():
    for slot in range(6):
        q = STAND.copy()
        q[slot] = np.nan
        done, _, acc = _tick(q, max_tilt=0.5, min_height=0.1)
        assert done.tolist() == [MM.NONFINITE], slot
        # slots 3 and 4 were left alone on that tick (then the episode restarted)
        assert acc["last"][0, 3] == 0.0 and acc["last"][0, 4] == np.inf


def test_accumulators_by_hand():
    cost = np.arange(13.0)  # sum 78
    f0 = np.full(12, 2.0)   # f0 . f0 = 48
    state = np.zeros(12)
    state[[6, 7, 11]] = [0.5, -0.25, 1.0]
    v_ref = np.array([0.25, 0.0, 9.0, 9.0, 9.0, 0.5])  # (0.25, -0.25, 0.5): 0.0625 + 0.0625 + 0.25
    acc = MM.new_state(1)
    done, trace, _ = _tick(_pose(roll=0.1, pitch=-0.2, z=0.19), iters=25, f0=f0, cost=cost, state=state,
                           v_ref=v_ref, acc=acc)
    assert done.tolist() == [0]
    assert acc["ep"][0].tolist() == [78.0, 48.0, 25.0, 0.2, 0.19, 0.375, 0.0, 0.0]
    assert acc["ep_ticks"].tolist() == [1] and acc["episodes"].tolist() == [0] and not acc["last"].any()
    assert trace[0].tolist() == [0.0, 0.0, 0.19, 0.1, -0.2, 0.0, 0.0, 1.0, 25.0, 1.0, 78.0, 48.0, 0.0, 0.0, 0.0, 0.0]
    _tick(_pose(roll=-0.3, pitch=0.1, z=0.21), iters=50, f0=f0, cost=cost, state=state, v_ref=v_ref, acc=acc)
    assert acc["ep"][0].tolist() == [156.0, 96.0, 75.0, 0.3, 0.19, 0.75, 0.0, 0.0]
    assert acc["ep_ticks"].tolist() == [2]
    assert acc["totals"].tolist() == [2, 0, 0, 0, 0, 0, 0, 0]
    # left to right: 1e16 + 1 + 1 ... stays 1e16, while any pairwise order would not
    c2 = np.ones(13)
    c2[0] = 1e16
    a2 = MM.new_state(1)
    _tick(STAND, cost=c2, acc=a2)
    assert a2["ep"][0, 0] == 1e16


def test_a_solver_tick_skips_its_sums():
    cost, f0 = np.arange(13.0), np.full(12, 2.0)
    state = np.ones(12)
    acc = MM.new_state(1)
    _tick(_pose(roll=0.1), iters=5, f0=f0, cost=cost, state=state, acc=acc)
    before = acc["ep"][0].copy()
    done, trace, _ = _tick(_pose(roll=0.25, z=0.15), status=-11, iters=7, f0=np.full(12, np.nan),
                           cost=np.full(13, np.nan), state=np.full(12, np.nan), acc=acc)
    assert done.tolist() == [MM.SOLVER]
    last = acc["last"][0]
    assert last[0] == before[0] and last[1] == before[1] and last[5] == before[5]  # nothing added
    assert last[2] == before[2] + 7.0 and last[3] == 0.25 and last[4] == 0.15      # these still move
    assert last[8] == 2.0 and last[9] == MM.SOLVER and last[10:16].tolist() == _pose(roll=0.25, z=0.15).tolist()
    assert np.isnan(trace[0, 10]) and np.isnan(trace[0, 11])  # the trace shows the tick as it was


def test_the_episode_restarts_after_a_done_tick():
    acc = MM.new_state(2)
    cost = np.ones(13)
    _tick([STAND, STAND], cost=cost, acc=acc)
    done, trace, _ = _tick([_pose(roll=0.9), STAND], cost=cost, acc=acc)
    assert done.tolist() == [MM.TILT, 0]
    assert acc["ep"][0].tolist() == [0.0, 0.0, 0.0, 0.0, np.inf, 0.0, 0.0, 0.0]
    assert acc["ep"][1, 0] == 26.0
    assert acc["ep_ticks"].tolist() == [0, 2] and acc["episodes"].tolist() == [1, 0]
    assert acc["last"][0, 0] == 26.0 and acc["last"][0, 3] == 0.9 and acc["last"][0, 8] == 2.0
    assert not acc["last"][1].any()
    assert trace[:, 9].tolist() == [2.0, 2.0]  # before the restart
    _tick([STAND, STAND], cost=cost, acc=acc)
    assert acc["ep"][0, 0] == 13.0 and acc["ep_ticks"].tolist() == [1, 3]
    assert acc["totals"].tolist() == [6, 1, 0, 1, 0, 0, 0, 0]
    # an explicit reset discards the running episode and counts nothing
    MM.reset(acc, [0, 1])
    assert acc["ep"][1].tolist() == [0.0, 0.0, 0.0, 0.0, np.inf, 0.0, 0.0, 0.0] and acc["ep_ticks"].tolist() == [1, 0]
    assert acc["episodes"].tolist() == [1, 0] and acc["ep"][0, 0] == 13.0


def test_timeout_at_exactly_max_ticks():
    acc = MM.new_state(1)
    seen = []
    for _ in range(7):
        done, _, _ = _tick(STAND, acc=acc, max_ticks=3)
        seen.append(int(done[0]))
    assert seen == [0, 0, MM.TIMEOUT, 0, 0, MM.TIMEOUT, 0]
    assert acc["last"][0, 8] == 3.0 and acc["episodes"].tolist() == [2] and acc["ep_ticks"].tolist() == [1]
    done, _, _ = _tick(STAND, max_ticks=1)
    assert done.tolist() == [MM.TIMEOUT]
    done, _, _ = _tick(STAND, max_ticks=0)
    assert done.tolist() == [0]


def test_batch_generator_reaches_every_bit_and_boundary():
    """Properties of the GPU batch test's inputs (tests/monitor_cases.py), checked where no
    device is needed: every reason bit occurs for B >= 63, the robots sitting exactly at a
    threshold end by the tick limit alone, and NaN and infinite poses are among the inputs."""
    import monitor_cases as MC
    for B in (1, 63, 64, 65, 130):
        calls = MC.batch_calls(B, 500 + B)
        runs = MC.model_calls(calls, B)
        exact = list(set(MC.exact_robots(B)))
        seen = 0
        for c, (done, _, _) in enumerate(runs):
            seen |= int(np.bitwise_or.reduce(done))
            assert (done[exact] == (MM.TIMEOUT if c == 1 else 0)).all(), (B, c)
        assert calls[0]["q_w"][exact[0], 3] == MC.PARAMS["max_tilt"]
        assert set(np.concatenate([c["status"] for c in calls]).tolist()) <= set(MC.STATUSES)
        if B >= 63:
            assert seen == sum(MM.BITS), (B, seen)
            assert set(np.concatenate([c["status"] for c in calls]).tolist()) == set(MC.STATUSES), B
            assert any(np.isnan(c["q_w"]).any() for c in calls) and any(np.isinf(c["q_w"]).any() for c in calls)
            assert (runs[-1][2]["totals"][1:7] > 0).all(), B


def test_worst_case_pushes_cross_their_thresholds():
    """The session tests' pushes end an episode within 4 ticks whatever the controller does:
    with every foot in stance and resisting with fz_max (monitor_cases.worst_case)."""
    import monitor_cases as MC
    h, t = MC.worst_case("height"), MC.worst_case("tilt")
    assert h[2][0] < 0.1 and h[3][0] < 0.1 - 0.1  # 0.075 after 3 ticks, -0.023 after 4
    assert t[2][1] > 0.5 + 0.5 and t[3][1] > 0.5 + 1.0  # 1.04 rad after 3 ticks, 1.83 after 4
    assert all(tilt == 0.0 for _, tilt in h)  # the downward push does not tilt


def test_same_is_bitwise():
    a = np.array([0.0, np.nan, 1.0])
    assert MM.same(a, a.copy())
    assert not MM.same(a, np.array([-0.0, np.nan, 1.0]))
    assert not MM.same(a, np.array([0.0, 2.0, 1.0]))
    assert not MM.same(np.zeros(2, np.int32), np.zeros(2, np.int64))
