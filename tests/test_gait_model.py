"""CPU: the gait model (tests/gait_model.py) against hand-written tables, its two anchors to the
reference's roll (oracle.Planner.plan(PLAN_ROLL)), the trot -> bound -> stand -> trot schedule's
properties, and the schedule in closed loop on the oracle's pieces."""
import numpy as np
import pytest

import gait_cases as GC
import gait_model as GM

ALL = (1, 1, 1, 1)
A, B_ = (1, 0, 0, 1), (0, 1, 1, 0)  # trot's diagonals


def _tab(*rows):
    g = np.zeros((20, 5))
    for r, row in enumerate(rows):
        g[r] = row
    return g


def _one(p, lib, g, st, v_ref=None):
    g, st = g.copy(), np.array(st, np.int32)
    wrote = GM.roll_one(p, np.asarray(lib, np.float64), v_ref, g, st)
    return g, tuple(int(v) for v in st), wrote


PLAIN = GM.params(n_gaits=1)
LIB3 = GC.LIB[:3]  # trot, bound, stand
P3 = GM.params(n_gaits=3)


def test_roll_branches_without_a_gait():
    """active = -1 is the reference's roll: each of its four branches."""
    none = (-1, -1, 0, 0)
    # row 0's contacts equal row last's: that count += 1; front count > 1: decremented
    g, st, wrote = _one(PLAIN, GC.LIB[:1], _tab((3, *A), (2, *B_), (1, *A)), none)
    assert wrote and st == none
    assert np.array_equal(g, _tab((2, *A), (2, *B_), (2, *A)))
    # they differ: a new row [1, row 0's contacts]
    g, _, _ = _one(PLAIN, GC.LIB[:1], _tab((3, *A), (2, *B_)), none)
    assert np.array_equal(g, _tab((2, *A), (2, *B_), (1, *A)))
    # front count 1: the rows shift up, row 19 zero
    g, _, _ = _one(PLAIN, GC.LIB[:1], _tab((1, *ALL), (2, *B_)), none)
    assert np.array_equal(g, _tab((2, *B_), (1, *ALL)))
    # a single row appends to itself and is decremented
    g, _, _ = _one(PLAIN, GC.LIB[:1], _tab((5, *ALL)), none)
    assert np.array_equal(g, _tab((5, *ALL)))
    # 19 rows in use, row 18's contacts equal row 0's: its count += 1, then the shift
    rows = [(1, r % 2, 1, (r + 1) % 2, 1) for r in range(19)]
    g, _, _ = _one(PLAIN, GC.LIB[:1], _tab(*rows), none)
    assert np.array_equal(g, _tab(*(rows[1:18] + [(2, 0, 1, 1, 1)])))
    # 18 rows in use, row 17 differs from row 0: a new row 18, then the shift
    g, _, _ = _one(PLAIN, GC.LIB[:1], _tab(*rows[:18]), none)
    assert np.array_equal(g, _tab(*(rows[1:18] + [rows[0]])))
    # 19 rows in use and a new row into row 19 without a shift: no zero row is left
    rows2 = [(2, *A)] + [(1, r % 2, 1, (r + 1) % 2, 1) for r in range(18)]
    g, _, wrote = _one(PLAIN, GC.LIB[:1], _tab(*rows2), none)
    assert wrote and (g[:, 0] != 0).all() and np.array_equal(g[19], (1, *A)) and g[0, 0] == 1


def test_switch_waits_for_the_boundary_then_starts_the_cycle():
    g = GC.table("trot", 16)  # [1 all][7 A][1 all][7 B]
    st = np.array([GC.BOUND, -1, 0, 0], np.int32)
    # tick 0: row 0 (all) differs from row last (B): a boundary at once
    GM.roll_one(P3, LIB3, None, g, st)
    assert tuple(st) == (GC.BOUND, GC.BOUND, 1, 1) and np.array_equal(g[3], (1, *ALL))
    # now mid-cycle of bound: a request for trot waits until bound's phase is a row's first step
    st[0] = GC.TROT
    seen = []
    for t in range(1, 12):
        GM.roll_one(P3, LIB3, None, g, st)
        seen.append(int(st[1]))
        assert g[:, 0].sum() == 16
    # bound's rows start at steps 0, 1, 8, 9: phase 1 (tick 1) is a boundary
    assert seen[0] == GC.TROT and st[3] == 2
    # a running trot cycle (phase 3, mid-row) refuses, and takes the switch at step 8
    g = GC.table("trot", 16)
    st = np.array([GC.BOUND, GC.TROT, 3, 0], np.int32)
    took = None
    for t in range(8):
        GM.roll_one(P3, LIB3, None, g, st)
        if st[1] == GC.BOUND and took is None:
            took = t
    assert took == 5  # phases 3..7 run out (ticks 0..4), step 8 starts a row: tick 5


def test_align_zero_switches_at_once():
    p = GM.params(n_gaits=3, align=0)
    g = GC.table("trot", 16)
    st = np.array([GC.BOUND, GC.TROT, 3, 0], np.int32)
    GM.roll_one(p, LIB3, None, g, st)
    assert tuple(st) == (GC.BOUND, GC.BOUND, 1, 1)
    g = GC.table("trot", 16)
    g, st, _ = _one(p, LIB3, _tab((2, *A), (1, *A)), (GC.BOUND, -1, 0, 0))  # row 0 == row last, index 2: no boundary
    assert st == (GC.BOUND, GC.BOUND, 1, 1)
    g, st, _ = _one(P3, LIB3, _tab((2, *A), (1, *A)), (GC.BOUND, -1, 0, 0))
    assert st == (GC.BOUND, -1, 0, 0)


def test_stand_leaves_at_any_tick_and_a_one_row_table_is_a_boundary():
    for ticks in range(1, 6):
        g = GC.table("trot", 16)
        st = np.array([GC.STAND, GC.STAND, 0, 1], np.int32)
        for _ in range(ticks):
            GM.roll_one(P3, LIB3, None, g, st)
        st[0] = GC.TROT
        GM.roll_one(P3, LIB3, None, g, st)
        assert tuple(st) == (GC.TROT, GC.TROT, 1, 2), ticks
    g, st, _ = _one(P3, LIB3, _tab((16, *ALL)), (GC.TROT, -1, 0, 0))  # index == 1
    assert st == (GC.TROT, GC.TROT, 1, 1) and np.array_equal(g, _tab((16, *ALL)))


def test_a_request_withdrawn_before_it_is_taken():
    g = GC.table("trot", 16)
    st = np.array([GC.BOUND, GC.TROT, 3, 0], np.int32)
    GM.roll_one(P3, LIB3, None, g, st)
    assert st[1] == GC.TROT
    st[0] = -1
    for _ in range(20):
        GM.roll_one(P3, LIB3, None, g, st)
    assert st[0] == -1 and st[1] == GC.TROT and st[3] == 0  # the active gait stays active


def test_defensive_reads():
    g0 = GC.table("trot", 16)
    for bad in (-2, 3, 99, -2 ** 31, 2 ** 31 - 1):
        g, st, _ = _one(P3, LIB3, g0, (bad, -1, 5, 0))
        assert st == (-1, -1, 5, 0)  # want read as -1; phase is not touched without a gait
        g, st, _ = _one(P3, LIB3, g0, (-1, bad, 5, 0))
        assert st == (-1, -1, 5, 0)
        assert np.array_equal(g, _one(PLAIN, LIB3[:1], g0, (-1, -1, 0, 0))[0])
    for ph, want in ((16, 1), (-1, 0), (35, 4), (-17, 0), (2 ** 31 - 1, (2 ** 31 - 1) % 16 + 1), (-2 ** 31, 1)):
        g, st, _ = _one(P3, LIB3, g0, (-1, GC.TROT, ph, 0))
        assert st == (-1, GC.TROT, want % 16, 0), ph


SP = GM.params(n_gaits=4, select=GM.BY_SPEED, thresholds=GC.THRESHOLDS, hysteresis=GC.HYSTERESIS)


def _v(vx, wz=0.0, vy=0.0):
    return np.array([vx, vy, 0.0, 0.0, 0.0, wz])


def test_by_speed_bands_and_thresholds():
    for vx, band in ((0.0, 0), (np.nextafter(0.25, 0), 0), (0.25, 1), (0.5, 2), (np.nextafter(1.0, 0), 2), (1.0, 3), (9.0, 3),
                     (-0.5, 2)):
        assert GM.select(SP, -1, _v(vx)) == band, vx
    # the yaw term: 0.2 m/s and 1 rad/s
    s = 0.2 + GM.YAW_WEIGHT
    assert GM.select(SP, -1, _v(0.2, wz=-1.0)) == (1 if s < 0.5 else 2)
    # the last n_gaits - 1 thresholds only: a two-entry library has one band edge
    p2 = GM.params(n_gaits=2, select=GM.BY_SPEED, thresholds=(0.25, 0.5))
    assert GM.select(p2, -1, _v(9.0)) == 1
    assert GM.select(GM.params(n_gaits=1, select=GM.BY_SPEED), -1, _v(9.0)) == 0


def test_hysteresis_both_directions_and_one_direction_per_tick():
    h = GC.HYSTERESIS
    assert GM.select(SP, 1, _v(0.5 + h)) == 1            # not strictly above: stays
    assert GM.select(SP, 1, _v(np.nextafter(0.5 + h, 9))) == 2
    assert GM.select(SP, 1, _v(0.25 - h)) == 1           # not strictly below: stays
    assert GM.select(SP, 1, _v(np.nextafter(0.25 - h, 0))) == 0
    assert GM.select(SP, 0, _v(5.0)) == 3                # a chain of bands up in one call
    assert GM.select(SP, 3, _v(0.0)) == 0                # and down
    assert GM.select(SP, 2, _v(0.5)) == 2                # inside the dead band
    # up and down in one call cannot happen: thresholds that coincide, a speed between the edges
    p = GM.params(n_gaits=3, select=GM.BY_SPEED, thresholds=(0.5, 0.5), hysteresis=0.0)
    assert GM.select(p, 0, _v(0.75)) == 2 and GM.select(p, 2, _v(0.25)) == 0


def test_nan_speed_moves_nothing():
    for want in (-1, 0, 2, 3):
        assert GM.select(SP, want, _v(np.nan)) == want
        assert GM.select(SP, want, _v(0.1, wz=np.nan)) == want
    assert GM.select(SP, -1, _v(np.inf)) == 3


def test_no_zero_row_is_left_untouched():
    g0 = _tab(*[(2, r % 2, 1, (r + 1) % 2, 1) for r in range(20)])
    for st0 in ((GC.BOUND, -1, 0, 0), (7, 9, -3, 2), (-1, GC.TROT, 40, 1)):
        g, st, wrote = _one(P3, LIB3, g0, st0)
        assert not wrote and st == st0 and np.array_equal(g, g0)
    g, st, wrote = _one(SP, GC.SPEED_LIB, g0, (-1, -1, 0, 0), _v(0.7))
    assert not wrote and st == (-1, -1, 0, 0)


def test_sum_of_counts_is_constant():
    rng = np.random.default_rng(3)
    gait, state = GC.random_tables(rng, 64)
    sums = gait[:, :, 0].sum(axis=1)
    p = GM.params(n_gaits=4)
    for _ in range(40):
        GM.roll(p, GC.LIB, None, gait, state)
        assert np.array_equal(gait[:, :, 0].sum(axis=1), sums)
        assert ((state[:, 1] >= -1) | (gait[:, :, 0] != 0).all(axis=1)).all()


# ---------------------------------------------------------------- anchors to the reference
def _oracle_roll(O, N, g0, ticks, T_gait):
    pl = O.Planner(N, g0, O.default_planner_params(T_gait=T_gait))
    out = []
    z = np.zeros(12)
    for k in range(ticks):
        assert pl.plan(O.PLAN_ROLL, k, z, np.zeros((3, 4)), np.zeros(6)) == 0
        out.append(pl.gait.copy())
    return out


@pytest.mark.parametrize("N", [16, 32])
@pytest.mark.parametrize("name", ["trot", "bound"])
def test_anchor_own_cycle_is_the_reference_roll(oracle, N, name):
    """A cycle equal to the table's own period, P | N, requested before tick 0: the reference's
    roll on every one of 64 ticks."""
    lib = np.stack([GC.cycle(name)])
    g, st = GC.table(name, N), np.array([0, -1, 0, 0], np.int32)
    ref = _oracle_roll(oracle, N, g, 64, 0.32)
    for k in range(64):
        GM.roll_one(PLAIN, lib, None, g, st)
        assert np.array_equal(g, ref[k]), k
    assert tuple(st) == (0, 0, 64 % 16, 1)


def test_anchor_period_not_dividing_the_horizon(oracle):
    """The period-8 trot cycle on the N = 12 table [1 all][5 A][1 all][5 B]: the reference's
    roll up to tick 3, first different at tick 4."""
    lib = np.stack([GC.cycle("trot", half=4)])
    g, st = GC.table("trot", 12, half=6), np.array([0, -1, 0, 0], np.int32)
    ref = _oracle_roll(oracle, 12, g, 12, 0.24)
    same = []
    for k in range(12):
        GM.roll_one(PLAIN, lib, None, g, st)
        same.append(np.array_equal(g, ref[k]))
        assert g[:, 0].sum() == 12
    assert same[:4] == [True] * 4 and not same[4]


# ---------------------------------------------------------------- the schedule
def test_schedule_switch_ticks_and_swing_lengths():
    """trot -> bound -> stand -> trot (-> bound) at N = 16, one robot, 120 ticks, align = 1."""
    reqs = {t: np.array([g], np.int32) for t, g in GC.SCHEDULE}
    gs, ss = GC.model_run(GC.table("trot", 16)[None], LIB3, P3, 120, reqs)
    sw = [t for t in range(120) if ss[t, 0, 3] != (ss[t - 1, 0, 3] if t else 0)]
    assert sw == [8, 32, 55, 63]
    assert (gs[:, 0, :, 0].sum(axis=1) == 16).all()
    assert ((gs[:, 0, :, 0] != 0).sum(axis=1) <= 5).all()
    used = gs[:, 0, :, 0] != 0
    assert (gs[:, 0, :, 1:].sum(axis=2)[used] >= 2).all()  # every row: at least two feet in stance
    # the step that enters the horizon at tick t is the last step of the table after it; every
    # swing of every foot lasts 7 steps
    steps = []
    for t in range(120):
        last = int(np.flatnonzero(gs[t, 0, :, 0])[-1])
        steps.append(gs[t, 0, last, 1:])
    steps = np.array(steps)
    for foot in range(4):
        runs, n = [], 0
        for v in steps[:, foot]:
            if v == 0:
                n += 1
            elif n:
                runs.append(n)
                n = 0
        assert runs and set(runs) == {7}, (foot, runs)


def test_closed_loop_on_the_oracle(oracle):
    """The schedule in closed loop (gait_cases.closed_loop: the oracle's planner passes, the
    model's roll, formulate / qp_solve / retrieve as oracle.Session.tick): the tables and rows
    are the open-loop model's, the robot that never requests is a plain oracle.Session, and the
    statuses are recorded for the GPU test (which asserts equality with them, not SOLVED)."""
    rec = GC.closed_loop()
    B = rec["status"].shape[1]
    gs, ss = GC.model_run(np.stack([GC.table("trot", 16)] * B), LIB3, P3, GC.SCHEDULE_TICKS, GC.requests(B, never=4))
    assert np.array_equal(rec["gait"], gs) and np.array_equal(rec["state"], ss)
    plain = oracle.Session(16, GC.table("trot", 16))
    for k in range(GC.SCHEDULE_TICKS):
        plain.tick(k, GC.CLOSED_V_REF)
        assert plain.status == rec["status"][k, 4] and plain.iters == rec["iters"][k, 4]
        assert np.array_equal(plain.x, rec["x"][k, 4])
    assert (ss[-1, :4, 3] >= 3).all() and ss[-1, 4, 3] == 0
    vals, counts = np.unique(rec["status"], return_counts=True)
    print("closed-loop oracle statuses:", dict(zip(vals.tolist(), counts.tolist())), "max iters", rec["iters"].max())
    assert (rec["status"] == 1).all()  # the oracle solves every tick of the schedule
