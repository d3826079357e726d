"""GPU: session snapshots -- the gather kernel alone against numpy's fancy indexing, and what
save / restore / fork / export / import promise on sessions with everything enabled.

Every comparison is bit equality (monitor_model.same: NaN equals NaN).  MPCQ_SV_ORDER is
compared as "is a permutation" only: it is rebuilt after a restore, its order inside a bucket of
16 iterations is left to LDS atomics by design, and results do not depend on it."""
import ctypes as C

import numpy as np
import pytest

import scenario_cases as SC
import scenario_model as SM
import swing_param_cases as WC
from monitor_model import same

pytestmark = pytest.mark.gpu

SV = ("SV_F0", "SV_X", "SV_X_ROBOT", "SV_Q_W", "SV_COST", "SV_XREF", "SV_FSTEPS", "SV_GAIT", "SV_STATUS", "SV_ITERS",
      "SV_RHO", "SV_Y", "SV_STATE", "SV_L_FEET", "SV_ROT_FLAG", "SV_H_ROT", "SV_ORDER", "SV_FIRST")
SWING = ("SV_SWING_REF", "SV_SWING_STATE", "SV_FRAME")
PV = ("PV_STATE_END", "PV_F_EFF", "PV_WRENCH")
MV = ("MV_DONE", "MV_EP", "MV_EP_TICKS", "MV_EPISODES", "MV_LAST", "MV_TOTALS")
CV = ("CV_EPOCH", "CV_TICK", "CV_V_REF", "CV_PUSH", "CV_WRENCH", "CV_ROBOTS", "CV_DRAW")
TABLES = ("robots",)  # Session.get_robots: the model's table
MON = dict(max_ticks=5, auto_reset=1)  # every episode ends after ticks 4 and 9: inside the windows below
PUSHED = (1, 2, 7)  # the robots with a wrench of the user's
POISON = 0xA5


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


@pytest.fixture(scope="module")
def eng(mpcq):
    with mpcq.Engine(16) as e:
        yield e


# ------------------------------------------------------------------------------- the kernel alone
ROW_BYTES = (4, 8, 12, 16, 48, 104, 800, 3072, 5632)
GUARD = 512  # poisoned bytes behind every destination
# device arrays start this many bytes into a 256-byte aligned allocation: 16-, 8- and 4-byte accesses
SHIFT = {48: 8, 800: 4, 12: 4, 8: 8}


def _maps(rows_src, rows_dst, rng):
    quarter = rng.integers(0, rows_src, rows_dst).astype(np.int32)
    quarter[rng.random(rows_dst) < 0.25] = -1
    quarter[0] = -1
    return {"identity": None,
            "one row": np.full(rows_dst, rows_src - 1, np.int32),
            "random": rng.integers(0, rows_src, rows_dst).astype(np.int32),
            "quarter -1": quarter}


def _expected(src, dst0, m, rows_src, rows_dst):
    """numpy's fancy indexing; an entry outside [0, rows_src) leaves the row alone."""
    m = np.arange(rows_dst, dtype=np.int64) if m is None else m.astype(np.int64)
    ok = (m >= 0) & (m < rows_src)
    out = []
    for s, d in zip(src, dst0):
        e = d.copy()
        e[:rows_dst][ok] = s[m[ok]]
        out.append(e)
    return out


def _gather(mpcq, eng, src_ptrs, dst_ptrs, rows_src, rows_dst, map_ptr, flags):
    n = len(ROW_BYTES)
    eng._call("mpcq_debug_gather_rows", eng._h, n, (C.c_void_p * n)(*src_ptrs), (C.c_void_p * n)(*dst_ptrs),
              (C.c_int64 * n)(*ROW_BYTES), rows_src, rows_dst, C.c_void_p(map_ptr) if map_ptr else None, flags)


@pytest.mark.parametrize("rows_src", [1, 65])
@pytest.mark.parametrize("rows_dst", [1, 63, 64, 65, 130])
def test_gather_rows_vs_fancy_indexing(mpcq, eng, rows_dst, rows_src):
    import torch
    rng = np.random.default_rng(1000 * rows_dst + rows_src)
    src = [rng.integers(0, 256, (rows_src, rb), dtype=np.uint8) for rb in ROW_BYTES]
    # the guard region: whole rows behind the rows_dst the call may write
    dst0 = [np.full((rows_dst + -(-GUARD // rb), rb), POISON, np.uint8) for rb in ROW_BYTES]
    maps = _maps(rows_src, rows_dst, rng)
    bad = maps["quarter -1"].copy()  # what only a device map may hold: all must act as -1
    bad[0::3] = np.resize(np.array([rows_src, np.iinfo(np.int32).max, -7], np.int32), bad[0::3].shape)
    maps["device only"] = bad

    def dev(a, shift=0):
        t = torch.full((shift + a.size,), 0, dtype=torch.uint8, device="cuda")
        t[shift:] = torch.from_numpy(a.reshape(-1))
        return t

    d_src = [dev(s, SHIFT.get(rb, 0)) for s, rb in zip(src, ROW_BYTES)]
    for name, m in maps.items():
        want = _expected(src, dst0, m, rows_src, rows_dst)
        ctx = (rows_dst, rows_src, name)
        if name != "device only":  # host pointers
            got = [d.copy() for d in dst0]
            _gather(mpcq, eng, [s.ctypes.data for s in src], [g.ctypes.data for g in got], rows_src, rows_dst,
                    0 if m is None else m.ctypes.data, 0)
            for g, w, rb in zip(got, want, ROW_BYTES):
                assert np.array_equal(g, w), (ctx, "host", rb)
        # device pointers: the same bytes, and the guards behind every array still poisoned
        d_dst = [dev(d, SHIFT.get(rb, 0)) for d, rb in zip(dst0, ROW_BYTES)]
        d_map = None if m is None else torch.from_numpy(m).to("cuda")
        torch.cuda.synchronize()
        _gather(mpcq, eng, [t.data_ptr() + SHIFT.get(rb, 0) for t, rb in zip(d_src, ROW_BYTES)],
                [t.data_ptr() + SHIFT.get(rb, 0) for t, rb in zip(d_dst, ROW_BYTES)], rows_src, rows_dst,
                0 if d_map is None else d_map.data_ptr(), mpcq.FLAG_DEVICE_PTRS)
        for t, w, rb in zip(d_dst, want, ROW_BYTES):
            g = t.cpu().numpy()
            assert not g[:SHIFT.get(rb, 0)].any(), (ctx, "before the array", rb)
            assert np.array_equal(g[SHIFT.get(rb, 0):].reshape(w.shape), w), (ctx, "device", rb)


# ------------------------------------------------------------------------------- sessions
def _names(sess, scenario=True):
    return SV + SWING + PV + MV + (CV if scenario else ()) + TABLES


def _read(mpcq, sess, names):
    out = {}
    for n in names:
        if n == "robots":
            out[n] = sess.get_robots()
            continue
        read = sess.read if n.startswith("SV") else sess.plant_read if n.startswith("PV") else \
            sess.monitor_read if n.startswith("MV") else sess.scenario_read
        out[n] = read(getattr(mpcq, n))
    return out


def _eq(a, b):
    if a.dtype.names:
        return a.shape == b.shape and all(same(np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])) for f in a.dtype.names)
    return same(a, b)


def _check(a, b, ctx, rows_a=None, rows_b=None, skip=()):
    """Every array of two reads equal (rows_a of a against rows_b of b where given; the batch-wide
    MV_TOTALS is then left out); SV_ORDER: a permutation on both sides."""
    for n in a:
        if n in skip:
            continue
        if n == "SV_ORDER":
            for o in (a[n], b[n]):
                assert np.array_equal(np.sort(o), np.arange(o.shape[0])), (ctx, n)
            continue
        x, y = a[n], b[n]
        if rows_a is not None or rows_b is not None:
            if n == "MV_TOTALS":
                continue
            x = x if rows_a is None else x[rows_a]
            y = y if rows_b is None else y[rows_b]
        assert _eq(np.ascontiguousarray(x), np.ascontiguousarray(y)), (ctx, n)


def _v_ref(B, seed=41):
    return WC.session_v_ref(B, seed)


def _wrench(B):
    w = np.zeros((B, 6))
    w[PUSHED[0]] = [5.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    w[PUSHED[1]] = [0.0, -4.0, 0.0, 0.0, 0.0, 0.2]
    w[PUSHED[2] % B] = [-3.0, 2.0, 1.0, 0.0, 0.1, 0.0]
    return w


def _tables(mpcq, B):
    rng = np.random.default_rng(77)
    return (mpcq.robots(B, mass=rng.uniform(2.3, 2.7, B), mu=rng.uniform(0.7, 1.0, B)),
            mpcq.robots(B, mass=rng.uniform(2.2, 2.9, B), mu=rng.uniform(0.6, 1.0, B)))


def _open(mpcq, eng, B, scenario=True, monitor=True, tables=True, k_mpc=None, gaits=None):
    """A session with everything enabled: mixed trot / bound / pace, swing, the rigid plant with a
    table of its own and wrenches on three robots, the monitor with auto-reset and a tick limit of
    5, the small scenario (commands, pushes, robots), a model table."""
    N, dt = eng.n_steps, eng.params.dt
    sess = mpcq.Session(eng, B, gait0=WC.session_gaits(N, B) if gaits is None else gaits,
                        planner_params=mpcq.default_planner_params(dt=dt))
    sess.enable_swing(None if k_mpc is None else mpcq.default_swing_params(k_mpc=k_mpc))
    sess.enable_plant()
    sess.set_wrench(_wrench(B))
    if tables:
        model, plant = _tables(mpcq, B)
        sess.set_robots(model)
        sess.set_plant_robots(plant)
    if monitor:
        sess.enable_monitor(**MON)
    if scenario:
        sess.enable_scenario(**SC.SMALL)
    return sess


def _ticks(mpcq, sess, n, v=None, names=None, out=None):
    for _ in range(n):
        sess.tick(v)
        if out is not None:
            out.append(_read(mpcq, sess, names))
    return out


def _continuation(mpcq, eng, B, k_mpc=None, blob=False):
    """Tick 6, save, tick 6 more reading everything, restore, tick the same 6: the reads."""
    with _open(mpcq, eng, B, k_mpc=k_mpc) as sess:
        names = _names(sess)
        _ticks(mpcq, sess, 6)
        with sess.snapshot() as snap:
            saved = _read(mpcq, sess, names)
            data = snap.tobytes() if blob else None
            first = _ticks(mpcq, sess, 6, names=names, out=[])
            assert sess.k == 12
            sess.restore(snap)
            assert sess.k == 6
            _check(_read(mpcq, sess, names), saved, "restored")
            second = _ticks(mpcq, sess, 6, names=names, out=[])
    for k, (a, b) in enumerate(zip(first, second)):
        _check(b, a, ("tick", 6 + k))
    # the window saw episodes end and restart, pushes and more than one status of the order
    assert first[-1]["MV_EPISODES"].min() >= 2 and first[-1]["MV_TOTALS"][1] > saved["MV_TOTALS"][1]
    assert any(r["CV_PUSH"].any() for r in first)
    return saved, first, data


@pytest.fixture(scope="module")
def cont16(mpcq, eng):
    return _continuation(mpcq, eng, 65, blob=True)


def test_continuation_n16(cont16):
    assert len(cont16[1]) == 6


def test_continuation_n32(mpcq):
    with mpcq.Engine(32) as e:
        _continuation(mpcq, e, 17)


def test_continuation_n8_k_mpc_7(mpcq):
    with mpcq.Engine(8, dt=0.04) as e:  # swing rows of 7 x 36 doubles: the `all` case's stride
        saved, _, _ = _continuation(mpcq, e, 17, k_mpc=7)
        assert saved["SV_SWING_REF"].shape == (17, 7, 4, 9)


def test_branch(mpcq, eng):
    """fork(r): every slot continues as robot r does in an untouched twin; a wrench on half of the
    branches then moves those and only those."""
    B, r = 65, 4  # r paces, its neighbours trot and bound
    v0, v1 = _v_ref(B), np.array([0.4, 0.05, 0.0, 0.0, 0.0, 0.2])
    with _open(mpcq, eng, B, scenario=False) as a, _open(mpcq, eng, B, scenario=False) as twin:
        names = _names(a, scenario=False)
        g = a.read(mpcq.SV_GAIT)
        assert not same(g[r], g[r - 1]) and not same(g[r], g[r + 1])
        for s in (a, twin):
            _ticks(mpcq, s, 6, v0)
        a.fork(r)
        assert a.k == 6
        _check(_read(mpcq, a, names), _read(mpcq, twin, names), "forked", rows_b=[r] * B)
        for k in range(6):
            a.tick(v1)
            twin.tick(v1)
            _check(_read(mpcq, a, names), _read(mpcq, twin, names), ("tick", 6 + k), rows_b=[r] * B)
        w = np.tile(twin.plant_read(mpcq.PV_WRENCH)[r], (B, 1))
        half = np.arange(B) % 2 == 0
        w[half] += [6.0, -3.0, 0.0, 0.0, 0.0, 0.1]
        a.set_wrench(w)
        a.tick(v1)
        twin.tick(v1)
        end, ref = a.plant_read(mpcq.PV_STATE_END), twin.plant_read(mpcq.PV_STATE_END)[r]
        assert np.isfinite(ref).all()
        assert all(not same(end[b], ref) for b in np.flatnonzero(half))
        assert all(same(end[b], ref) for b in np.flatnonzero(~half))
        others = tuple(n for n in names if n != "PV_WRENCH")
        _check({n: x for n, x in _read(mpcq, a, others).items()}, _read(mpcq, twin, others), "unpushed",
               rows_a=np.flatnonzero(~half), rows_b=[r] * int((~half).sum()))


def test_selective_restore(mpcq, eng):
    B = 65
    odd = np.arange(B) % 2 == 1
    m = np.full(B, -1, np.int32)
    even = np.flatnonzero(~odd)
    m[even] = np.random.default_rng(5).permutation(even)
    with _open(mpcq, eng, B) as a, _open(mpcq, eng, B) as twin:
        names = _names(a)
        for s in (a, twin):
            _ticks(mpcq, s, 6)
        with a.snapshot() as snap:
            saved = _read(mpcq, a, names)
            for s in (a, twin):
                _ticks(mpcq, s, 2)
            before = _read(mpcq, a, names)
            a.restore(snap, m)
            assert a.k == 8
            now, ref = _read(mpcq, a, names), _read(mpcq, twin, names)
            _check(now, ref, "odd: untouched", rows_a=odd, rows_b=odd)
            _check(now, saved, "even: their rows of the snapshot", rows_a=even, rows_b=m[even])
            # a mapped restore leaves the batch-wide totals alone
            assert same(now["MV_TOTALS"], before["MV_TOTALS"]) and not same(now["MV_TOTALS"], saved["MV_TOTALS"])
            for k in range(4):
                a.tick(None)
                twin.tick(None)
                _check(_read(mpcq, a, names), _read(mpcq, twin, names), ("odd", 8 + k), rows_a=odd, rows_b=odd)
            a.restore(snap)  # the identity: the totals too
            assert a.k == 6
            _check(_read(mpcq, a, names), saved, "all of it")


def test_snapshot_from_before_the_first_tick_is_a_pending_reset(mpcq, eng):
    B = 65
    third = np.arange(B) % 3 == 0
    v = _v_ref(B)
    names = SV + SWING
    with _open(mpcq, eng, B, scenario=False) as a, _open(mpcq, eng, B, scenario=False) as twin:
        with a.snapshot() as snap:
            for s in (a, twin):
                _ticks(mpcq, s, 6, v)
            a.restore(snap, np.where(third, np.arange(B), -1))
            twin.reset(mask=third)
            assert a.k == 6
            assert np.array_equal(a.read(mpcq.SV_FIRST), third.astype(np.int32))
            _check(_read(mpcq, a, names), _read(mpcq, twin, names), "restored")
            for k in range(4):
                a.tick(v)
                twin.tick(v)
                _check(_read(mpcq, a, names), _read(mpcq, twin, names), ("tick", 6 + k))
                # served by the first tick after it (the tick limit marks the other robots at tick 9)
                assert not a.read(mpcq.SV_FIRST)[third].any()


def test_seeding_across_batch_sizes(mpcq, eng):
    B, v3 = 65, _v_ref(3, seed=9)
    m = np.arange(B, dtype=np.int32) % 3
    kw = dict(scenario=False, tables=False)
    with _open(mpcq, eng, 3, **kw) as small, _open(mpcq, eng, B, gaits=WC.session_gaits(16, B)[::-1].copy(), **kw) as big:
        names = tuple(n for n in _names(small, scenario=False) if n != "robots")
        _ticks(mpcq, small, 8, v3)
        with small.snapshot() as snap:
            untouched = _read(mpcq, big, SV)
            bad = m.copy()
            bad[40] = -1
            with pytest.raises(mpcq.MpcqError, match=r"map\[40\]") as err:
                big.restore(snap, bad)  # the robot left out would run a warm tick on creation state
            assert err.value.code == mpcq._lib.E_INVALID and big.k == 0
            _check(_read(mpcq, big, SV), untouched, "refused")
            big.restore(snap, m)
            assert big.k == 8  # the session had not ticked: the snapshot's tick index
            _check(_read(mpcq, big, names), _read(mpcq, small, names), "seeded", rows_b=m)
            for k in range(4):
                small.tick(v3)
                big.tick(v3[m])
                _check(_read(mpcq, big, names), _read(mpcq, small, names), ("tick", 8 + k), rows_b=m)


def test_scenario_branches_diverge_as_specified(mpcq, eng):
    B, r = 65, 7
    p = SM.params(**SC.SMALL)
    with _open(mpcq, eng, B) as a:
        _ticks(mpcq, a, 6)
        at_save = _read(mpcq, a, CV + PV)
        plant_row = _tables(mpcq, B)[1][r]
        a.fork(r)
        cv = _read(mpcq, a, CV)
        for n in ("CV_EPOCH", "CV_TICK", "CV_ROBOTS", "CV_DRAW"):
            assert _eq(cv[n], np.ascontiguousarray(at_save[n][[r] * B])), n
        st = dict(epoch=cv["CV_EPOCH"].copy(), tick=cv["CV_TICK"].copy(), robots=cv["CV_ROBOTS"].copy(),
                  draw=cv["CV_DRAW"].copy())
        base = np.ascontiguousarray(np.broadcast_to(plant_row, (B,)))  # every slot holds r's row of the table
        user = np.tile(at_save["PV_WRENCH"][r], (B, 1))
        spread = 0
        for k in range(6):  # slot b draws (seed, b, the inherited epoch, tau) from the next tick on
            first = a.read(mpcq.SV_FIRST)
            v, pu, wo, _ = SM.step(p, st, first, False, base, user)
            a.tick(None)
            cv = _read(mpcq, a, CV)
            assert same(cv["CV_V_REF"], v) and same(cv["CV_PUSH"], pu) and same(cv["CV_WRENCH"], wo), k
            assert same(cv["CV_EPOCH"], st["epoch"]) and same(cv["CV_TICK"], st["tick"]), k
            spread += len(np.unique(cv["CV_V_REF"], axis=0)) > B // 2
        assert spread > 0  # different futures from one state
        assert len(np.unique(a.read(mpcq.SV_Q_W), axis=0)) > B // 2


def test_device_map(mpcq, eng):
    import torch
    B = 65
    rng = np.random.default_rng(3)
    m = rng.integers(0, B, B).astype(np.int32)
    m[rng.random(B) < 0.25] = -1
    v = _v_ref(B)
    d_m, d_v = torch.from_numpy(m).to("cuda"), torch.from_numpy(v).to("cuda")
    torch.cuda.synchronize()
    with _open(mpcq, eng, B, scenario=False) as a, _open(mpcq, eng, B, scenario=False) as b:
        names = _names(a, scenario=False)
        for s in (a, b):
            _ticks(mpcq, s, 6, v)
        with a.snapshot() as sa, b.snapshot() as sb:
            for s in (a, b):
                _ticks(mpcq, s, 2, v)
            a.restore(sa, m)
            b.restore_device(sb, d_m.data_ptr(), asynchronous=True)
            _check(_read(mpcq, b, names), _read(mpcq, a, names), "async device map")
            # enqueued between two rollouts, nothing synchronised in between
            a.run(v, 3)
            a.restore(sa, m)
            a.run(v, 3)
            b.run_device(d_v.data_ptr(), 3)
            b.restore_device(sb, d_m.data_ptr())
            b.run_device(d_v.data_ptr(), 3)
            assert a.k == b.k == 14
            _check(_read(mpcq, b, names), _read(mpcq, a, names), "between two run_device calls")
            a.fork(m)
            b.fork_device(d_m.data_ptr())
            _check(_read(mpcq, b, names), _read(mpcq, a, names), "fork")


def test_export_import(mpcq, eng, cont16):
    saved, first, blob = cont16
    with _open(mpcq, eng, 65) as fresh:
        names = _names(fresh)
        untouched = _read(mpcq, fresh, names)
        magic = bytearray(blob)
        magic[3] ^= 0x20
        for what, data in (("truncated", blob[:-1]), ("magic", bytes(magic)), ("longer", blob + b"\0")):
            with pytest.raises(mpcq.MpcqError) as err:
                fresh.snapshot_from(data)
            assert err.value.code == mpcq._lib.E_INVALID, what
            _check(_read(mpcq, fresh, names), untouched, what)
        with mpcq.Engine(32) as other, mpcq.Session(other, 3) as s32:
            with pytest.raises(mpcq.MpcqError, match="N = 16") as err:
                s32.snapshot_from(blob)
            assert err.value.code == mpcq._lib.E_INVALID
        with fresh.snapshot_from(blob) as snap:
            assert snap.k == 6 and snap.batch == 65 and snap.nbytes() == len(blob) and snap.tobytes() == blob
            fresh.restore(snap)
        assert fresh.k == 6
        _check(_read(mpcq, fresh, names), saved, "imported")
        second = _ticks(mpcq, fresh, 6, names=names, out=[])
    for k, (a, b) in enumerate(zip(first, second)):
        _check(b, a, ("tick", 6 + k))


def test_refusals_leave_the_session_as_it_was(mpcq, eng):
    B = 17
    names = SV + SWING
    v = _v_ref(B)

    def refused(sess, call, match):
        before = _read(mpcq, sess, names)
        k = sess.k
        with pytest.raises(mpcq.MpcqError, match=match) as err:
            call()
        assert err.value.code == mpcq._lib.E_INVALID
        assert sess.k == k
        _check(_read(mpcq, sess, names), before, match)

    kw = dict(scenario=False, monitor=False)
    with _open(mpcq, eng, B, **kw) as a, _open(mpcq, eng, B, k_mpc=7, **kw) as other_k, \
            _open(mpcq, eng, B + 1, **kw) as bigger, mpcq.Engine(16) as eng2, _open(mpcq, eng2, B, **kw) as elsewhere:
        for s in (a, other_k, bigger, elsewhere):
            _ticks(mpcq, s, 3, _v_ref(s.batch))
        with a.snapshot() as snap:
            refused(other_k, lambda: other_k.restore(snap), "k_mpc")  # another swing k_mpc
            refused(elsewhere, lambda: elsewhere.restore(snap), "another context")  # another engine
            refused(bigger, lambda: bigger.restore(snap), "batch")  # map = None with differing B
            bad = np.arange(B, dtype=np.int32)
            bad[11] = B  # B_snapshot itself
            refused(a, lambda: a.restore(snap, bad), r"map\[11\]")
            refused(a, lambda: a.fork(bad), r"map\[11\]")
            a.set_plant_robots(None)  # a table cleared after the save
            refused(a, lambda: a.restore(snap), "plant robots table")
            a.set_plant_robots(_tables(mpcq, B)[1])
            a.restore(snap)
            a.enable_monitor(**MON)  # the monitor enabled after the save
            refused(a, lambda: a.restore(snap), "monitor")
            snap.save()  # saving again re-captures with the monitor: the restore goes through
            _ticks(mpcq, a, 2, v)
            a.restore(snap)
            assert a.k == 3 and not a.monitor_read(mpcq.MV_EP_TICKS).any()
        empty = mpcq.Snapshot(a)
        refused(a, lambda: a.restore(empty), "save")
        empty.close()
