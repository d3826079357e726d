"""GPU: the dispatch-order kernels against the host model (dispatch_model.py).

test_gpu_order.py / test_gpu_slice.py show that the class order, the sliced solves and the
session order change no result -- which any permutation does, the identity included.  The
gains they were built for rest on the kernels producing the order their comments describe,
so here every kernel runs alone (mpcq_debug_*, microseconds each) and must equal the model:
the class slots, the whole class-order permutation (the sort is stable), the learned table,
the suspended list; of the session's order everything but the order inside a bucket.  Then the
wiring, on real solves at small shapes: what a solve with the class order / a sliced solve
actually dispatched by (mpcq_debug_last_dispatch) is what the model derives from the table
and the returned iteration counts."""
import numpy as np
import pytest

import dispatch_model as M

pytestmark = pytest.mark.gpu

# the wave (64), workgroup (1024 = one chunk of the order kernels' loop) and chunk edges
ORDER_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 4100)


@pytest.fixture(scope="module")
def eng():
    import mpcq
    with mpcq.Engine(16) as e:
        yield e


@pytest.fixture(scope="module")
def slot_batch():
    """The hand-built tables (dispatch_model.slot_cases), each a few times in a seeded shuffle
    over two blocks of class_kernel: (names, fsteps, model slots)."""
    cases = M.slot_cases()
    rng = np.random.default_rng(5)
    pick = np.concatenate([np.arange(len(cases)), rng.integers(0, len(cases), 300 - len(cases))])
    rng.shuffle(pick)
    fsteps = np.stack([cases[i][1] for i in pick])
    want = np.array([0 if cases[i][2] is None else cases[i][2] % M.SLOTS for i in pick], np.int32)
    return [cases[i][0] for i in pick], fsteps, want


def _zero_table():
    return np.zeros(M.SLOTS, np.uint64), np.zeros(M.SLOTS, np.uint64)


# ------------------------------------------------------------------ class slots
def test_class_slots_equal_the_model(eng, slot_batch):
    names, fsteps, want = slot_batch
    assert np.array_equal(M.class_slots(fsteps), want)   # (the model on its hand-worked bitmaps)
    eng.set_class_table(*_zero_table())
    cls, order = eng.class_order(fsteps)
    bad = np.flatnonzero(cls != want)
    assert bad.size == 0, [(names[i], int(cls[i]), int(want[i])) for i in bad[:8]]
    assert np.array_equal(order, np.arange(len(want)))   # an all-zero table: the identity
    # two different gaits, one slot (the collision the table lives with)
    ia, ib = names.index("coll-a1"), names.index("coll-a2")
    assert cls[ia] == cls[ib] == 1 and not np.array_equal(fsteps[ia], fsteps[ib], equal_nan=True)


def test_class_slots_of_the_synthetic_gaits(eng):
    from mpcq import synth
    syn = synth.make_batch(90, 16, gaits=synth.GAITS, seed=4)
    cls, _ = eng.class_order(syn["fsteps"])
    assert np.array_equal(cls, np.array([212, 226, 190], np.int32)[syn["gait"]])


# ------------------------------------------------------------------ class order
# The classes of the order test, from the hand-built set (a single mask m lands in slot 2^m mod
# 251); their slots are computed by the model.  The first ten have ten different slots (the
# tables below address them); "odd" shares mask4's slot, the coll-a pair and term0 / noterm
# share theirs.
def _palette():
    names = ("mask1", "mask2", "mask3", "mask4", "mask5", "mask6", "mask7", "mask9", "mask12", "trot",
             "all15", "term0", "coll-a1", "coll-a2", "noterm", "flying", "odd")
    cases = {n: fs for n, fs, _ in M.slot_cases()}
    fs = np.stack([cases[n] for n in names])
    return names, fs, M.class_slots(fs)


def _tables(slots):
    """Named class tables written through the hook, over the palette's slots ``slots``."""
    out = {}
    out["zero"] = _zero_table()
    s, n = _zero_table()
    # slots[0..3]: adjacent means on either side of multiples of 16 (15 | 16, 31 | 32)
    s[slots[0]], n[slots[0]] = 159, 10        # 15.9 -> 15 -> bucket 0
    s[slots[1]], n[slots[1]] = 160, 10        # 16   -> bucket 1
    s[slots[2]], n[slots[2]] = 31 * 7 + 6, 7  # 31   -> bucket 1
    s[slots[3]], n[slots[3]] = 32 * 7, 7      # 32   -> bucket 2
    s[slots[4]], n[slots[4]] = 4080 * 3, 3    # 4080 -> bucket 255, unclamped
    s[slots[5]], n[slots[5]] = 4079 * 3 + 2, 3  # 4079 -> bucket 254
    s[slots[6]], n[slots[6]] = 10 ** 7, 2     # clamps to 255
    s[slots[7]], n[slots[7]] = 886 * 40000, 40000
    s[slots[8]], n[slots[8]] = 600 * 123 + 5, 123
    # slots[9..]: unseen (cnt 0, one with a stale sum): the mean over the seen slots; two seen
    # slots outside the palette pull that mean
    s[slots[9]] = 777
    for extra, (a, c) in ((249, (300 * 9, 9)), (100, (2000 * 50, 50))):
        assert extra not in slots
        s[extra], n[extra] = a, c
    out["mixed"] = (s, n)
    s, n = _zero_table()   # the mean itself clamps: every unseen class in bucket 255 too
    s[slots[0]], n[slots[0]] = 50, 1
    s[slots[1]], n[slots[1]] = 10 ** 12, 3
    out["mean-clamps"] = (s, n)
    s, n = _zero_table()   # one seen slot only: every class in its bucket or the mean's (the same)
    s[slots[2]], n[slots[2]] = 640, 1
    out["one-seen"] = (s, n)
    return out


def test_class_order_equals_the_model(eng):
    names, pal, slots = _palette()
    assert len(set(slots[:10].tolist())) == 10 and len(set(slots.tolist())) == 14
    assert slots[names.index("coll-a1")] == slots[names.index("coll-a2")] and slots[names.index("odd")] == slots[3]
    tables = _tables(slots.tolist())
    costs = M.class_costs(*tables["mixed"])
    assert len({costs[c] for c in slots}) >= 7 and costs[slots[9]] == costs[slots[10]]  # unseen: one bucket
    rng = np.random.default_rng(9)
    for B in ORDER_SIZES:
        pick = rng.integers(0, len(pal), B)
        fsteps = pal[pick]
        for tname, (s, n) in tables.items():
            eng.set_class_table(s, n)
            cls, order = eng.class_order(fsteps)
            assert np.array_equal(cls, slots[pick]), (B, tname)
            want = M.class_order(cls, s, n)
            assert np.array_equal(order, want), (B, tname, np.flatnonzero(order != want)[:5])
            if tname == "zero":
                assert np.array_equal(order, np.arange(B))
            rs, rn = eng.class_table()   # the order reads the table only
            assert np.array_equal(rs, s) and np.array_equal(rn, n)


# ------------------------------------------------------------------ class learn
def test_class_learn_equals_the_model(eng):
    rng = np.random.default_rng(3)
    s, n = _zero_table()
    s[7], n[7] = 12345, 20
    s[250], n[250] = 2 ** 40, 2 ** 33   # beyond 32 bits both
    for B in (1, 256, 257, 700, 2100):   # 256-thread blocks: one, an edge, several
        cls = rng.integers(0, M.SLOTS, B).astype(np.int32)
        cls[rng.integers(0, B, B // 3)] = 7   # a crowded slot
        iters = rng.integers(1, 4001, B).astype(np.int32)
        iters[rng.integers(0, B, B // 5)] = 0          # not counted
        iters[rng.integers(0, B, B // 7)] = -3
        if B > 1:
            cls[0], iters[0] = 0, 25
            cls[1], iters[1] = M.SLOTS - 1, -1
        eng.set_class_table(s, n)
        eng.class_learn(cls, iters)
        ws, wn = M.class_learn(s, n, cls, iters)
        gs, gn = eng.class_table()
        assert np.array_equal(gs, ws) and np.array_equal(gn, wn), B
        s, n = ws, wn   # the next size accumulates on top
    import mpcq
    with pytest.raises(mpcq.MpcqError):
        eng.class_learn(np.array([M.SLOTS], np.int32), np.array([5], np.int32))


def test_class_count_survives_2_pow_32(eng):
    """A slot that has counted just under 2^32 instances of 600 iterations learns 64 more: its
    cost stays in (or next to) bucket 600 >> 4.  A 32-bit count wraps to 32 here, the mean
    becomes sum / 32 and the class is pinned to bucket 255, ahead of every other."""
    cases = {name: fs for name, fs, _ in M.slot_cases()}
    a, b = M.class_slot(cases["mask3"]), M.class_slot(cases["mask5"])
    s, n = _zero_table()
    n[a] = 2 ** 32 - 32
    s[a] = 600 * int(n[a])
    s[b], n[b] = 1000 * 10, 10   # a dearer class: bucket 62
    eng.set_class_table(s, n)
    rng = np.random.default_rng(1)
    iters = rng.integers(590, 611, 64).astype(np.int32)
    eng.class_learn(np.full(64, a, np.int32), iters)
    gs, gn = eng.class_table()
    assert int(gn[a]) == 2 ** 32 + 32 and int(gs[a]) == int(s[a]) + int(iters.sum())
    cost = M.class_costs(gs, gn)
    assert abs(cost[a] - (600 >> 4)) <= 1
    # and the kernel's own reading of the table: the dearer class first
    fsteps = np.stack([cases["mask3"], cases["mask5"]] * 40)
    cls, order = eng.class_order(fsteps)
    assert np.array_equal(order, M.class_order(cls, gs, gn))
    assert (cls[order[:40]] == b).all() and (cls[order[40:]] == a).all()


# ------------------------------------------------------------------ suspended list
def _sus_case(n, seed, frac):
    """status (n,) mixing the suspended code with others (frac: share suspended; 0 / 1: none /
    all), key (n,2) with the special values (element 1 is not the key: garbage)."""
    import mpcq
    code = mpcq.Engine.suspended_status()
    rng = np.random.default_rng(seed)
    others = np.array([1, 2, -2, -3, 0, 3, -10, code + 1, code - 1, -code], np.int32)
    status = others[rng.integers(0, len(others), n)]
    status[rng.random(n) < frac] = code
    key = np.empty((n, 2))
    key[:, 0] = M.suspended_keys(n, seed)
    key[:, 1] = rng.permutation(key[:, 0]) * 0.5
    return code, status, key


@pytest.mark.parametrize("n", [1, 64, 65, 1024, 1025, 3000])
def test_suspended_list_equals_the_model(eng, n):
    assert eng.suspended_status() == 100
    for frac in (0.6, 0.0, 1.0, 0.03):
        code, status, key = _sus_case(n, n + int(100 * frac), frac)
        M.check_key_edges(key[:, 0])
        rng = np.random.default_rng(n)
        for prev in (None, rng.permutation(n).astype(np.int32)):
            got, count = eng.suspended_list(prev, n, status, key)
            want = M.suspended_list(prev, n, status, key, code)
            tag = (n, frac, prev is None)
            assert count == len(want) == int((status == code).sum()), tag
            assert np.array_equal(got, want), (tag, np.flatnonzero(got != want)[:5])
    # prev a part of the instances only (n of 2 n, not all of them in it)
    code, status, key = _sus_case(2 * n, 7 * n + 1, 0.5)
    prev = np.random.default_rng(n + 1).permutation(2 * n)[:n].astype(np.int32)
    got, count = eng.suspended_list(prev, n, status, key)
    assert np.array_equal(got, M.suspended_list(prev, n, status, key, code))
    import mpcq
    with pytest.raises(mpcq.MpcqError):   # an index past the status array is refused on the host
        eng.suspended_list(np.full(n, 2 * n, np.int32), n, status, key)


# ------------------------------------------------------------------ session order
@pytest.mark.parametrize("B", [1, 1024, 1025, 2600])
def test_session_order_buckets(eng, B):
    rng = np.random.default_rng(B)
    pool = np.array([-2 ** 31, -5, -1, 0, 1, 15, 16, 17, 31, 32, 400, 401, 886, 4079, 4080, 4081, 5000, 10 ** 6,
                     2 ** 31 - 1], np.int64)
    iters = np.where(rng.random(B) < 0.5, pool[rng.integers(0, len(pool), B)], rng.integers(0, 4200, B)).astype(np.int32)
    if B == 1:
        iters[0] = 4080
    order = eng.session_order(iters)
    assert np.array_equal(np.sort(order), np.arange(B))   # a permutation
    bk = np.array([M.iters_bucket(v) for v in iters])
    along = bk[order]
    assert (np.diff(along) <= 0).all()                     # the longest bucket first
    for q in np.unique(bk):   # each bucket's members (their order inside it is arbitrary)
        assert np.array_equal(np.sort(order[along == q]), np.flatnonzero(bk == q)), q


# ------------------------------------------------------------------ wiring: the class order
def test_solve_dispatches_by_the_learned_table():
    import mpcq
    from mpcq import synth
    syn = synth.make_batch(192, 16, gaits=synth.GAITS, seed=7)
    slots = M.class_slots(syn["fsteps"])
    assert sorted(set(slots.tolist())) == [190, 212, 226]
    s, n = _zero_table()
    with mpcq.Engine(16) as e:
        for launch in range(3):
            r = e.solve(syn["xref"], syn["fsteps"], order_by_class=True)
            d = e.last_dispatch()
            assert d["batch"] == 192 and d["by_class"] and not d["sliced"] and d["count"] == 0
            assert np.array_equal(d["cls"], slots)
            want = M.class_order(slots, s, n)   # from the table as it stood before the launch
            assert np.array_equal(d["order"], want), launch
            if launch == 0:
                assert np.array_equal(want, np.arange(192))
            else:
                cost = M.class_costs(s, n)
                assert not np.array_equal(want, np.arange(192))
                dearest = max((190, 212, 226), key=lambda c: int(s[c]) // int(n[c]))
                assert cost[dearest] > min(cost[c] for c in (190, 212, 226))
                assert slots[d["order"][0]] == dearest
            s, n = M.class_learn(s, n, slots, r["iters"])
            gs, gn = e.class_table()
            assert np.array_equal(gs, s) and np.array_equal(gn, n), launch
        # a solve without the flag neither reads nor feeds the table
        e.solve(syn["xref"], syn["fsteps"])
        d = e.last_dispatch()
        assert not d["by_class"] and d["order"] is None
        gs, gn = e.class_table()
        assert np.array_equal(gs, s) and np.array_equal(gn, n)


# ------------------------------------------------------------------ wiring: sliced solves
@pytest.fixture(scope="module")
def trot20():
    """N = 20 (the smallest compiled horizon beyond 16), 300 trot instances, seed 2 (the batch
    of test_gpu_slice.py: iteration counts beyond 800) and its unsliced solve."""
    import mpcq
    from mpcq import synth
    syn = synth.make_batch(300, 20, gaits=("trot",), seed=2)
    with mpcq.Engine(20) as e:
        ref = e.solve(syn["xref"], syn["fsteps"])
        assert not e.last_dispatch()["sliced"]
    assert ref["iters"].max() > 800
    return syn, ref


def _check_sliced(e, syn, ref, q, by_class, want_key=None):
    r = e.solve(syn["xref"], syn["fsteps"], order_by_class=by_class)
    for k in ("f0", "status", "iters"):
        assert np.array_equal(r[k], ref[k], equal_nan=True), (q, k)
    d = e.last_dispatch()
    tag = (q, by_class)
    assert d["sliced"] and d["by_class"] == by_class and d["batch"] == 300, tag
    lst, iters = d["list"], r["iters"]
    assert d["count"] == len(lst) and len(set(lst.tolist())) == len(lst), tag   # no duplicates
    assert lst.min(initial=0) >= 0 and lst.max(initial=0) < 300
    assert (iters[lst] >= q).all(), tag   # a suspended instance ran the slice at least
    bound = M.suspend_bound(q)
    listed = np.zeros(300, bool)
    listed[lst] = True
    assert listed[iters > bound].all(), (tag, bound)   # every instance beyond the bound was suspended
    prev = d["order"] if by_class else np.arange(300, dtype=np.int32)
    if by_class:
        assert np.array_equal(np.sort(prev), np.arange(300))
    key = d["key"]
    bk = np.array([M.key_bucket(float(key[i, 0])) for i in lst])
    assert (np.diff(bk) <= 0).all(), tag   # the farthest from convergence first
    # inside a bucket the previous order; with the suspended set given, the model's whole list
    status = np.where(listed, e.suspended_status(), 1).astype(np.int32)
    want = M.suspended_list(prev, 300, status, key, e.suspended_status())
    assert np.array_equal(lst, want), (tag, np.flatnonzero(lst != want)[:5])
    if want_key is not None:
        assert (key[lst, 0] == want_key).all(), (tag, key[lst, 0][key[lst, 0] != want_key][:5])
        assert np.array_equal(lst, np.asarray(prev)[listed[prev]]), tag   # one bucket: prev's order
    return d


@pytest.mark.parametrize("q", [100, 333])
def test_sliced_solve_resumes_by_key(trot20, q):
    import mpcq
    syn, ref = trot20
    with mpcq.Engine(20) as e:
        e.set_slice(q)
        d = _check_sliced(e, syn, ref, q, False)
        assert d["count"] > 0
        if q == 333:   # a spread of keys for the sort to act on (at 100 the residuals of this batch
            # have not begun to decay between the sample and the suspension: every key 1e30)
            assert len({M.key_bucket(float(v)) for v in d["key"][d["list"], 0]}) > 3
    with mpcq.Engine(20) as e:   # with the class order, after one learning launch
        e.set_slice(q)
        e.solve(syn["xref"], syn["fsteps"], order_by_class=True)
        d = _check_sliced(e, syn, ref, q, True)
        assert np.array_equal(d["order"], np.arange(300))   # one class: the identity


def test_sliced_solve_mixed_classes_keeps_the_class_order_inside_a_bucket():
    """The same with a class order that is not the identity (trot / bound / pace)."""
    import mpcq
    from mpcq import synth
    syn = synth.make_batch(150, 20, gaits=synth.GAITS, seed=2)
    with mpcq.Engine(20) as e:
        ref = e.solve(syn["xref"], syn["fsteps"])
    with mpcq.Engine(20) as e:
        e.set_slice(100)
        e.solve(syn["xref"], syn["fsteps"], order_by_class=True)
        r = e.solve(syn["xref"], syn["fsteps"], order_by_class=True)
        d = e.last_dispatch()
        assert np.array_equal(r["iters"], ref["iters"]) and d["sliced"] and d["by_class"]
        assert not np.array_equal(d["order"], np.arange(150))
        listed = np.zeros(150, bool)
        listed[d["list"]] = True
        status = np.where(listed, e.suspended_status(), 1).astype(np.int32)
        assert np.array_equal(d["list"], M.suspended_list(d["order"], 150, status, d["key"], e.suspended_status()))
        assert listed[r["iters"] > M.suspend_bound(100)].all() and (r["iters"][d["list"]] >= 100).all()


def test_short_slice_falls_back_to_the_largest_key(trot20):
    """A slice shorter than half a check segment (7 of 25) suspends at the first segment end
    without a half-way sample of the residuals: every suspended instance's key is the documented
    fallback 1e30 ("as long as can be"), one bucket, so the list is the previous order restricted
    to the suspended set -- on a fresh context (whose scratch nobody has written) and on one
    whose earlier call, slice 333, left its own samples behind."""
    import mpcq
    syn, ref = trot20
    with mpcq.Engine(20) as e:
        e.set_slice(7)
        d = _check_sliced(e, syn, ref, 7, False, want_key=1e30)
        assert d["count"] == int((ref["iters"] > 25).sum()) > 200
    with mpcq.Engine(20) as e:
        e.set_slice(333)
        _check_sliced(e, syn, ref, 333, False)
        e.set_slice(7)
        _check_sliced(e, syn, ref, 7, False, want_key=1e30)
        _check_sliced(e, syn, ref, 7, True, want_key=1e30)


def test_short_slice_of_a_warm_solve_ignores_a_cold_call_s_samples(trot20):
    """The stale sample that does change a key: a cold call with slice 100 leaves, per instance,
    a sample iteration (51), the cold dual residual there and -- in the primal sample's place --
    its key, 1e30.  A warm-started call with slice 7 on the same context is suspended at
    iteration 25 with small residuals and no sample of its own; extrapolating from the cold
    call's leftovers gives a finite (negative) key where both leftovers exceed the residuals
    now.  With the samples cleared every suspended instance has the fallback 1e30."""
    import mpcq
    syn, _ = trot20
    with mpcq.Engine(20) as e:
        cold = e.solve(syn["xref"], syn["fsteps"], want_x=True, want_y=True)
        warm = dict(warm_x=cold["x"], warm_y=cold["y"], rho=cold["rho"])
        ref = e.solve(syn["xref"], syn["fsteps"], **warm)
    assert (ref["iters"] > 25).sum() >= 1   # (most warm instances end at the first check)
    with mpcq.Engine(20) as e:
        e.set_slice(100)
        e.solve(syn["xref"], syn["fsteps"])
        assert e.last_dispatch()["count"] == 300
        e.set_slice(7)
        r = e.solve(syn["xref"], syn["fsteps"], **warm)
        d = e.last_dispatch()
        assert np.array_equal(r["iters"], ref["iters"]) and np.array_equal(r["f0"], ref["f0"])
        assert d["sliced"] and d["count"] == int((ref["iters"] > 25).sum())
        key = d["key"][d["list"], 0]
        assert (key == 1e30).all(), key[key != 1e30][:5]
        assert np.array_equal(d["list"], np.flatnonzero(ref["iters"] > 25))   # one bucket: index order


def test_slice16_in_the_environment_does_not_slice_the_default_library(monkeypatch):
    """MPCQ_SLICE16=1 (once the switch of an experiment build; nothing reads it any more) against
    the library, whose 16-stage engine holds no suspend / resume code: the solve must not take
    the two-launch path (its second launch would read a list nobody wrote) -- one launch, the
    same bits."""
    import mpcq
    from mpcq import synth
    # the library that answers this query is the one that gates slicing on the engine's build
    assert hasattr(mpcq.lib(), "mpcq_debug_last_dispatch")
    syn = synth.make_batch(200, 16, gaits=("trot",), seed=2)
    kw = dict(want_x=True, want_y=True)
    with mpcq.Engine(16) as e0:
        ref = e0.solve(syn["xref"], syn["fsteps"], **kw)
    monkeypatch.setenv("MPCQ_SLICE16", "1")
    with mpcq.Engine(16) as e1:
        e1.set_slice(25)
        for by_class in (False, True):
            got = e1.solve(syn["xref"], syn["fsteps"], order_by_class=by_class, **kw)
            d = e1.last_dispatch()
            assert not d["sliced"] and d["count"] == 0 and len(d["list"]) == 0 and d["key"] is None
            for k in ("f0", "x", "y", "status", "iters", "rho", "rho_updates", "admm_status", "polish",
                      "polish_rounds"):
                assert np.array_equal(ref[k], got[k], equal_nan=True), (by_class, k)
