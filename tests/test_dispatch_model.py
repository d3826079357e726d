"""CPU: the host model of the dispatch-order layer (dispatch_model.py) against values worked
out by hand -- the model is what test_gpu_dispatch.py holds the kernels to, so it is pinned
itself first: the synthetic gaits' class slots, a collision modulo 251, the sort, the key
buckets, the table's arithmetic, and the inputs the GPU tests share."""
import math

import numpy as np

import dispatch_model as M


def test_synthetic_gaits_slots():
    """trot: masks {15, 9, 6} -> 2^15 + 2^9 + 2^6 = 33344 = 132 * 251 + 212; bound {15, 3, 12}
    -> 36872 = 146 * 251 + 226; pace {15, 5, 10} -> 33824 = 134 * 251 + 190 -- at every roll
    offset (a rolled table still holds every phase of its period)."""
    from mpcq import synth
    want = {"trot": 212, "bound": 226, "pace": 190}
    for N in (16, 20):
        syn = synth.make_batch(96, N, gaits=synth.GAITS, seed=1)
        assert len(np.unique(syn["offset"])) > 8
        slots = M.class_slots(syn["fsteps"])
        for gi, g in enumerate(synth.GAITS):
            assert (slots[syn["gait"] == gi] == want[g]).all(), g
    assert (1 << 15 | 1 << 9 | 1 << 6) % 251 == 212


def test_collision_and_hand_built_tables():
    cases = {name: (fs, bm) for name, fs, bm in M.slot_cases()}
    for name, (fs, bm) in cases.items():
        assert M.class_bitmap(fs) == bm, name
    # two different gaits in one slot: {0} = 1 and {2..7} = 252 = 251 + 1
    a, b = cases["coll-a1"], cases["coll-a2"]
    assert a[1] != b[1] and a[1] % 251 == b[1] % 251
    assert M.class_slot(a[0]) == M.class_slot(b[0]) == 1
    assert M.class_slot(cases["coll-b1"][0]) == M.class_slot(cases["coll-b2"][0]) == 6
    assert M.class_slot(cases["noterm"][0]) == 0 and M.class_slot(cases["term0"][0]) == 0
    # every non-empty mask occurs, alone and in combinations
    seen = set()
    for _, bm in cases.values():
        seen |= {m for m in range(16) if bm is not None and bm >> m & 1}
    assert seen == set(range(16))


def test_stable_sort_hand_written():
    #          0  1    2  3  4    5  6  7
    buckets = [3, 255, 0, 3, 255, 7, 0, 3]
    want = [1, 4, 5, 0, 3, 7, 2, 6]
    assert M.stable_order(buckets).tolist() == want
    assert M.stable_order_fast(buckets).tolist() == want
    assert M.stable_order([5] * 6).tolist() == list(range(6))
    rng = np.random.default_rng(0)
    b = rng.integers(0, 256, 3000)
    assert np.array_equal(M.stable_order(b), M.stable_order_fast(b))


def test_class_costs_by_hand():
    s = np.zeros(M.SLOTS, np.uint64)
    n = np.zeros(M.SLOTS, np.uint64)
    assert M.class_costs(s, n) == [0] * M.SLOTS   # before any launch
    s[3], n[3] = 159, 10       # mean 15 -> bucket 0
    s[4], n[4] = 160, 10       # mean 16 -> bucket 1
    s[9], n[9] = 4079 * 2 + 1, 2   # mean 4079 -> bucket 254
    s[10], n[10] = 4080, 1     # -> 255
    s[11], n[11] = 10 ** 9, 1  # clamped
    c = M.class_costs(s, n)
    assert (c[3], c[4], c[9], c[10], c[11]) == (0, 1, 254, 255, 255)
    unseen = (159 + 160 + 8159 + 4080 + 10 ** 9) // (10 + 10 + 2 + 1 + 1)
    assert c[0] == c[250] == min(unseen >> 4, 255) == 255
    s2, n2 = M.class_learn(s, n, [3, 3, 4, 7], [1, 0, -5, 640])
    assert (int(s2[3]), int(n2[3]), int(s2[4]), int(n2[4]), int(s2[7]), int(n2[7])) == (160, 11, 160, 10, 640, 1)
    # 64-bit counts: a slot past 2^32 launches keeps its mean
    s[20], n[20] = 600 * (2 ** 32 - 32), 2 ** 32 - 32
    s3, n3 = M.class_learn(s, n, [20] * 64, [600] * 64)
    assert int(n3[20]) == 2 ** 32 + 32 and M.class_costs(s3, n3)[20] == 600 >> 4


def test_key_buckets_by_hand():
    kb = M.key_bucket
    assert [kb(v) for v in (0.0, -1.0, math.nan, -math.inf)] == [0, 0, 0, 0]
    assert [kb(v) for v in (math.inf, 1e30, 2.0 ** 16, 2.0 ** 17)] == [255] * 4
    assert kb(1.0) == 128 and kb(1.05) == 128 and kb(0.95) == 127 and kb(2.0) == 136
    assert kb(2.0 ** -16) == 0 and kb(2.0 ** -17) == 0 and kb(2.0 ** -15.8) == 1
    assert kb(2.0 ** (15.875 + 1 / 64)) == 255 and kb(2.0 ** (15.875 - 1 / 64)) == 254
    st = [100, 1, 100, 100, 2, 100]
    key = [[4.0, 0], [9e9, 0], [1e30, 0], [4.1, 0], [1.0, 0], [0.0, 0]]
    assert M.suspended_list(None, 6, st, key, 100).tolist() == [2, 0, 3, 5]
    assert M.suspended_list([5, 3, 4, 0, 2, 1], 6, st, key, 100).tolist() == [2, 3, 0, 5]
    assert M.suspended_list([5, 3, 4, 0, 2, 1], 3, st, key, 100).tolist() == [3, 5]


def test_shared_keys_stay_off_bucket_edges():
    """The keys test_gpu_dispatch.py feeds the suspended-list kernel: none but an exact power
    of two within 1e-9 of an edge (they keep 0.0156 and more), every special value present."""
    for n in (1, 64, 65, 1024, 1025, 3000):
        for seed in (n, n + 1):
            keys = M.suspended_keys(n, seed)
            assert keys.shape == (n,)
            M.check_key_edges(keys, 1e-9)
    keys = M.suspended_keys(3000, 3000)
    assert np.isnan(keys).any() and np.isposinf(keys).any() and (keys == 1e30).any() and (keys < 0).any()
    assert {2.0 ** -17, 2.0 ** -16, 1.0, 2.0 ** 16, 0.0} <= set(keys[np.isfinite(keys)].tolist())
    assert len({M.key_bucket(float(v)) for v in keys}) == 256


def test_iters_bucket_and_suspend_bound():
    assert [M.iters_bucket(v) for v in (-7, 0, 15, 16, 4079, 4080, 10 ** 6)] == [0, 0, 0, 1, 254, 255, 255]
    # slice 100: the end at 100 may update rho, the next one (125) suspends; 333 -> 350; 7 -> 25
    assert (M.suspend_bound(100), M.suspend_bound(333), M.suspend_bound(7), M.suspend_bound(101)) == (125, 350, 25, 125)
