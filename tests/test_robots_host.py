"""CPU: the mpcq_robot ABI, its Python mirrors, and the power of tests/robot_cases.py.

test_gpu_robots.py compares the engine under a per-robot table with per-instance oracle solves.
That comparison only means something if the table moves every instance: the power test below
re-establishes, from the oracle alone and at every horizon of the table, that

* every instance is SOLVED;
* the oracle's checker build and its -O3 -march=native build agree on status and iteration
  count on every instance (no instance on a rounding knife-edge);
* every instance's f0 moves by more than 1e-5 (200x the GPU tolerance) from the default robot's
  result and from the result under its neighbour's robot (robots[(b + 1) % B]): a kernel that
  ignored the table, or read another row, would miss.

These are conditions on the inputs, not tolerances: a recipe that fails them is replaced, not
relaxed.
"""
import ctypes as C

import numpy as np
import pytest

import robot_cases as RC


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as m
    m.build()
    return m


def test_robot_struct_layout(mpcq):
    L = mpcq._lib
    assert C.sizeof(L.Robot) == 128
    assert [(n, getattr(L.Robot, n).offset) for n, _ in L.Robot._fields_] == [
        ("mass", 0), ("gI", 8), ("mu", 80), ("fz_max", 88), ("reserved", 96)]
    dt = mpcq.ROBOT_DTYPE
    assert dt.itemsize == 128
    assert [(n, dt.fields[n][1]) for n in dt.names] == [("mass", 0), ("gI", 8), ("mu", 80), ("fz_max", 88),
                                                        ("reserved", 96)]
    # (the C side: include/mpcq.h carries a static assertion of the size, so a library whose
    # struct is not 128 bytes does not build)
    import os
    from conftest import REPO
    src = open(os.path.join(REPO, "include", "mpcq.h")).read()
    assert src.count("_Static_assert(sizeof(mpcq_robot) == 128") == 1
    assert src.count("static_assert(sizeof(mpcq_robot) == 128") == 1  # (the C++ spelling)


def test_default_robot_equals_default_params(mpcq):
    p = mpcq.default_params()
    for r in (mpcq.default_robot(), mpcq.default_robot(p)):
        assert r.mass == p.mass and r.mu == p.mu and r.fz_max == p.fz_max
        assert list(r.gI) == list(p.gI)
        assert list(r.reserved) == [0.0] * 4
    q = mpcq.default_params(mass=3.5, mu=0.5, fz_max=17.0, gI=(C.c_double * 9)(*range(1, 10)))
    r = mpcq.default_robot(q)
    assert (r.mass, r.mu, r.fz_max, list(r.gI)) == (3.5, 0.5, 17.0, [float(v) for v in range(1, 10)])
    mpcq.lib().mpcq_default_robot(None, None)  # a NULL output is ignored, never a crash


def test_robots_broadcasting_and_defaults(mpcq):
    p = mpcq.default_params()
    gI0 = np.array(p.gI[:]).reshape(3, 3)
    t = mpcq.robots(5)
    assert t.shape == (5,) and t.dtype == mpcq.ROBOT_DTYPE and t.flags.c_contiguous
    assert (t["mass"] == p.mass).all() and (t["mu"] == p.mu).all() and (t["fz_max"] == p.fz_max).all()
    assert (t["gI"] == gI0).all() and (t["reserved"] == 0).all()
    # scalar, (B,), (3,3) and (B,3,3) inputs; the rest from params
    q = mpcq.default_params(mu=0.6, fz_max=19.0)
    m = np.linspace(2.0, 4.0, 5)
    g1 = np.arange(9.0).reshape(3, 3) + 1
    t = mpcq.robots(5, mass=m, gI=g1, params=q)
    assert np.array_equal(t["mass"], m) and (t["mu"] == 0.6).all() and (t["fz_max"] == 19.0).all()
    assert (t["gI"] == g1).all()
    gB = np.arange(45.0).reshape(5, 3, 3)
    t = mpcq.robots(5, mass=3.0, gI=gB, mu=np.full(5, 0.7), fz_max=21.0)
    assert (t["mass"] == 3.0).all() and np.array_equal(t["gI"], gB) and (t["mu"] == 0.7).all()
    assert (t["fz_max"] == 21.0).all()
    # row-major gI, as mpcq_params.gI: the bytes of a row are a mpcq_robot
    r = mpcq.Robot.from_buffer_copy(t[2].tobytes())
    assert list(r.gI) == gB[2].ravel().tolist() and r.mass == 3.0 and r.fz_max == 21.0
    with pytest.raises(ValueError):
        mpcq.robots(5, mass=np.ones(4))
    with pytest.raises(ValueError):
        mpcq.robots(5, gI=np.ones((4, 3, 3)))


def test_recipe_is_the_documented_one(mpcq):
    """The first instance of N = 16 drawn by hand in the documented order."""
    d = np.diag(np.array(mpcq.default_params().gI[:]).reshape(3, 3))
    rng = np.random.default_rng(716)
    sc = rng.uniform(0.5, 2.0, 3)
    off = rng.uniform(-0.1, 0.1, (3, 3)) * np.sqrt(np.outer(d * sc, d * sc))
    np.fill_diagonal(off, 0.0)
    t = RC.make_robots(16)
    assert t.shape == (16,)
    assert np.array_equal(t["gI"][0], np.diag(d * sc) + off)
    assert t["mass"][0] == rng.uniform(1.5, 4.0) and t["mu"][0] == rng.uniform(0.4, 1.0)
    assert t["fz_max"][0] == rng.uniform(20, 30)
    assert not np.allclose(t["gI"][0], t["gI"][0].T, rtol=1e-3, atol=0)  # not symmetric, on purpose
    assert (t["mass"] >= 1.5).all() and (t["mass"] < 4.0).all() and (t["mu"] >= 0.4).all() and (t["mu"] < 1.0).all()


@pytest.mark.parametrize("N", RC.HORIZONS)
def test_recipe_has_power(oracle, N):
    rob = RC.make_robots(N)
    B = rob.shape[0]
    assert B == (16 if N <= 20 else 8)
    r = RC.oracle_solve(oracle, N, rob, key="table")
    nat = RC.oracle_solve(oracle, N, rob, native=True)
    dflt = RC.oracle_solve(oracle, N, None)
    nb = RC.oracle_solve(oracle, N, np.roll(rob, -1))  # instance b under robots[(b + 1) % B]
    assert (r["status"] == 1).all(), r["status"]
    assert np.array_equal(r["status"], nat["status"])
    assert np.array_equal(r["iters"], nat["iters"]), (r["iters"], nat["iters"])
    d_nat = float(np.abs(r["f0"] - nat["f0"]).max())
    mv_d = np.abs(r["f0"] - dflt["f0"]).max(axis=1)
    mv_n = np.abs(r["f0"] - nb["f0"]).max(axis=1)
    print(f"N={N}: iters {r['iters'].min()}..{r['iters'].max()}, builds differ by {d_nat:.1e}, "
          f"movement vs defaults >= {mv_d.min():.2e}, vs the neighbour's robot >= {mv_n.min():.2e}")
    assert (mv_d > 1e-5).all(), mv_d
    assert (mv_n > 1e-5).all(), mv_n
