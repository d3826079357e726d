"""CPU: the session epilogue's array algebra written in numpy, as MPC.py and Logger.py write it,
against the oracle's restatement (oracle.retrieve, session_oracle.c) at all 61 compiled horizons.

test_session_oracle.py pins oracle.retrieve to fixtures captured from the reference at N = 16 and
32 only.  The oracle's cost components come from a hand-written copy of numpy's pairwise summation
(8 partial sums up to 128 elements, halves rounded to a multiple of 8 above) over strided data,
and its warm start from index arithmetic; both have a different shape at every horizon (N < 8:
a plain loop for the states; 12N crosses 128 at N = 11, the halves change with N).  Here numpy
itself sums: ``np.sum`` over the strided slice ``[i:12N:12]`` and over the contiguous force part,
so the oracle's summation order is tied to numpy's at the other 59 horizons too, bit for bit.

The GPU's retrieve_kernel<N> is then compared with the oracle bit for bit at every horizon in
test_gpu_retrieve_horizons.py."""
import numpy as np
import pytest

from horizon_cases import ALL_HORIZONS

SCALES = (1e-3, 1.0, 30.0)
DRAWS = 3


def numpy_retrieve(N, x, xref, weights):
    """x_robot (12, N), cost (13,), warm_x (24N,) from array expressions alone.
    ``weights``: (13,) the diagonal of P per state, then the forces' weight."""
    n = 12 * N
    x_robot = x[:n].reshape(12, N, order="F") + xref[:, 1:]           # MPC.py:432-449
    w = np.concatenate([np.tile(weights[:12], N), np.full(n, weights[12])])
    c = (x * w) * x                                                    # (diag(x) @ diag(P)) @ x, Logger.py:406-418
    cost = np.array([np.sum(c[i:n:12]) for i in range(12)] + [np.sum(c[n:])])
    warm = np.concatenate([x[12:n], np.zeros(12), np.roll(x[n:], -12)])  # MPC.py:403-406
    return x_robot, cost, warm


def _params(O, weights):
    return O.default_params(state_weights=tuple(float(v) for v in weights[:12]), force_weight=float(weights[12]))


def test_all_horizons_are_covered():
    import mpcq
    assert tuple(ALL_HORIZONS) == tuple(mpcq.supported_horizons()) and len(ALL_HORIZONS) == 61


@pytest.mark.parametrize("N", ALL_HORIZONS)
def test_oracle_retrieve_is_numpy(oracle, N):
    rng = np.random.default_rng(4000 + N)
    gait = np.zeros((20, 5))
    gait[0] = [2, 1, 0, 0, 1]
    fsteps = np.full((20, 13), np.nan)
    qw = np.array([0.1, -0.2, 0.2027682, 0.0, 0.0, 0.3])
    for scale in SCALES:
        for _ in range(DRAWS):
            x = scale * rng.standard_normal(24 * N)
            xref = rng.standard_normal((12, N + 1))
            weights = rng.uniform(0.1, 20.0, 13)
            weights[rng.integers(0, 12)] = 0.0  # (the default tuning has zero weights too)
            xr, cost, warm = numpy_retrieve(N, x, xref, weights)
            o = oracle.retrieve(N, x, xref, fsteps, gait, qw, params=_params(oracle, weights))
            assert np.array_equal(o["x_robot"], xr), (N, scale)
            assert o["cost"].tobytes() == cost.tobytes(), (N, scale, o["cost"] - cost)
            assert o["warm_x"].tobytes() == warm.tobytes(), (N, scale)
            # a failed solve restarts cold and leaves the pose alone
            f = oracle.retrieve(N, x, xref, fsteps, gait, qw, failed=True, params=_params(oracle, weights))
            assert not f["warm_x"].any() and np.array_equal(f["q_w"], qw) and not np.array_equal(o["q_w"], qw)


def test_a_left_to_right_sum_differs(oracle):
    """The check has power: from 8 stages on, a plain loop over a state's N terms rounds differently
    from numpy's pairwise sum for some draw (below 8 terms numpy itself loops)."""
    rng = np.random.default_rng(1)
    for N in ALL_HORIZONS:
        differs = False
        for _ in range(20):
            x = rng.standard_normal(24 * N)
            _, cost, _ = numpy_retrieve(N, x, np.zeros((12, N + 1)), np.ones(13))
            c = x * x
            loop = [0.0] * 12
            for k in range(N):
                for i in range(12):
                    loop[i] += c[12 * k + i]
            differs |= not np.array_equal(np.array(loop), cost[:12])
        assert differs == (N >= 8), N
