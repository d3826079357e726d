"""Host model of the rigid-body plant (mpc-tsid_amd/csrc/mpcq_plant.hip), in numpy.

A restatement of what mpcq_plant_step_batch computes per robot, and of what a session tick
with the plant enabled does after it, written from the equations of include/mpcq.h:

  effective   the forces the plant applies: none at a swing foot (any NaN coordinate); with
              clamp a stance foot's fz limited to [0, fz_max] and its tangential part scaled
              onto the Coulomb cone t = mu fz
  step        one tick: PLANT_MODEL, the MPC's own discrete step (MPC.py:110-119, 171-178,
              201) with the plant's constants, or PLANT_RIGID, n_sub semi-implicit Euler
              substeps of the full rotational dynamics
  tail        the world pose and the virtual robot's next state and feet from the state a
              robot ends the tick in (MPC.py:503-510, Interface.py:100-138)
  session_tick  a session's plant launch: world wrench -> local frame, step, tail

Everything is elementwise float64 arithmetic over the batch axis, sums left to right in the
order the kernel documents and never through BLAS, so model and kernel differ by the device
library's sin / cos (and by the one fma of the world pose, which numpy's np.dot(R, q) makes
and this file does not: one rounding of an O(1) quantity) only.
"""
import numpy as np

MODEL, RIGID = 0, 1
DEFAULTS = dict(dt=0.02, gravity=9.81, n_sub=20, integrator=RIGID, clamp=1)
# mpcq_default_params: MPC.py:28, 35-37, 39, 228
MASS = 2.50000279
GI = np.array([[3.09249e-2, -8.00101e-7, 1.865287e-5],
               [-8.00101e-7, 5.106100e-2, 1.245813e-4],
               [1.865287e-5, 1.245813e-4, 6.939757e-2]])
MU, FZ_MAX = 0.9, 25.0
SHOULDERS = np.array([[0.19, 0.19, -0.19, -0.19], [0.15005, -0.15005, 0.15005, -0.15005]])


def constants(B, mass=None, gI=None, mu=None, fz_max=None):
    """(mass (B,), gI (B,3,3), mu (B,), fz_max (B,)); None = the default parameters."""
    bc = lambda v, d, shp: np.broadcast_to(np.asarray(d if v is None else v, np.float64), shp).copy()  # noqa: E731
    return bc(mass, MASS, (B,)), bc(gI, GI, (B, 3, 3)), bc(mu, MU, (B,)), bc(fz_max, FZ_MAX, (B,))


def from_table(table):
    """The same from a (B,) array of mpcq.ROBOT_DTYPE."""
    return (table["mass"].astype(np.float64), table["gI"].astype(np.float64).reshape(-1, 3, 3),
            table["mu"].astype(np.float64), table["fz_max"].astype(np.float64))


def effective(feet, f, mu, fz_max, clamp):
    """feet (B,3,4) as l_feet, f (B,12) foot-major -> (f_eff (B,4,3), swing (B,4))."""
    f = np.array(f, np.float64).reshape(-1, 4, 3)
    swing = np.isnan(np.asarray(feet, np.float64)).any(axis=1)  # (B,4)
    fx = np.where(swing, 0.0, f[:, :, 0])
    fy = np.where(swing, 0.0, f[:, :, 1])
    fz = np.where(swing, 0.0, f[:, :, 2])
    if clamp:
        with np.errstate(invalid="ignore", divide="ignore"):
            fz = np.where(fz < 0.0, 0.0, fz)  # comparisons: a NaN stays a NaN
            fz = np.where(fz > fz_max[:, None], np.broadcast_to(fz_max[:, None], fz.shape), fz)
            t = np.sqrt(fx * fx + fy * fy)
            lim = mu[:, None] * fz
            out = t > lim
            sc = np.where(out, lim / np.where(out, t, 1.0), 1.0)
            fx = np.where(out, fx * sc, fx)
            fy = np.where(out, fy * sc, fy)
    return np.stack([fx, fy, fz], axis=2), swing


def _solve3(m, b):
    """inv(m) b by the adjugate; m (B,3,3), b (B,3)."""
    c00 = m[:, 1, 1] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 1]
    c01 = m[:, 0, 2] * m[:, 2, 1] - m[:, 0, 1] * m[:, 2, 2]
    c02 = m[:, 0, 1] * m[:, 1, 2] - m[:, 0, 2] * m[:, 1, 1]
    c10 = m[:, 1, 2] * m[:, 2, 0] - m[:, 1, 0] * m[:, 2, 2]
    c11 = m[:, 0, 0] * m[:, 2, 2] - m[:, 0, 2] * m[:, 2, 0]
    c12 = m[:, 0, 2] * m[:, 1, 0] - m[:, 0, 0] * m[:, 1, 2]
    c20 = m[:, 1, 0] * m[:, 2, 1] - m[:, 1, 1] * m[:, 2, 0]
    c21 = m[:, 0, 1] * m[:, 2, 0] - m[:, 0, 0] * m[:, 2, 1]
    c22 = m[:, 0, 0] * m[:, 1, 1] - m[:, 0, 1] * m[:, 1, 0]
    det = (m[:, 0, 0] * c00 + m[:, 0, 1] * c10) + m[:, 0, 2] * c20
    return np.stack([((c00 * b[:, 0] + c01 * b[:, 1]) + c02 * b[:, 2]) / det,
                     ((c10 * b[:, 0] + c11 * b[:, 1]) + c12 * b[:, 2]) / det,
                     ((c20 * b[:, 0] + c21 * b[:, 1]) + c22 * b[:, 2]) / det], axis=1)


def _mat(rows):
    """(B,3,3) from a 3x3 nest of (B,) arrays."""
    return np.stack([np.stack(r, axis=1) for r in rows], axis=1)


def step(state, feet, f, wrench=None, consts=None, **params):
    """One tick for B robots.  state (B,12), feet (B,3,4), f (B,12), wrench (B,6) or None in
    the state's frame, consts = (mass, gI, mu, fz_max) or None.  Returns (state_out (B,12),
    f_eff (B,12))."""
    p = dict(DEFAULTS, **params)
    x = np.array(state, np.float64).reshape(-1, 12)
    B = x.shape[0]
    feet = np.asarray(feet, np.float64).reshape(B, 3, 4)
    mass, gI, mu, fz_max = consts if consts is not None else constants(B)
    w = np.zeros((B, 6)) if wrench is None else np.asarray(wrench, np.float64).reshape(B, 6)
    fe, swing = effective(feet, f, mu, fz_max, p["clamp"])
    F = [np.zeros(B), np.zeros(B), np.zeros(B)]
    T = [np.zeros(B), np.zeros(B), np.zeros(B)]
    for q in range(4):  # lever arms at the tick's start, held for the tick
        sw = swing[:, q]
        rx = np.where(sw, 0.0, feet[:, 0, q] - x[:, 0])
        ry = np.where(sw, 0.0, feet[:, 1, q] - x[:, 1])
        rz = np.where(sw, 0.0, feet[:, 2, q] - x[:, 2])
        fx, fy, fz = fe[:, q, 0], fe[:, q, 1], fe[:, q, 2]
        F = [F[0] + fx, F[1] + fy, F[2] + fz]
        T = [T[0] + (ry * fz - rz * fy), T[1] + (rz * fx - rx * fz), T[2] + (rx * fy - ry * fx)]
    F = [F[i] + w[:, i] for i in range(3)]
    T = np.stack([T[i] + w[:, 3 + i] for i in range(3)], axis=1)
    dt, g = float(p["dt"]), float(p["gravity"])
    x = x.copy()
    if p["integrator"] == MODEL:
        c, s = np.cos(x[:, 5]), np.sin(x[:, 5])
        m = _mat([[c * gI[:, 0, j] - s * gI[:, 1, j] for j in range(3)],
                  [s * gI[:, 0, j] + c * gI[:, 1, j] for j in range(3)],
                  [gI[:, 2, j] for j in range(3)]])  # Rz(yaw0) gI, the reference's form
        al = _solve3(m, T)
        x[:, 0:3] = x[:, 0:3] + dt * x[:, 6:9]
        x[:, 3:6] = x[:, 3:6] + dt * x[:, 9:12]
        x[:, 6] = x[:, 6] + (dt * F[0]) / mass
        x[:, 7] = x[:, 7] + (dt * F[1]) / mass
        x[:, 8] = (x[:, 8] + (dt * F[2]) / mass) - dt * g
        x[:, 9:12] = x[:, 9:12] + dt * al
        return x, fe.reshape(B, 12)
    if p["integrator"] != RIGID:
        raise ValueError("unknown integrator")
    n_sub = int(p["n_sub"])
    h = dt / float(n_sub)
    a = [F[0] / mass, F[1] / mass, F[2] / mass - g]
    for _ in range(n_sub):
        cr, sr = np.cos(x[:, 3]), np.sin(x[:, 3])
        cp, sp = np.cos(x[:, 4]), np.sin(x[:, 4])
        cy, sy = np.cos(x[:, 5]), np.sin(x[:, 5])
        R = [[cy * cp, (cy * sp) * sr - sy * cr, (cy * sp) * cr + sy * sr],
             [sy * cp, (sy * sp) * sr + cy * cr, (sy * sp) * cr - cy * sr],
             [-sp, cp * sr, cp * cr]]  # Rz(yaw) Ry(pitch) Rx(roll)
        RG = [[(R[i][0] * gI[:, 0, j] + R[i][1] * gI[:, 1, j]) + R[i][2] * gI[:, 2, j] for j in range(3)]
              for i in range(3)]
        Iw = [[(RG[i][0] * R[j][0] + RG[i][1] * R[j][1]) + RG[i][2] * R[j][2] for j in range(3)] for i in range(3)]
        wx, wy, wz = x[:, 9], x[:, 10], x[:, 11]
        Lw = [(Iw[i][0] * wx + Iw[i][1] * wy) + Iw[i][2] * wz for i in range(3)]
        rhs = np.stack([T[:, 0] - (wy * Lw[2] - wz * Lw[1]), T[:, 1] - (wz * Lw[0] - wx * Lw[2]),
                        T[:, 2] - (wx * Lw[1] - wy * Lw[0])], axis=1)
        al = _solve3(_mat(Iw), rhs)
        for i in range(3):
            x[:, 6 + i] = x[:, 6 + i] + h * a[i]
            x[:, 9 + i] = x[:, 9 + i] + h * al[:, i]
            x[:, i] = x[:, i] + h * x[:, 6 + i]
        nx, ny, nz = x[:, 9].copy(), x[:, 10].copy(), x[:, 11].copy()
        x[:, 3] = x[:, 3] + h * ((cy * nx + sy * ny) / cp)
        x[:, 4] = x[:, 4] + h * ((-sy) * nx + cy * ny)
        x[:, 5] = x[:, 5] + h * (((cy * sp) * nx + (sy * sp) * ny) / cp + nz)
    return x, fe.reshape(B, 12)


def tail(end, q_w_prev, fsteps, gait, shoulders=SHOULDERS):
    """The retrieve's formulas with the plant's end state in place of x_robot[:, 0]:
    end (B,12), q_w_prev (B,6), fsteps (B,20,13), gait (B,20,5) -> (q_w, state, l_feet)."""
    qn = np.asarray(end, np.float64)
    B = qn.shape[0]
    qp = np.asarray(q_w_prev, np.float64)
    c, s = np.cos(qp[:, 5]), np.sin(qp[:, 5])
    q_w = np.empty((B, 6))
    q_w[:, 0] = qp[:, 0] + (c * qn[:, 0] + (-s) * qn[:, 1])
    q_w[:, 1] = qp[:, 1] + (s * qn[:, 0] + c * qn[:, 1])
    q_w[:, 2:5] = qn[:, 2:5]
    q_w[:, 5] = qp[:, 5] + qn[:, 5]
    cy, sy = np.cos(qn[:, 5]), np.sin(qn[:, 5])
    ns = np.zeros((B, 12))
    ns[:, 2:5] = qn[:, 2:5]
    ns[:, 6] = cy * qn[:, 6] + sy * qn[:, 7]
    ns[:, 7] = -sy * qn[:, 6] + cy * qn[:, 7]
    ns[:, 8] = qn[:, 8]
    ns[:, 9] = cy * qn[:, 9] + sy * qn[:, 10]
    ns[:, 10] = -sy * qn[:, 9] + cy * qn[:, 10]
    ns[:, 11] = qn[:, 11]
    # the stance feet of the phase current after the next roll; swing feet under the shoulders
    row = np.where(np.asarray(gait)[:, 0, 0] > 1.0, 0, 1)
    fs = np.asarray(fsteps, np.float64)[np.arange(B), row, 1:].reshape(B, 4, 3)
    swing = np.isnan(fs).any(axis=2)
    sh = np.asarray(shoulders, np.float64).reshape(2, 4)
    px = np.where(swing, sh[0][None, :] + qn[:, 0:1], fs[:, :, 0])
    py = np.where(swing, sh[1][None, :] + qn[:, 1:2], fs[:, :, 1])
    pz = np.where(swing, 0.0, fs[:, :, 2])
    dx, dy = px - qn[:, 0:1], py - qn[:, 1:2]
    lf = np.empty((B, 3, 4))
    lf[:, 0] = cy[:, None] * dx + sy[:, None] * dy
    lf[:, 1] = -sy[:, None] * dx + cy[:, None] * dy
    lf[:, 2] = pz
    return q_w, ns, lf


def session_tick(state, fsteps, gait, f0, q_w_prev, wrench_world=None, consts=None, shoulders=SHOULDERS,
                 **params):
    """A session's plant launch for robots that solved: state (B,12) what the tick's planner
    read (xref[:, :, 0]), the stance feet of fsteps row 0, f0 = SV_F0, the WORLD wrench rotated
    by Rz(-yaw), yaw = q_w_prev[:, 5].  Returns dict(end, f_eff, q_w, state, l_feet)."""
    B = np.asarray(state).shape[0]
    fs = np.asarray(fsteps, np.float64)
    feet = fs[:, 0, 1:].reshape(B, 4, 3).transpose(0, 2, 1)  # (B,3,4) as l_feet
    qp = np.asarray(q_w_prev, np.float64)
    w = None
    if wrench_world is not None:
        ww = np.asarray(wrench_world, np.float64).reshape(B, 6)
        c, s = np.cos(qp[:, 5]), np.sin(qp[:, 5])
        w = ww.copy()
        w[:, 0] = c * ww[:, 0] + s * ww[:, 1]
        w[:, 1] = -s * ww[:, 0] + c * ww[:, 1]
        w[:, 3] = c * ww[:, 3] + s * ww[:, 4]
        w[:, 4] = -s * ww[:, 3] + c * ww[:, 4]
    end, fe = step(state, feet, f0, w, consts, **params)
    q_w, ns, lf = tail(end, qp, fs, gait, shoulders)
    return dict(end=end, f_eff=fe, q_w=q_w, state=ns, l_feet=lf)
