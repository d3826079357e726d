"""Drop-in module name for the reference's FootTrajectoryGenerator.py: the class
``Foot_trajectory_generator(h, time_adaptative_disabled)`` (FootTrajectoryGenerator.py:184-380)
over the HIP swing kernel (mpcq_swing_step_batch), a batch of one.

``get_next_foot(x0, dx0, ddx0, y0, dy0, ddy0, x1, y1, t0, t1, dt)`` returns the reference's
list ``[x0, dx0, ddx0, y0, dy0, ddy0, z0, dz0, ddz0, x1, y1]``; ``lastCoeffs``, ``x1`` and ``y1``
are the reference's attributes.  There is no CPU fallback.  (The reference's
``FootTrajectoryGenerator`` wrapper class is not provided: nothing instantiates it.)
"""
import numpy as np

import mpcq

_engine = None


def _shared_engine(device=0):
    global _engine
    if _engine is None:
        _engine = mpcq.Engine(16, device=device)
    return _engine


class Foot_trajectory_generator(object):
    def __init__(self, h=0.03, time_adaptative_disabled=0.200, engine=None):
        self.h = h
        self.time_adaptative_disabled = time_adaptative_disabled
        self._swing = mpcq.Swing(engine if engine is not None else _shared_engine(), 1)
        self._st = self._swing.state[0, 0]

    @property
    def lastCoeffs(self):
        return [float(v) for v in self._st[0:24]]

    @lastCoeffs.setter
    def lastCoeffs(self, v):
        self._st[0:24] = np.asarray(v, np.float64)

    @property
    def x1(self):
        return float(self._st[24])

    @x1.setter
    def x1(self, v):
        self._st[24] = float(v)

    @property
    def y1(self):
        return float(self._st[25])

    @y1.setter
    def y1(self, v):
        self._st[25] = float(v)

    def get_next_foot(self, x0, dx0, ddx0, y0, dy0, ddy0, x1, y1, t0, t1, dt):
        p = self._swing.params
        p.dt, p.max_height, p.t_lock = float(dt), float(self.h), float(self.time_adaptative_disabled)
        args = np.full((1, 4, 10), np.nan)  # feet 1..3: skipped
        args[0, 0] = (x0, dx0, ddx0, y0, dy0, ddy0, x1, y1, t0, t1)
        return [float(v) for v in self._swing.step(args)[0, 0]]
