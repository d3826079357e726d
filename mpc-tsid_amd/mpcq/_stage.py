"""Marshalling the stage wrappers share: the device-pointer calls' pointers and flags, and the
inputs of the stages that run the controller's model (estimator.py, disturb.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import ROBOT_DTYPE


def v(q: int):
    """A device pointer for a ``step_device`` call; 0 = absent."""
    return C.c_void_p(q) if q else None


def device_flags(asynchronous: bool) -> int:
    return L.FLAG_DEVICE_PTRS | (L.FLAG_ASYNC if asynchronous else 0)


def model_inputs(name: str, meas, f_prev, feet_prev, rows, width: int, first, failed_prev, robots):
    """The arrays of one model-stage tick as the C entry points take them: ``meas`` (B, 12) under
    its ``name``, ``f_prev`` (B, 12), ``feet_prev`` (B, 3, 4), ``rows`` (B, width) (None: zeros),
    the (B,) masks and the (B,) robots table.  Returns B, rows and the arrays (or None) from
    ``first`` to ``rows`` in the entry points' order, ``all_first`` left out."""
    meas = np.ascontiguousarray(meas, np.float64)
    if meas.ndim != 2 or meas.shape[1] != 12:
        raise ValueError(f"{name} must be (B, 12)")
    B = meas.shape[0]
    f_prev = np.ascontiguousarray(np.broadcast_to(np.asarray(f_prev, np.float64), (B, 12)))
    feet_prev = np.ascontiguousarray(np.broadcast_to(np.asarray(feet_prev, np.float64), (B, 3, 4)))
    if rows is None:
        rows = np.zeros((B, width))
    if not (isinstance(rows, np.ndarray) and rows.shape == (B, width) and rows.dtype == np.float64
            and rows.flags.c_contiguous):
        raise ValueError(f"rows must be a contiguous float64 array of shape ({B}, {width})")
    mask = lambda m: None if m is None else np.ascontiguousarray(  # noqa: E731
        np.broadcast_to(np.asarray(m) != 0, (B,)), np.int32)
    fi, fa = mask(first), mask(failed_prev)
    tab = None
    if robots is not None:
        tab = np.ascontiguousarray(robots, ROBOT_DTYPE)
        if tab.shape != (B,):
            raise ValueError(f"robots must be ({B},)")
    return B, rows, (fi, meas, f_prev, feet_prev, fa, tab, rows)
