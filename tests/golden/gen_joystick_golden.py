"""Generate tests/golden/joystick_golden.npz (run where the reference tree is; never by a test).

    MPC_TSID_REFERENCE=<reference checkout> python tests/golden/gen_joystick_golden.py

Imports the UNMODIFIED reference file Joystick.py.  It imports ``gamepadClient`` (which imports
``inputs``) at its top, only for the gamepad path; empty stand-ins go into ``sys.modules``.
Records ``v_ref`` of ``Joystick(k_mpc=20).update_v_ref_predefined(20 * tau)`` for the MPC ticks
tau = 0..260 (the ramp of Joystick.py:82-83 starts at tau = 48 and ends at tau = 223): keys
``tau`` (261,) int32 and ``v_ref`` (261, 6) float64.

Only data leaves this script.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
K_MPC, TICKS = 20, 261


def main():
    ref = os.environ.get("MPC_TSID_REFERENCE")
    if not ref or not os.path.exists(os.path.join(ref, "Joystick.py")):
        raise SystemExit("set MPC_TSID_REFERENCE to a checkout of the reference")
    for name in ("gamepadClient", "inputs"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, ref)
    import Joystick
    joy = Joystick.Joystick(K_MPC)
    rows = []
    for tau in range(TICKS):
        joy.update_v_ref_predefined(K_MPC * tau)
        rows.append(np.asarray(joy.v_ref, np.float64).reshape(6).copy())
    out = os.path.join(HERE, "joystick_golden.npz")
    np.savez_compressed(out, tau=np.arange(TICKS, dtype=np.int32), v_ref=np.array(rows))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
