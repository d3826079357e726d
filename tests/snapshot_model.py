"""The snapshot blob's format, restated with numpy from the text of include/mpcq.h
(mpcq_session_snapshot_export): the header of format versions 1 to 5 and the ordered list of the
arrays behind it.  Shared by the GPU layout test and the host test of the layout unit.

``layout(...)`` returns ``(header, arrays)``: the header's bytes and a list of ``(name, bytes)``,
name the ``mpcq`` constant of a named array ("SV_F0", "PV_WRENCH", "robots", ...) or, for an array
the snapshot holds behind the named ones, a name in parentheses."""
import struct

MAGIC = b"MPCQSNP1"
# the parts in the blob's order, with the flags bit and the format version each one forces
PARTS = ("main", "swing", "plant", "monitor", "scenario", "robots", "plant_robots", "channel", "estimator", "gait",
         "disturb")
OPTIONAL = PARTS[1:]
FLAG = {"swing": 4, "plant": 8, "monitor": 16, "scenario": 32, "robots": 64, "plant_robots": 128, "channel": 256,
        "estimator": 512, "gait": 1024, "disturb": 2048}
VERSION = {"channel": 2, "estimator": 3, "gait": 4, "disturb": 5}
HEADER_BYTES = {1: 128, 2: 128, 3: 128, 4: 144, 5: 160}
ROBOT_BYTES = 128  # mpcq_robot: 16 doubles
SWING_STATE, EST_ROW, DIST_ROW, MAX_DELAY, MAX_LATENCY = 40, 332, 80, 8, 4


def arrays_of(part, N, B, k_mpc=0):
    """(name, bytes) of the arrays of one part that a snapshot holds, by array id."""
    d, i = 8 * B, 4 * B
    if part == "main":  # MPCQ_SV_ORDER, the swing slots and the staging of host inputs are not held
        return [("SV_F0", 12 * d), ("SV_X", 24 * N * d), ("SV_X_ROBOT", 12 * N * d), ("SV_Q_W", 6 * d),
                ("SV_COST", 13 * d), ("SV_XREF", 12 * (N + 1) * d), ("SV_FSTEPS", 260 * d), ("SV_GAIT", 100 * d),
                ("SV_STATUS", i), ("SV_ITERS", i), ("SV_RHO", d), ("SV_Y", 44 * N * d), ("SV_STATE", 12 * d),
                ("SV_L_FEET", 12 * d), ("SV_ROT_FLAG", i), ("SV_H_ROT", d), ("SV_FIRST", i),
                ("(warm start)", 24 * N * d), ("(planner status)", i), ("(engine info)", 4 * i),
                ("(creation gait)", 100 * d)]
    if part == "swing":
        return [("SV_SWING_REF", k_mpc * 36 * d), ("SV_SWING_STATE", 4 * SWING_STATE * d), ("SV_FRAME", 3 * d)]
    if part == "plant":  # the plant's copy of q_w is not held
        return [("PV_STATE_END", 12 * d), ("PV_F_EFF", 12 * d), ("PV_WRENCH", 6 * d)]
    if part == "monitor":
        return [("MV_DONE", i), ("MV_EP", 8 * d), ("MV_EP_TICKS", i), ("MV_EPISODES", i), ("MV_LAST", 16 * d),
                ("MV_TOTALS", 64)]
    if part == "scenario":
        return [("CV_EPOCH", i), ("CV_TICK", i), ("CV_V_REF", 6 * d), ("CV_PUSH", 6 * d), ("CV_WRENCH", 6 * d),
                ("CV_ROBOTS", ROBOT_BYTES * B), ("CV_DRAW", 8 * d)]
    if part == "robots":
        return [("robots", ROBOT_BYTES * B)]
    if part == "plant_robots":
        return [("(plant robots)", ROBOT_BYTES * B)]
    if part == "channel":
        return [("HV_CLOCK", 2 * i), ("HV_OBS", 12 * d), ("HV_F_CMD", 12 * d), ("HV_DRAW", 16 * d),
                ("HV_S_RING", MAX_DELAY * 12 * d), ("HV_F_RING", MAX_LATENCY * 12 * d)]
    if part == "estimator":  # MPCQ_EV_EST is derived
        return [("EV_ROW", EST_ROW * d)]
    if part == "gait":
        return [("GV_STATE", 4 * i)]
    if part == "disturb":  # MPCQ_DV_DIST and MPCQ_DV_RESID are derived
        return [("DV_ROW", DIST_ROW * d)]
    raise KeyError(part)


def version_of(parts):
    return max([1] + [VERSION.get(p, 1) for p in parts])


def layout(N, B, k_mpc=0, parts=(), delay=0, latency=0, n_gaits=0, have_order=False, resets=False, user=0):
    """``parts``: the optional parts present (names of OPTIONAL; "swing" goes with k_mpc > 0, delay and
    latency with "channel", n_gaits with "gait")."""
    parts = set(parts)
    assert parts <= set(OPTIONAL) and ("swing" in parts) == (k_mpc > 0)
    present = [p for p in PARTS if p == "main" or p in parts]
    arrays, part_bytes = [], {}
    for p in present:
        a = arrays_of(p, N, B, k_mpc)
        arrays += a
        part_bytes[p] = sum(nb for _, nb in a)
    version = version_of(parts)
    flags = (1 if have_order else 0) | (2 if resets else 0)
    for p in parts:
        flags |= FLAG[p]
    total = HEADER_BYTES[version] + sum(part_bytes.values())
    h = MAGIC + struct.pack("<IiqiI", version, N, B, k_mpc, flags)
    h += struct.pack("<7q", *(part_bytes.get(p, 0) for p in PARTS[:7]))
    h += struct.pack("<qq", total, user)
    h += struct.pack("<qiiq", part_bytes.get("channel", 0), delay, latency, part_bytes.get("estimator", 0))
    if version >= 4:
        h += struct.pack("<qii", part_bytes.get("gait", 0), n_gaits, 0)
    if version >= 5:
        h += struct.pack("<qq", part_bytes.get("disturb", 0), 0)
    assert len(h) == HEADER_BYTES[version]
    return h, arrays


# The eight shapes both tests walk: name -> the keywords of layout() but N, B and the flags.
CASES = {
    "nothing": dict(),
    "seven_parts": dict(k_mpc=7, parts=("swing", "plant", "monitor", "scenario", "robots", "plant_robots")),
    "channel": dict(parts=("channel",), delay=2, latency=1),
    "channel_estimator": dict(parts=("channel", "estimator"), delay=2, latency=1),
    "estimator": dict(parts=("estimator",)),
    "gait": dict(parts=("gait",), n_gaits=2),
    "disturb": dict(parts=("disturb",)),
    "everything": dict(k_mpc=7, parts=OPTIONAL, delay=2, latency=1, n_gaits=2),
}
CASE_VERSION = {"nothing": 1, "seven_parts": 1, "channel": 2, "channel_estimator": 3, "estimator": 3, "gait": 4,
                "disturb": 5, "everything": 5}
