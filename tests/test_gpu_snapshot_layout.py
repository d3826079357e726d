"""GPU: the snapshot blob of every combination of parts that forces a format version, against
tests/snapshot_model.py (written from include/mpcq.h): the header byte for byte, the total, every
part's bytes against the session's own reads, the round trip through import, and the refusals
of a truncated blob and of a restore into a session of another shape.

N = 8, B = 3: the smallest shape with the N = 8 gait table, a non-trivial row gather and every part."""
import re

import numpy as np
import pytest

import snapshot_model as SM
import swing_param_cases as WC

pytestmark = pytest.mark.gpu

N, B, TICKS = 8, 3, 2
# per case: the session of another shape the blob's snapshot is restored into, and the first
# difference the refusal names
OTHER = {
    "nothing": (dict(parts=("plant",)), "the plant arrays exist on one side only"),
    "seven_parts": (dict(SM.CASES["seven_parts"], k_mpc=None), "the swing k_mpc differs"),
    "channel": (dict(parts=("channel",), delay=1, latency=1),
                "the channel's delay differs (the rings were filled under another)"),
    "channel_estimator": (SM.CASES["channel"], "the estimator arrays exist on one side only"),
    "estimator": (dict(), "the estimator arrays exist on one side only"),
    "gait": (dict(parts=("gait",), n_gaits=3), "the gait library sizes differ (the rows index another library)"),
    "disturb": (dict(), "the disturb arrays exist on one side only"),
    "everything": (dict(SM.CASES["everything"], latency=2),
                   "the channel's latency differs (the rings were filled under another)"),
}


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


@pytest.fixture(scope="module")
def eng(mpcq):
    with mpcq.Engine(N, dt=0.04) as e:
        yield e


def _open(mpcq, eng, parts=(), k_mpc=0, delay=0, latency=0, n_gaits=0):
    """A session with exactly these parts (k_mpc None: swing with the default k_mpc)."""
    dt = eng.params.dt
    sess = mpcq.Session(eng, B, gait0=WC.session_gaits(N, B), planner_params=mpcq.default_planner_params(dt=dt))
    rng = np.random.default_rng(5)
    if "swing" in parts:
        sess.enable_swing(None if k_mpc is None else mpcq.default_swing_params(k_mpc=k_mpc))
    if "plant" in parts:
        sess.enable_plant()
    if "monitor" in parts:  # with every part: an auto-reset, so that the blob records a reset
        sess.enable_monitor(max_ticks=1, auto_reset=1 if len(parts) == len(SM.OPTIONAL) else 0)
    if "scenario" in parts:
        sess.enable_scenario()
    if "robots" in parts:
        sess.set_robots(mpcq.robots(B, mass=rng.uniform(2.3, 2.7, B)))
    if "plant_robots" in parts:
        sess.set_plant_robots(mpcq.robots(B, mass=rng.uniform(2.2, 2.9, B)))
    if "channel" in parts:
        sess.enable_channel(delay=delay, latency=latency)
    if "estimator" in parts:
        sess.enable_estimator()
    if "gait" in parts:
        sess.enable_gait([mpcq.gait.cycle(n, dt=dt) for n in ("trot", "bound", "pace")[:n_gaits]])
    if "disturb" in parts:
        sess.enable_disturb()
    return sess


def _reader(mpcq, sess, name):
    if name == "robots":
        return sess.get_robots()
    if name == "GV_STATE":
        return sess.gait_state()
    read = {"SV": sess.read, "PV": sess.plant_read, "MV": sess.monitor_read, "CV": sess.scenario_read,
            "HV": sess.channel_read, "EV": sess.estimator_read, "DV": sess.disturb_read}[name[:2]]
    return read(getattr(mpcq, name))


@pytest.mark.parametrize("case", list(SM.CASES))
def test_blob_layout(mpcq, eng, case):
    cfg = SM.CASES[case]
    v = WC.session_v_ref(B, 41)
    with _open(mpcq, eng, **cfg) as sess:
        for _ in range(TICKS):
            sess.tick(v)
        with sess.snapshot() as snap:
            blob = snap.tobytes()
        resets = "monitor" in cfg.get("parts", ()) and sess.monitor_params.auto_reset == 1
        header, arrays = SM.layout(N, B, have_order=True, resets=resets, user=TICKS, **cfg)
        version = int.from_bytes(blob[8:12], "little")
        print(case, "version", version, "header", len(header), "blob", len(blob), "model",
              len(header) + sum(nb for _, nb in arrays))
        assert version == SM.CASE_VERSION[case]
        assert blob[:len(header)] == header
        assert len(blob) == len(header) + sum(nb for _, nb in arrays)
        off = len(header)
        for name, nb in arrays:
            if not name.startswith("("):  # a named array: the session's own read, bit for bit
                live = np.ascontiguousarray(_reader(mpcq, sess, name))
                assert live.nbytes == nb, (case, name)
                assert live.tobytes() == blob[off:off + nb], (case, name)
            off += nb
        assert off == len(blob)
        with sess.snapshot_from(blob) as again:
            assert again.k == TICKS and again.batch == B and again.tobytes() == blob
        with pytest.raises(mpcq.MpcqError) as err:
            sess.snapshot_from(blob[:-8])
        assert err.value.code == mpcq._lib.E_INVALID
        other_cfg, diff = OTHER[case]
        with _open(mpcq, eng, **other_cfg) as other, other.snapshot_from(blob) as foreign:
            with pytest.raises(mpcq.MpcqError, match=re.escape("the snapshot's shape is not the session's: " + diff)) as err:
                other.restore(foreign)
            assert err.value.code == mpcq._lib.E_INVALID
