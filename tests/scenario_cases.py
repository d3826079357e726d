"""The cases tests/test_gpu_scenario.py runs the scenario kernel on, and the properties of
them it leans on (tests/test_scenario_model.py asserts those on the model alone, on the CPU)."""
import numpy as np

import scenario_model as SM

SEED = 20240607  # the committed seed of the small scenario (coverage() holds under it)
CALLS = 40
BATCHES = (1, 63, 64, 65, 130)
# short periods, so that 40 calls see ramps, holds, three segments and several push windows;
# every range but the (positive) constants straddles zero
SMALL = dict(seed=SEED, commands=1, cmd_start=1, cmd_ramp=3, cmd_period=6,
             v_lo=[-0.3, -0.1, -0.4], v_hi=[0.5, 0.1, 0.4],
             pushes=1, push_first=2, push_period=5, push_jitter=2, push_ticks=2, push_prob=0.5, push_flip=0b000011,
             wrench_lo=[5.0, -8.0, -15.0, -0.3, -0.2, -0.1], wrench_hi=[20.0, 8.0, 5.0, 0.3, 0.2, 0.15],
             robots=3, mass_scale_lo=0.8, mass_scale_hi=1.3, mu_lo=0.5, mu_hi=1.0)
KINDS = ("ramp", "hold", "segment1", "segment2", "active", "inactive_in_occurring", "skipped", "jitter0", "jitter1",
         "jitter2", "flipped", "unflipped", "mid_first")


def base_table(B, seed):
    """Robots that differ: the table the constants are applied to."""
    rng = np.random.default_rng(seed)
    t = np.zeros(B, SM.ROBOT_DTYPE)
    t["mass"] = rng.uniform(2.0, 3.0, B)
    gi = np.diag([3.1e-2, 5.1e-2, 6.9e-2])[None] * rng.uniform(0.8, 1.2, (B, 1, 1))
    gi[:, 0, 1] = gi[:, 1, 0] = -8.0e-7
    t["gI"] = gi
    t["mu"] = rng.uniform(0.6, 1.0, B)
    t["fz_max"] = rng.uniform(20.0, 30.0, B)
    return t


def first_masks(B, seed, calls=CALLS):
    """first [calls][B] int32: call 0 is all_first (its mask is unused and zero); later calls
    restart some robots, about one robot-call in sixteen, and some calls restart nobody."""
    rng = np.random.default_rng(seed)
    m = (rng.random((calls, B)) < 1.0 / 16.0).astype(np.int32)
    m[0] = 0
    m[1::7] = 0
    return m


def wrench(B, seed):
    return np.random.default_rng(seed + 1).uniform(-3.0, 3.0, (B, 6))


def model_calls(p, B, seed, with_base=True, with_wrench=True, calls=CALLS, default_row=None):
    """What the model gives for the calls: a list of dict(v_ref, push, wrench_out, epoch, tick,
    robots, draw, seen) after each call.  Without base the rows are default_row's."""
    masks = first_masks(B, seed, calls)
    base = base_table(B, seed) if with_base else np.full(B, default_row, SM.ROBOT_DTYPE)
    win = wrench(B, seed) if with_wrench else None
    st = SM.new_state(B)
    out = []
    for c in range(calls):
        v, pu, wo, seen = SM.step(p, st, masks[c], c == 0, base, win)
        out.append(dict(v_ref=v, push=pu, wrench_out=wo, epoch=st["epoch"].copy(), tick=st["tick"].copy(),
                        robots=st["robots"].copy(), draw=st["draw"].copy(), seen=seen))
    return out


def coverage(p, results):
    """The kinds of robot-tick the calls contain, by the model alone."""
    kinds = set()
    for c, r in enumerate(results):
        for b, (epoch, tau, is_first) in enumerate(r["seen"]):
            j, t, a = SM.alpha(p, tau)
            if 0.0 < a < 1.0:
                kinds.add("ramp")
            if a == 1.0:
                kinds.add("hold")
            if j in (1, 2):
                kinds.add(f"segment{j}")
            if is_first and c > 0:
                kinds.add("mid_first")
            w = SM.window(p, b, epoch, tau)
            if w is None:
                continue
            if not w["occurs"]:
                kinds.add("skipped")
                continue
            kinds.add(f"jitter{w['jitter']}")
            if w["active"]:
                kinds.add("active")
                kinds.add("flipped" if w["bits"] & 1 else "unflipped")
                kinds.add("flipped" if w["bits"] & 2 else "unflipped")
            else:
                kinds.add("inactive_in_occurring")
    return kinds
