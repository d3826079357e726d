"""What the rigid-body plant (mpcq_session_enable_plant) costs a session's tick.

    python tools/plantbench.py [--batch 1024] [--horizon 16] [--repeats 7] [--ticks 100] [--warmup 8]

C2-size sessions (N = 16, B = 1024, mixed trot / bound / pace, virtual robot, device-resident
v_ref) on one engine, ticked in lockstep, alternating inside every repeat so that clock drift
hits them alike:

  plain    a session that never enabled the plant: the launches every session had before
  toggled  the plant enabled and disabled again before the first tick: the same launches and
           the same solves as `plain` (checked: f0 and iters bit-identical) -- the noise floor
  model    PLANT_MODEL without clamp: the MPC's own step, so the robots end each tick where
           the QP predicted up to OSQP's residual and the solves are nearly `plain`'s -- the
           difference to `plain` is the plant launch and the copy of q_w
  rigid    the default plant (PLANT_RIGID, 20 substeps, Coulomb clamp): the robots no longer
           follow the prediction, so the solves differ too (iters_last_tick shows by how
           much) -- a workload figure, not an overhead figure

and the plant kernel on its own: ``ticks`` back-to-back mpcq_plant_step_batch launches on
device arrays of the same batch (`kernel_rigid`, `kernel_model`, microseconds per launch).

Each figure is the median over ``repeats`` windows of ``ticks`` back-to-back asynchronous
ticks (launches) between two device events, after ``warmup`` ticks (tick 0, cold, among them).
Prints one JSON line.  A run without a HIP device fails; there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mpc-tsid_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=8)
    args = ap.parse_args()
    import torch
    import mpcq
    from mpcq import synth
    if not torch.cuda.is_available():
        raise SystemExit("plantbench needs a HIP device")
    dev = torch.device("cuda", 0)
    B, N = args.batch, args.horizon
    rng = np.random.default_rng(2)
    gaits = np.stack([synth.gait_table(synth.GAITS[b % len(synth.GAITS)], N) for b in range(B)])
    v_ref = np.stack([rng.uniform(-.5, 1, B), rng.uniform(-.3, .3, B), np.zeros(B), np.zeros(B), np.zeros(B),
                      rng.uniform(-.5, .5, B)], axis=1)
    vr = torch.from_numpy(v_ref).to(dev)
    eng = mpcq.Engine(N)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    eng.set_stream(stream.cuda_stream)
    names = ("plain", "toggled", "model", "rigid")
    sess = {n: mpcq.Session(eng, B, gait0=gaits) for n in names}
    sess["toggled"].enable_plant()
    sess["toggled"].disable_plant()
    sess["model"].enable_plant(mpcq.default_plant_params(dt=eng.params.dt, integrator=mpcq.PLANT_MODEL, clamp=0))
    sess["rigid"].enable_plant()

    # the kernel alone: a standing robot under its own weight, on device arrays
    state = np.zeros((B, 12))
    state[:, 2] = 0.2027682
    feet = np.tile([[0.19, 0.19, -0.19, -0.19], [0.15005, -0.15005, 0.15005, -0.15005], [0.0] * 4], (B, 1, 1))
    f = np.tile([0.5, -0.5, eng.params.mass * 9.81 / 4], (B, 4))
    d_state, d_feet, d_f = (torch.from_numpy(a).to(dev) for a in (state, feet, f))
    d_out, d_fe = torch.empty_like(d_state), torch.empty_like(d_f)
    plants = {"kernel_rigid": mpcq.Plant(eng),
              "kernel_model": mpcq.Plant(eng, mpcq.default_plant_params(dt=eng.params.dt,
                                                                         integrator=mpcq.PLANT_MODEL))}

    def tick(name):
        if name in plants:
            plants[name].step_device(B, d_state.data_ptr(), d_feet.data_ptr(), d_f.data_ptr(), d_out.data_ptr(),
                                     d_fe.data_ptr())
        else:
            sess[name].tick_device(vr.data_ptr())

    every = names + tuple(plants)
    for name in every:
        for _ in range(args.warmup):
            tick(name)
    stream.synchronize()
    ms = {n: [] for n in every}
    for rep in range(args.repeats + 1):  # (repeat 0 is a warm-up of the windows' own shape)
        for name in every:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.ticks):
                tick(name)
            e1.record(stream)
            stream.synchronize()
            if rep:
                ms[name].append(e0.elapsed_time(e1) / args.ticks)
    res = {n: (sess[n].read(mpcq.SV_F0), sess[n].read(mpcq.SV_ITERS), sess[n].read(mpcq.SV_STATUS)) for n in names}
    assert np.array_equal(res["plain"][0], res["toggled"][0]) and np.array_equal(res["plain"][1], res["toggled"][1])
    out = {"bench": "session_plant_tick", "batch": B, "horizon": N, "ticks": args.ticks, "repeats": args.repeats,
           "warmup": args.warmup, "build": mpcq.build_info().get("src_sha256")}
    for name in names:
        out[name] = {"ms_per_tick_median": float(np.median(ms[name])), "ms_per_tick_min": min(ms[name]),
                     "ms_per_tick_max": max(ms[name]), "iters_last_tick": int(res[name][1].sum()),
                     "solved": int(np.isin(res[name][2], (1, 2)).sum())}
    for name in plants:
        out[name] = {"us_per_launch_median": 1e3 * float(np.median(ms[name])), "us_per_launch_min": 1e3 * min(ms[name]),
                     "us_per_launch_max": 1e3 * max(ms[name])}
    for name in names[1:]:
        out[f"{name}_over_plain"] = out[name]["ms_per_tick_median"] / out["plain"]["ms_per_tick_median"]
    print(json.dumps(out))
    for s in sess.values():
        s.close()
    eng.close()


if __name__ == "__main__":
    main()
