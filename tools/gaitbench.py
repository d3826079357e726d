"""What the gait stage (mpcq_session_enable_gait) costs a session's tick.

    python tools/gaitbench.py [--batch 1024] [--horizon 16] [--repeats 7] [--ticks 100] [--warmup 8]

C2-size sessions (N = 16, B = 1024, mixed trot / bound / pace, virtual robot, device-resident
v_ref) on one engine, ticked in lockstep, alternating inside every repeat so that clock drift
hits them alike:

  plain    the stage never enabled: the launches every such session had before
  plain2   the same again: what `plain` shows against itself, the noise floor
  idle     the stage on, nobody requesting: the gait launch in place of the planner's own roll
           (the results are the plain session's, bit for bit: asserted)
  cycling  every robot's request moves to the next of trot / bound / stand every 24 ticks, from
           a device array: a workload figure (other gaits, other iteration counts), not an
           overhead figure
  speed    MPCQ_GAIT_BY_SPEED on the same v_ref: the selection rule in the launch

and the gait kernel on its own: ``ticks`` back-to-back mpcq_gait_roll_batch launches on device
arrays of the same batch (`kernel`, microseconds per launch), beside the planner's roll alone
(`planner_roll`: mpcq_plan_batch with MPCQ_PLAN_ROLL), which it replaces.

Each figure is the median over ``repeats`` windows of ``ticks`` back-to-back asynchronous
ticks (launches) between two device events, after ``warmup`` ticks (tick 0, cold, among them).
Prints one JSON line.  A run without a HIP device fails; there is no fallback.
"""
import argparse
import ctypes as C
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
        raise SystemExit("gaitbench needs a HIP device")
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
    names = ("plain", "plain2", "idle", "cycling", "speed")
    sess = {n: mpcq.Session(eng, B, gait0=gaits) for n in names}
    lib = ["trot", "bound", "stand"]
    sess["idle"].enable_gait(lib)
    sess["cycling"].enable_gait(lib)
    sess["speed"].enable_gait(["stand", "trot", "bound"], select=mpcq.GAIT_BY_SPEED, thresholds=[0.1, 0.6],
                              hysteresis=0.05)
    ids = [torch.full((B,), g, dtype=torch.int32, device=dev) for g in range(3)]
    count = {"cycling": 0}

    # the kernels alone, on device arrays
    d_gait = torch.from_numpy(gaits.copy()).to(dev)
    d_state = torch.from_numpy(mpcq.gait.new_state(B)).to(dev)
    alone = mpcq.Gait(eng, lib)
    p_gait = torch.from_numpy(gaits.copy()).to(dev)
    zeros = {k: torch.zeros(n, dtype=torch.float64, device=dev) for k, n in
             (("state", B * 12), ("l_feet", B * 12), ("xref", B * 12 * (N + 1)), ("fsteps", B * 260), ("h_rot", B))}
    rot = torch.zeros(B, dtype=torch.int32, device=dev)
    pp = mpcq.default_planner_params(dt=eng.params.dt)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def tick(name):
        if name == "kernel":
            alone.roll_device(B, d_gait.data_ptr(), d_state.data_ptr())
        elif name == "planner_roll":
            eng._call("mpcq_plan_batch", eng._h, C.byref(pp), B, mpcq.PLAN_ROLL, 1, p(zeros["state"]), None, None,
                      p(zeros["l_feet"]), p(vr), None, p(p_gait), p(rot), p(zeros["h_rot"]), p(zeros["xref"]),
                      p(zeros["fsteps"]), None, mpcq.FLAG_DEVICE_PTRS | mpcq.FLAG_ASYNC)
        else:
            if name == "cycling":
                if count[name] % 24 == 0:
                    sess[name].set_gait_device(ids[(count[name] // 24) % 3].data_ptr())
                count[name] += 1
            sess[name].tick_device(vr.data_ptr())

    every = names + ("kernel", "planner_roll")
    torch.cuda.synchronize()
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
    res = {n: (sess[n].read(mpcq.SV_F0), sess[n].read(mpcq.SV_ITERS), sess[n].read(mpcq.SV_STATUS),
               sess[n].read(mpcq.SV_GAIT)) for n in names}
    # the idle stage is the planner's own roll
    for n in ("plain2", "idle"):
        assert all(np.array_equal(res["plain"][i], res[n][i], equal_nan=True) for i in (0, 1, 3)), n
    out = {"bench": "session_gait_tick", "batch": B, "horizon": N, "ticks": args.ticks, "repeats": args.repeats,
           "warmup": args.warmup, "build": mpcq.build_info().get("src_sha256")}
    for name in names:
        out[name] = {"ms_per_tick_median": float(np.median(ms[name])), "ms_per_tick_min": min(ms[name]),
                     "ms_per_tick_max": max(ms[name]), "iters_last_tick": int(res[name][1].sum()),
                     "solved": int(np.isin(res[name][2], (1, 2)).sum())}
        if name in ("cycling", "speed"):
            st = sess[name].gait_state()
            out[name].update(switches=int(st[:, 3].sum()), active=np.bincount(st[:, 1] + 1, minlength=4).tolist())
    for name in ("kernel", "planner_roll"):
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
