"""What the disturbance stage (mpcq_session_enable_disturb) costs a session's tick, its kernel
alone, and what it buys a session whose robots carry payloads and are pushed.

    python tools/disturbbench.py [--batch 1024] [--horizon 16] [--repeats 7] [--ticks 100] [--warmup 8]
                                 [--workload-ticks 300]

C2-size sessions (N = 16, B = 1024, mixed trot / bound / pace, the default rigid-body plant, the
monitor on with its tests off so that no episode ends) on one engine, run in lockstep, alternating
inside every repeat so that clock drift hits them alike:

  never     the stage never enabled: the launches every such session had before (the plain kernels)
  never2    the same again: what `never` shows against itself, the noise floor
  estimate  the stage on with compensate = 0: one more launch per tick, the solve untouched
  enabled   the stage on with compensate = 1: the solve reads MPCQ_DV_DIST, through the engine's
            per-instance-table (ROB) kernels, and solves other problems

and the kernel on its own at ``batch`` and at 65,536 robots, at f_lag 0 and at f_lag 4: ``ticks``
back-to-back launches on device arrays between two events (microseconds per launch), and at
65,536 one device-to-device hipMemcpyAsync in the same process and stream whose traffic (bytes
read plus bytes written) is the kernel's.  Per robot and launch in the steady state the kernel
reads 448 B (measurement 96, previous row 96, d 48, clock 16, f_prev 96, feet 96; at f_lag > 0 the
acting force's slot, 96 more) and writes 368 B (previous row 96, d 48, clock 16, ring slot 96, the
output row 64, the sample 48): 816 B at f_lag 0, 912 B at f_lag 4.

The workload figure (``--workload-ticks`` > 0) is DESIGN.md section 4.14's, with the scenario's
payloads and pushes on top: two sessions of ``batch`` robots on the default plant behind the
channel (delay 2, latency 1, sigma 1e-3 on the pose and 1e-2 on the rates) with the estimator
(lag 2, f_lag 1, r = sigma^2), the scenario drawing a true mass of 1.0 to 1.4 times the model's
and pushes of up to 4 N per episode, the monitor's auto-reset on with its default thresholds; one
with the stage (f_lag 1, the default gains) and one without: the monitor's episode totals and the
mean over the solved, running robot-ticks of |z - h_ref|, |roll|, |pitch| and |vx - v_ref| of the
true state.

Each timing is the median over ``repeats`` windows of ``ticks`` ticks enqueued by one
mpcq_session_run between two device events, after ``warmup`` ticks (tick 0, cold, among them).
Prints one JSON line.  A run without a HIP device fails; there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mpc-tsid_amd"))

SIGMA = [1e-3] * 6 + [1e-2] * 6
CHANNEL = dict(seed=7, delay=2, latency=1, sigma=SIGMA)
SCENARIO = dict(seed=11, commands=0, pushes=1, push_first=10, push_period=40, push_jitter=10, push_ticks=15,
                push_prob=1.0, wrench_lo=[-4.0, -4.0, 0.0, 0.0, 0.0, 0.0], wrench_hi=[4.0, 4.0, 0.0, 0.0, 0.0, 0.0],
                robots=1, mass_scale_lo=1.0, mass_scale_hi=1.4, mu_lo=0.9, mu_hi=0.9)
F_LAGS = {"flag0": 0, "flag4": 4}
BYTES = {"flag0": 448 + 368, "flag4": 544 + 368}  # per robot and launch: read + written
BIG = 65536
V_REF = [0.3, 0.0, 0.0, 0.0, 0.0, 0.1]
H_REF = 0.2027682


def workload(mpcq, eng, B, gaits, ticks):
    out = {}
    for name in ("without_stage", "with_stage"):
        s = mpcq.Session(eng, B, gait0=gaits)
        s.enable_plant()
        s.enable_monitor(auto_reset=1)
        s.enable_scenario(**SCENARIO)
        s.enable_channel(**CHANNEL)
        s.enable_estimator(lag=CHANNEL["delay"], f_lag=CHANNEL["latency"], r=[v * v for v in SIGMA])
        if name == "with_stage":
            s.enable_disturb(f_lag=CHANNEL["latency"])
        err, n = np.zeros(4), 0
        for _ in range(ticks):
            s.tick(V_REF)
            ok = np.isin(s.read(mpcq.SV_STATUS), (1, 2)) & (s.monitor_read(mpcq.MV_DONE) == 0)
            x = s.read(mpcq.SV_STATE)[ok]
            err += np.abs(np.stack([x[:, 2] - H_REF, x[:, 3], x[:, 4], x[:, 6] - V_REF[0]], axis=1)).sum(axis=0)
            n += int(ok.sum())
        t = s.monitor_read(mpcq.MV_TOTALS)
        out[name] = {"totals": [int(v) for v in t], "robot_ticks": n,
                     "mean_abs_error_z_roll_pitch_vx": [float(v) for v in err / max(n, 1)]}
        if name == "with_stage":
            d = s.disturb_read(mpcq.DV_DIST)["a"]
            out[name]["mean_abs_d"] = [float(v) for v in np.abs(d).mean(axis=0)]
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--workload-ticks", type=int, default=300)
    args = ap.parse_args()
    import torch
    import mpcq
    from mpcq import disturb, synth
    if not torch.cuda.is_available():
        raise SystemExit("disturbbench needs a HIP device")
    dev = torch.device("cuda", 0)
    B, N = args.batch, args.horizon
    gaits = np.stack([synth.gait_table(synth.GAITS[b % len(synth.GAITS)], N) for b in range(B)])
    eng = mpcq.Engine(N)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    eng.set_stream(stream.cuda_stream)
    names = ("never", "never2", "estimate", "enabled")
    sess = {n: mpcq.Session(eng, B, gait0=gaits) for n in names}
    for s in sess.values():
        s.enable_plant()
        s.enable_monitor(auto_reset=0, max_tilt=np.inf, min_height=-np.inf)
    sess["estimate"].enable_disturb(compensate=0)
    sess["enabled"].enable_disturb()
    d_vref = torch.from_numpy(np.tile(V_REF, (B, 1))).to(dev)

    # the kernel alone, on device arrays of both sizes; the copy's buffers
    # (skip_repeats off: the window's measurement does not change, and every tick shall sample)
    kern = {k: mpcq.Disturb(eng, mpcq.default_disturb_params(f_lag=v, skip_repeats=0)) for k, v in F_LAGS.items()}
    sizes = sorted({B, BIG})
    arrs = {}
    for nb in sizes:
        rng = np.random.default_rng(nb)
        meas = np.zeros((nb, 12))
        meas[:, 2] = 0.2
        host = dict(meas=meas, f_prev=np.tile([0.0, 0.0, 6.0], (nb, 4)) + 0.1 * rng.standard_normal((nb, 12)),
                    feet=np.tile([0.19, 0.19, -0.19, -0.19, 0.15, -0.15, 0.15, -0.15, 0.0, 0.0, 0.0, 0.0], (nb, 1)),
                    dist=np.zeros((nb, 8)), resid=np.zeros((nb, 6)))
        arrs[nb] = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
        for k in F_LAGS:
            arrs[nb]["row_" + k] = torch.from_numpy(disturb.new_rows(nb)).to(dev)
    copies = {k: (torch.empty(BIG * v // 2, dtype=torch.uint8, device=dev), torch.zeros(BIG * v // 2, dtype=torch.uint8, device=dev))
              for k, v in BYTES.items()}

    def run(name, n):
        if name in sess:
            sess[name].run_device(d_vref.data_ptr(), n)
            return
        kind, nb = name.split("@")
        a = arrs.get(int(nb))
        with torch.cuda.stream(stream):
            for _ in range(n):
                if kind in F_LAGS:
                    kern[kind].step_device(int(nb), a["meas"].data_ptr(), a["f_prev"].data_ptr(), a["feet"].data_ptr(),
                                           a["row_" + kind].data_ptr(), a["dist"].data_ptr(), a["resid"].data_ptr())
                else:  # copy_flag0 / copy_flag4: one hipMemcpyAsync device to device
                    dst, src = copies[kind[5:]]
                    dst.copy_(src, non_blocking=True)

    alone = [f"{k}@{nb}" for nb in sizes for k in F_LAGS] + [f"copy_{k}@{BIG}" for k in BYTES]
    every = names + tuple(alone)
    torch.cuda.synchronize()
    for name in every:
        run(name, max(args.warmup, 16))
    stream.synchronize()
    ms = {n: [] for n in every}
    for rep in range(args.repeats + 1):  # (repeat 0 is a warm-up of the windows' own shape)
        for name in every:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run(name, args.ticks)
            e1.record(stream)
            stream.synchronize()
            if rep:
                ms[name].append(e0.elapsed_time(e1) / args.ticks)
    res = {n: (sess[n].read(mpcq.SV_F0), sess[n].read(mpcq.SV_ITERS), sess[n].read(mpcq.SV_STATUS)) for n in names}
    for other in ("never2", "estimate"):  # (estimating alone changes no bit of the loop)
        assert np.array_equal(res["never"][0], res[other][0]) and np.array_equal(res["never"][1], res[other][1]), other
    total = max(args.warmup, 16) + (args.repeats + 1) * args.ticks
    for k in F_LAGS:  # the kernel alone ran in its steady state: no robot ran a first tick after tick 0
        assert (disturb.unpack(arrs[B]["row_" + k].cpu().numpy())["tau_next"] == total).all(), k
    out = {"bench": "session_disturb_tick", "batch": B, "horizon": N, "ticks": args.ticks, "repeats": args.repeats,
           "warmup": args.warmup, "build": mpcq.build_info().get("src_sha256")}
    for name in names:
        out[name] = {"ms_per_tick_median": float(np.median(ms[name])), "ms_per_tick_min": min(ms[name]),
                     "ms_per_tick_max": max(ms[name]), "iters_last_tick": int(res[name][1].sum()),
                     "solved": int(np.isin(res[name][2], (1, 2)).sum())}
    for name in ("estimate", "enabled"):
        out[name]["least_tau_next"] = int(disturb.unpack(sess[name].disturb_read(mpcq.DV_ROW))["tau_next"].min())
        out[name]["mean_abs_d"] = [float(v) for v in np.abs(sess[name].disturb_read(mpcq.DV_DIST)["a"]).mean(axis=0)]
    for name in alone:
        out[name] = {"us_per_launch_median": 1e3 * float(np.median(ms[name])), "us_per_launch_min": 1e3 * min(ms[name]),
                     "us_per_launch_max": 1e3 * max(ms[name])}
    for k, v in BYTES.items():
        out[f"{k}_bytes_per_robot"] = v
        out[f"{k}_over_copy"] = out[f"{k}@{BIG}"]["us_per_launch_median"] / out[f"copy_{k}@{BIG}"]["us_per_launch_median"]
    for name in names[1:]:
        out[f"{name}_over_never"] = out[name]["ms_per_tick_median"] / out["never"]["ms_per_tick_median"]
    out["estimate_minus_never_us"] = 1e3 * (out["estimate"]["ms_per_tick_median"] - out["never"]["ms_per_tick_median"])
    for s in sess.values():
        s.close()
    if args.workload_ticks > 0:
        eng.set_stream(0)
        out["workload"] = dict(workload(mpcq, eng, B, gaits, args.workload_ticks), ticks=args.workload_ticks,
                               channel=CHANNEL, scenario=SCENARIO)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
