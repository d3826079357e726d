"""What the estimator (mpcq_session_enable_estimator) costs a session's tick, its kernel alone, and
what it buys a session behind a noisy, delayed channel.

    python tools/estimatorbench.py [--batch 1024] [--horizon 16] [--repeats 5] [--ticks 100] [--warmup 8]
                                   [--workload-ticks 300]

C2-size sessions (N = 16, B = 1024, mixed trot / bound / pace, the default rigid-body plant, the
monitor on with its tests off so that no episode ends) on one engine, run in lockstep, alternating
inside every repeat so that clock drift hits them alike:

  never    the estimator never enabled: the launches every such session had before
  never2   the same again: what `never` shows against itself, the noise floor
  enabled  the estimator on at lag 0 over the exact state (no channel): one more launch per tick

and the kernel on its own at ``batch`` and at 65,536 robots, at lag 0 and at lag 8 / f_lag 4:
``ticks`` back-to-back launches on device arrays between two events (microseconds per launch), and
at 65,536 one device-to-device hipMemcpyAsync in the same process and stream whose traffic (bytes
read plus bytes written) is the kernel's.  Per robot and launch in the steady state the kernel
reads 640 B (observation 96, previous row 96, posterior 96, P 144, clock 16, f_prev 96, feet 96)
plus 192 B for the time update's two slot halves and 192 B per forecast step, and writes 640 B
(posterior 96, previous row 96, P 144, clock 16, estimate 96, ring slot 192): 1472 B at lag 0,
3008 B at lag 8.  The forecast is a dependent chain of model steps: at lag 8 the launch's cost is
latency, not traffic.

The workload figure (``--workload-ticks`` > 0): two more sessions of ``batch`` robots on the
default plant behind the same channel (delay 2, latency 1, sigma 1e-3 on the pose and 1e-2 on the
rates), the monitor's auto-reset on with its default thresholds, one with the estimator (lag 2,
f_lag 1, r = sigma^2) and one without: the monitor's episode totals and the mean over ticks and
robots of |x_robot[:, 0] - PV_STATE_END| per component (how far the MPC's one-step prediction is
from what the plant did).

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
LAGS = {"lag0": (0, 0), "lag8": (8, 4)}
BYTES = {"lag0": 640 + 192 + 640, "lag8": 640 + 192 + 8 * 192 + 640}  # per robot and launch: read + written
BIG = 65536
V_REF = [0.3, 0.0, 0.0, 0.0, 0.0, 0.1]


def workload(mpcq, eng, B, gaits, ticks):
    out = {}
    for name in ("channel_only", "with_estimator"):
        s = mpcq.Session(eng, B, gait0=gaits)
        s.enable_plant()
        s.enable_monitor(auto_reset=1)
        s.enable_channel(**CHANNEL)
        if name == "with_estimator":
            s.enable_estimator(lag=CHANNEL["delay"], f_lag=CHANNEL["latency"], r=[v * v for v in SIGMA])
        err, n = np.zeros(12), 0
        for _ in range(ticks):
            s.tick(V_REF)
            ok = np.isin(s.read(mpcq.SV_STATUS), (1, 2)) & (s.monitor_read(mpcq.MV_DONE) == 0)
            d = np.abs(s.read(mpcq.SV_X_ROBOT)[:, :, 0] - s.plant_read(mpcq.PV_STATE_END))[ok]
            err += d.sum(axis=0)
            n += int(ok.sum())
        t = s.monitor_read(mpcq.MV_TOTALS)
        out[name] = {"totals": [int(v) for v in t], "robot_ticks": n,
                     "mean_abs_prediction_error": [float(v) for v in err / max(n, 1)]}
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--workload-ticks", type=int, default=300)
    args = ap.parse_args()
    import torch
    import mpcq
    from mpcq import estimator, synth
    if not torch.cuda.is_available():
        raise SystemExit("estimatorbench needs a HIP device")
    dev = torch.device("cuda", 0)
    B, N = args.batch, args.horizon
    gaits = np.stack([synth.gait_table(synth.GAITS[b % len(synth.GAITS)], N) for b in range(B)])
    eng = mpcq.Engine(N)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    eng.set_stream(stream.cuda_stream)
    names = ("never", "never2", "enabled")
    sess = {n: mpcq.Session(eng, B, gait0=gaits) for n in names}
    for s in sess.values():
        s.enable_plant()
        s.enable_monitor(auto_reset=0, max_tilt=np.inf, min_height=-np.inf)
    sess["enabled"].enable_estimator()
    d_vref = torch.from_numpy(np.tile(V_REF, (B, 1))).to(dev)

    # the kernel alone, on device arrays of both sizes; the copy's buffers
    # (skip_repeats off: the window's observation does not change, and every tick shall update)
    est = {k: mpcq.Estimator(eng, mpcq.default_estimator_params(lag=v[0], f_lag=v[1], skip_repeats=0))
           for k, v in LAGS.items()}
    sizes = sorted({B, BIG})
    arrs = {}
    for nb in sizes:
        rng = np.random.default_rng(nb)
        obs = np.zeros((nb, 12))
        obs[:, 2] = 0.2
        host = dict(obs=obs, f_prev=np.tile([0.0, 0.0, 6.0], (nb, 4)) + 0.1 * rng.standard_normal((nb, 12)),
                    feet=np.tile([0.19, 0.19, -0.19, -0.19, 0.15, -0.15, 0.15, -0.15, 0.0, 0.0, 0.0, 0.0], (nb, 1)),
                    est=np.zeros((nb, 12)))
        arrs[nb] = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
        for k in LAGS:
            arrs[nb]["row_" + k] = torch.from_numpy(estimator.new_rows(nb)).to(dev)
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
                if kind in LAGS:
                    est[kind].step_device(int(nb), a["obs"].data_ptr(), a["f_prev"].data_ptr(), a["feet"].data_ptr(),
                                          a["row_" + kind].data_ptr(), a["est"].data_ptr())
                else:  # copy_lag0 / copy_lag8: one hipMemcpyAsync device to device
                    dst, src = copies[kind[5:]]
                    dst.copy_(src, non_blocking=True)

    alone = [f"{k}@{nb}" for nb in sizes for k in LAGS] + [f"copy_{k}@{BIG}" for k in BYTES]
    every = names + tuple(alone)
    torch.cuda.synchronize()
    for name in every:
        run(name, max(args.warmup, 16))  # (the kernel alone: past the first 12 ticks, every slot read)
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
    assert np.array_equal(res["never"][0], res["never2"][0]) and np.array_equal(res["never"][1], res["never2"][1])
    total = max(args.warmup, 16) + (args.repeats + 1) * args.ticks
    ck = estimator.unpack(sess["enabled"].estimator_read(mpcq.EV_ROW))
    for k in LAGS:  # the kernel alone ran in its steady state: no robot initialised after tick 0
        assert (estimator.unpack(arrs[B]["row_" + k].cpu().numpy())["tau_next"] == total).all(), k
    out = {"bench": "session_estimator_tick", "batch": B, "horizon": N, "ticks": args.ticks, "repeats": args.repeats,
           "warmup": args.warmup, "build": mpcq.build_info().get("src_sha256")}
    for name in names:
        out[name] = {"ms_per_tick_median": float(np.median(ms[name])), "ms_per_tick_min": min(ms[name]),
                     "ms_per_tick_max": max(ms[name]), "iters_last_tick": int(res[name][1].sum()),
                     "solved": int(np.isin(res[name][2], (1, 2)).sum())}
    out["enabled"]["least_tau_next"] = int(ck["tau_next"].min())
    for name in alone:
        out[name] = {"us_per_launch_median": 1e3 * float(np.median(ms[name])), "us_per_launch_min": 1e3 * min(ms[name]),
                     "us_per_launch_max": 1e3 * max(ms[name])}
    for k, v in BYTES.items():
        out[f"{k}_bytes_per_robot"] = v
        out[f"{k}_over_copy"] = out[f"{k}@{BIG}"]["us_per_launch_median"] / out[f"copy_{k}@{BIG}"]["us_per_launch_median"]
    for name in names[1:]:
        out[f"{name}_over_never"] = out[name]["ms_per_tick_median"] / out["never"]["ms_per_tick_median"]
    out["enabled_minus_never_us"] = 1e3 * (out["enabled"]["ms_per_tick_median"] - out["never"]["ms_per_tick_median"])
    for s in sess.values():
        s.close()
    if args.workload_ticks > 0:
        eng.set_stream(0)
        out["workload"] = dict(workload(mpcq, eng, B, gaits, args.workload_ticks), ticks=args.workload_ticks,
                               channel=CHANNEL)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
