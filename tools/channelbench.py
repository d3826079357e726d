"""What the channel (mpcq_session_enable_channel) costs a session's tick, and its kernels alone.

    python tools/channelbench.py [--batch 1024] [--horizon 16] [--repeats 5] [--ticks 100] [--warmup 8]

C2-size sessions (N = 16, B = 1024, mixed trot / bound / pace, virtual robot on the default
rigid-body plant, the monitor on with its tests off so that no episode ends) on one engine, run
in lockstep, alternating inside every repeat so that clock drift hits them alike:

  never   the channel never enabled: the launches every such session had before
  never2  the same again: what `never` shows against itself, the noise floor
  zero    the channel on at its defaults (all zero): the same solves bit for bit (asserted), so
          the difference is the cost of the two launches
  noisy   a representative channel: two ticks of delay, one of latency, 5 % dropped frames,
          estimator-grade noise and bias, 5 % leg gain, force noise; the monitor's auto-reset on
          with its default thresholds -- a workload figure, not an overhead figure: its
          iteration counts are reported next to it

and each kernel on its own at ``batch`` and at 65,536 robots: ``ticks`` back-to-back launches on
device arrays with `noisy`'s parameters between two events (`observe`, `actuate`: microseconds
per launch), and at 65,536 one device-to-device hipMemcpyAsync in the same process and stream
whose traffic (bytes read plus bytes written) is the kernel's: the yardstick for a stage that
only moves rows.  Per robot and launch in the steady state the observe kernel reads 392 B (truth
96, clock 8, ring slot 96, bias 96, previous observation 96) and writes 200 B (ring slot 96,
observation 96, clock 8); the actuate kernel reads 232 B (f0 96, clock 8, gains 32, ring slot 96)
and writes 192 B (ring slot 96, f_cmd 96).

Each figure is the median over ``repeats`` windows of ``ticks`` ticks enqueued by one
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

NOISY = dict(seed=7, delay=2, latency=1, hold_prob=0.05,
             sigma=[0.002, 0.002, 0.002, 0.005, 0.005, 0.005, 0.01, 0.01, 0.01, 0.02, 0.02, 0.02],
             bias=[0.005, 0.005, 0.002, 0.01, 0.01, 0.01, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
             f_sigma=[0.1, 0.1, 0.2], f_gain=0.05)
BYTES = {"observe": 392 + 200, "actuate": 232 + 192}  # per robot and launch: read + written
BIG = 65536
V_REF = [0.3, 0.0, 0.0, 0.0, 0.0, 0.1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=8)
    args = ap.parse_args()
    import torch
    import mpcq
    from mpcq import channel, synth
    if not torch.cuda.is_available():
        raise SystemExit("channelbench needs a HIP device")
    dev = torch.device("cuda", 0)
    B, N = args.batch, args.horizon
    gaits = np.stack([synth.gait_table(synth.GAITS[b % len(synth.GAITS)], N) for b in range(B)])
    eng = mpcq.Engine(N)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    eng.set_stream(stream.cuda_stream)
    names = ("never", "never2", "zero", "noisy")
    sess = {n: mpcq.Session(eng, B, gait0=gaits) for n in names}
    off = dict(max_tilt=np.inf, min_height=-np.inf)
    for n, s in sess.items():
        s.enable_plant()
        s.enable_monitor(**(dict(auto_reset=1) if n == "noisy" else dict(auto_reset=0, **off)))
    sess["zero"].enable_channel()
    p_noisy = mpcq.default_channel_params(**NOISY)
    sess["noisy"].enable_channel(p_noisy)
    d_vref = torch.from_numpy(np.tile(V_REF, (B, 1))).to(dev)

    # the kernels alone, on device arrays of both sizes; the copy's buffers
    ch = mpcq.Channel(eng, p_noisy)
    sizes = sorted({B, BIG})
    arrs = {}
    for nb in sizes:
        host = dict(channel.new_state(nb), truth=np.random.default_rng(1).standard_normal((nb, 12)),
                    f0=np.random.default_rng(2).standard_normal((nb, 12)) * 10.0)
        arrs[nb] = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
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
                if kind == "observe":
                    ch.observe_device(int(nb), a["truth"].data_ptr(), a["clock"].data_ptr(), a["obs"].data_ptr(),
                                      a["draw"].data_ptr(), a["s_ring"].data_ptr(), a["f_ring"].data_ptr())
                elif kind == "actuate":
                    ch.actuate_device(int(nb), a["f0"].data_ptr(), a["clock"].data_ptr(), a["draw"].data_ptr(),
                                      a["f_ring"].data_ptr(), a["f_cmd"].data_ptr())
                else:  # copy_observe / copy_actuate: one hipMemcpyAsync device to device
                    dst, src = copies[kind[5:]]
                    dst.copy_(src, non_blocking=True)

    alone = [f"{k}@{nb}" for nb in sizes for k in ("observe", "actuate")] + [f"copy_{k}@{BIG}" for k in BYTES]
    every = names + tuple(alone)
    torch.cuda.synchronize()
    for name in every:
        run(name, args.warmup)
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
    # a zero channel is a pass-through: the three sessions solved the same problems
    for n in ("never2", "zero"):
        assert np.array_equal(res["never"][0], res[n][0]) and np.array_equal(res["never"][1], res[n][1]), n
    total = args.warmup + (args.repeats + 1) * args.ticks
    assert sess["zero"].channel_read(mpcq.HV_CLOCK).tolist() == [[1, total]] * B
    out = {"bench": "session_channel_tick", "batch": B, "horizon": N, "ticks": args.ticks, "repeats": args.repeats,
           "warmup": args.warmup, "build": mpcq.build_info().get("src_sha256")}
    for name in names:
        t = sess[name].monitor_read(mpcq.MV_TOTALS)
        out[name] = {"ms_per_tick_median": float(np.median(ms[name])), "ms_per_tick_min": min(ms[name]),
                     "ms_per_tick_max": max(ms[name]), "iters_last_tick": int(res[name][1].sum()),
                     "solved": int(np.isin(res[name][2], (1, 2)).sum()), "episodes": int(t[1])}
    out["noisy"]["max_epoch"] = int(sess["noisy"].channel_read(mpcq.HV_CLOCK)[:, 0].max())
    for name in alone:
        out[name] = {"us_per_launch_median": 1e3 * float(np.median(ms[name])), "us_per_launch_min": 1e3 * min(ms[name]),
                     "us_per_launch_max": 1e3 * max(ms[name])}
    for k, v in BYTES.items():
        out[f"{k}_bytes_per_robot"] = v
        out[f"{k}_over_copy"] = out[f"{k}@{BIG}"]["us_per_launch_median"] / out[f"copy_{k}@{BIG}"]["us_per_launch_median"]
    for name in names[1:]:
        out[f"{name}_over_never"] = out[name]["ms_per_tick_median"] / out["never"]["ms_per_tick_median"]
    out["zero_minus_never_us"] = 1e3 * (out["zero"]["ms_per_tick_median"] - out["never"]["ms_per_tick_median"])
    print(json.dumps(out))
    for s in sess.values():
        s.close()
    eng.close()


if __name__ == "__main__":
    main()
