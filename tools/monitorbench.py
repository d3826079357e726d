"""What the episode monitor (mpcq_session_enable_monitor) costs a session's tick.

    python tools/monitorbench.py [--batch 1024] [--horizon 16] [--repeats 7] [--ticks 100] [--warmup 8]

C2-size sessions (N = 16, B = 1024, mixed trot / bound / pace, virtual robot on the default
rigid-body plant, device-resident v_ref) on one engine, ticked in lockstep, alternating inside
every repeat so that clock drift hits them alike:

  plant    the plant on, the monitor never enabled: the launches every such session had before
  plant2   the same again: what `plant` shows against itself, the noise floor
  monitor  the monitor on, auto_reset = 0, tilt and height tests off: one more launch per tick
  auto     auto_reset = 1, tilt and height tests off: the monitor, and the reset and order
           launches with a mask that is zero unless a solve fails (`episodes` says how often)
  pushed   auto_reset = 1 with the default thresholds and 250 N down on 1/16 of the robots:
           those fall, are restarted and solve cold again -- a workload figure, not an overhead
           figure

and the monitor kernel on its own: ``ticks`` back-to-back mpcq_monitor_step_batch launches on
device arrays of the same batch (`kernel`, microseconds per launch).

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
        raise SystemExit("monitorbench needs a HIP device")
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
    names = ("plant", "plant2", "monitor", "auto", "pushed")
    sess = {n: mpcq.Session(eng, B, gait0=gaits) for n in names}
    for s in sess.values():
        s.enable_plant()
    off = dict(max_tilt=np.inf, min_height=-np.inf)
    sess["monitor"].enable_monitor(auto_reset=0, **off)
    sess["auto"].enable_monitor(auto_reset=1, **off)
    sess["pushed"].enable_monitor(auto_reset=1)
    push = np.zeros((B, 6))
    push[::16, 2] = -250.0
    sess["pushed"].set_wrench(push)

    # the kernel alone: standing robots, solved, on device arrays
    q_w = np.tile([0.0, 0.0, 0.2027682, 0.0, 0.0, 0.0], (B, 1))
    state = np.zeros((B, 12))
    state[:, 2] = 0.2027682
    ep = np.zeros((B, 8))
    ep[:, 4] = np.inf
    host = dict(q_w=q_w, status=np.ones(B, np.int32), iters=np.full(B, 50, np.int32),
                f0=np.tile([0.5, -0.5, 6.0], (B, 4)), cost=np.full((B, 13), 0.1), state=state, v_ref=v_ref, ep=ep,
                ep_ticks=np.zeros(B, np.int32), done=np.zeros(B, np.int32), episodes=np.zeros(B, np.int32),
                last=np.zeros((B, 16)), totals=np.zeros(8, np.uint64).view(np.int64), trace=np.zeros((B, 16)))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in host.items()}
    mon = mpcq.Monitor(eng)

    def tick(name):
        if name == "kernel":
            mon.step_device(B, d["q_w"].data_ptr(), d["status"].data_ptr(), d["iters"].data_ptr(),
                            d["f0"].data_ptr(), d["cost"].data_ptr(), d["state"].data_ptr(), d["v_ref"].data_ptr(),
                            d["ep"].data_ptr(), d["ep_ticks"].data_ptr(), d["done"].data_ptr(),
                            d["episodes"].data_ptr(), d["last"].data_ptr(), d["totals"].data_ptr(),
                            d["trace"].data_ptr())
        else:
            sess[name].tick_device(vr.data_ptr())

    every = names + ("kernel",)
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
    res = {n: (sess[n].read(mpcq.SV_F0), sess[n].read(mpcq.SV_ITERS), sess[n].read(mpcq.SV_STATUS)) for n in names}
    # the monitor changes nothing it looks at
    for n in ("plant2", "monitor"):
        assert np.array_equal(res["plant"][0], res[n][0]) and np.array_equal(res["plant"][1], res[n][1]), n
    out = {"bench": "session_monitor_tick", "batch": B, "horizon": N, "ticks": args.ticks, "repeats": args.repeats,
           "warmup": args.warmup, "build": mpcq.build_info().get("src_sha256")}
    for name in names:
        out[name] = {"ms_per_tick_median": float(np.median(ms[name])), "ms_per_tick_min": min(ms[name]),
                     "ms_per_tick_max": max(ms[name]), "iters_last_tick": int(res[name][1].sum()),
                     "solved": int(np.isin(res[name][2], (1, 2)).sum())}
        if name not in ("plant", "plant2"):
            t = sess[name].monitor_read(mpcq.MV_TOTALS)
            out[name].update(robot_ticks=int(t[0]), episodes=int(t[1]), reasons=[int(v) for v in t[2:7]])
    out["kernel"] = {"us_per_launch_median": 1e3 * float(np.median(ms["kernel"])),
                     "us_per_launch_min": 1e3 * min(ms["kernel"]), "us_per_launch_max": 1e3 * max(ms["kernel"])}
    for name in names[1:]:
        out[f"{name}_over_plant"] = out[name]["ms_per_tick_median"] / out["plant"]["ms_per_tick_median"]
    print(json.dumps(out))
    for s in sess.values():
        s.close()
    eng.close()


if __name__ == "__main__":
    main()
