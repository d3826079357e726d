"""What the per-robot reset (mpcq_session_reset) costs a session's tick.

    python tools/resetbench.py [--batch 1024] [--horizon 16] [--repeats 7] [--ticks 100] [--warmup 8]

C2-size sessions (N = 16, B = 1024, mixed trot / bound / pace, virtual robot, device-resident
v_ref) on one engine, three of them ticked in lockstep, alternating inside every repeat so that
clock drift hits them alike:

  never    a session on which reset was never called: the launches every session had before
  zero     the same session after one reset with an all-zero mask: the ticks consult
           MPCQ_SV_FIRST and launch the planner's extra pass, but no robot is first -- the
           same solves as `never` (checked: f0 and iters bit-identical), so only the flag
           reads and the one extra launch differ
  rolling  1/16 of the robots reset before every tick from a mask on the device (robot b at
           the ticks with b % 16 == tick % 16), reset call included in the timed window:
           other solves (a cold one per robot every 16 ticks) -- a workload figure, not an
           overhead figure

Each figure is the median over ``repeats`` windows of ``ticks`` back-to-back asynchronous
ticks between two device events, after ``warmup`` ticks (tick 0, cold, among them).  Prints
one JSON line.  A run without a HIP device fails; there is no fallback.
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
        raise SystemExit("resetbench needs a HIP device")
    dev = torch.device("cuda", 0)
    B, N = args.batch, args.horizon
    rng = np.random.default_rng(2)
    gaits = np.stack([synth.gait_table(synth.GAITS[b % len(synth.GAITS)], N) for b in range(B)])
    v_ref = np.stack([rng.uniform(-.5, 1, B), rng.uniform(-.3, .3, B), np.zeros(B), np.zeros(B), np.zeros(B),
                      rng.uniform(-.5, .5, B)], axis=1)
    vr = torch.from_numpy(v_ref).to(dev)
    masks = [(torch.arange(B, device=dev) % 16 == j).to(torch.int32) for j in range(16)]
    zero = torch.zeros(B, dtype=torch.int32, device=dev)
    eng = mpcq.Engine(N)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    eng.set_stream(stream.cuda_stream)
    names = ("never", "zero", "rolling")
    sess = {n: mpcq.Session(eng, B, gait0=gaits) for n in names}

    def tick(name):
        s = sess[name]
        if name == "rolling" and s.k >= args.warmup:
            s.reset_device(mask_ptr=masks[s.k % 16].data_ptr())
        s.tick_device(vr.data_ptr())

    for name in names:
        for _ in range(args.warmup):
            tick(name)
    sess["zero"].reset_device(mask_ptr=zero.data_ptr())
    stream.synchronize()
    ms = {n: [] for n in names}
    for rep in range(args.repeats + 1):  # (repeat 0 is a warm-up of the windows' own shape)
        for name in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.ticks):
                tick(name)
            e1.record(stream)
            stream.synchronize()
            if rep:
                ms[name].append(e0.elapsed_time(e1) / args.ticks)
    res = {n: (sess[n].read(mpcq.SV_F0), sess[n].read(mpcq.SV_ITERS), sess[n].read(mpcq.SV_STATUS)) for n in names}
    assert np.array_equal(res["never"][0], res["zero"][0]) and np.array_equal(res["never"][1], res["zero"][1])
    out = {"bench": "session_reset_tick", "batch": B, "horizon": N, "ticks": args.ticks, "repeats": args.repeats,
           "warmup": args.warmup, "build": mpcq.build_info().get("src_sha256")}
    for name in names:
        out[name] = {"ms_per_tick_median": float(np.median(ms[name])), "ms_per_tick_min": min(ms[name]),
                     "ms_per_tick_max": max(ms[name]), "iters_last_tick": int(res[name][1].sum()),
                     "solved": int(np.isin(res[name][2], (1, 2)).sum())}
    out["zero_over_never"] = out["zero"]["ms_per_tick_median"] / out["never"]["ms_per_tick_median"]
    out["rolling_over_never"] = out["rolling"]["ms_per_tick_median"] / out["never"]["ms_per_tick_median"]
    print(json.dumps(out))
    for s in sess.values():
        s.close()
    eng.close()


if __name__ == "__main__":
    main()
