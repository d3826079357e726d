"""What the scenario stage (mpcq_session_enable_scenario) costs a session's tick.

    python tools/scenariobench.py [--batch 1024] [--horizon 16] [--repeats 5] [--ticks 100] [--warmup 8]

C2-size sessions (N = 16, B = 1024, mixed trot / bound / pace, virtual robot on the default
rigid-body plant, the monitor on) on one engine, run in lockstep, alternating inside every
repeat so that clock drift hits them alike:

  base      the scenario never enabled; its v_ref is a device schedule [ticks][B][6] that
            mpcq.scenario.command restates on the host from `commands`' parameters: the same
            commands tick for tick, so the same solves -- the launches every such session had
            before
  base2     the same again: what `base` shows against itself, the noise floor
  commands  the scenario on, commands only, v_ref = NULL: one more launch per tick
  full      commands + pushes + robots, the monitor's auto-reset on with its default thresholds:
            pushed robots with their own mass and friction move, fall, restart and solve cold
            -- a workload figure, not an overhead figure

(base, base2 and commands run the monitor with its tilt and height tests off and no tick limit:
no episode ends, every robot stays in epoch 1, and the schedule is a function of the tick)

and the scenario kernel on its own: ``ticks`` back-to-back mpcq_scenario_step_batch launches on
device arrays of the same batch with `full`'s parameters (`kernel`, microseconds per launch).

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

COMMANDS = dict(seed=7, commands=1, v_lo=[-0.5, -0.3, -0.5], v_hi=[1.0, 0.3, 0.5], cmd_start=0, cmd_ramp=25,
                cmd_period=100)
FULL = dict(COMMANDS, pushes=1, push_first=20, push_period=50, push_jitter=10, push_ticks=10, push_prob=0.5,
            push_flip=0b000011, wrench_lo=[30.0, 30.0, 0.0, 0.0, 0.0, 0.0], wrench_hi=[60.0, 60.0, 0.0, 0.0, 0.0, 0.0],
            robots=3, mass_scale_lo=0.8, mass_scale_hi=1.4, mu_lo=0.4, mu_hi=1.0)


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
    from mpcq import scenario, synth
    if not torch.cuda.is_available():
        raise SystemExit("scenariobench needs a HIP device")
    dev = torch.device("cuda", 0)
    B, N = args.batch, args.horizon
    gaits = np.stack([synth.gait_table(synth.GAITS[b % len(synth.GAITS)], N) for b in range(B)])
    eng = mpcq.Engine(N)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    eng.set_stream(stream.cuda_stream)
    names = ("base", "base2", "commands", "full")
    sess = {n: mpcq.Session(eng, B, gait0=gaits) for n in names}
    off = dict(max_tilt=np.inf, min_height=-np.inf)
    for n, s in sess.items():
        s.enable_plant()
        s.enable_monitor(**(dict(auto_reset=1) if n == "full" else dict(auto_reset=0, **off)))
    p_cmd = mpcq.default_scenario_params(**COMMANDS)
    p_full = mpcq.default_scenario_params(**FULL)
    sess["commands"].enable_scenario(p_cmd)
    sess["full"].enable_scenario(p_full)
    # base's schedule: every robot in epoch 1, tau = the tick
    total = args.warmup + (args.repeats + 1) * args.ticks
    sched = scenario.command(p_cmd, np.arange(B)[None, :], 1, np.arange(total)[:, None])
    d_sched = torch.from_numpy(np.ascontiguousarray(sched)).to(dev)

    # the kernel alone, on device arrays
    scn = mpcq.Scenario(eng, p_full)
    host = dict(epoch=np.zeros(B, np.int32), tick=np.zeros(B, np.int32), v_ref=np.zeros((B, 6)), push=np.zeros((B, 6)),
                wrench=np.zeros((B, 6)), robots=np.zeros((B, 16)), draw=np.zeros((B, 8)))
    d = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    done = {n: 0 for n in names}

    def run(name, n):
        if name == "kernel":
            for _ in range(n):
                scn.step_device(B, d["epoch"].data_ptr(), d["tick"].data_ptr(), d["v_ref"].data_ptr(),
                                d["push"].data_ptr(), d["wrench"].data_ptr(), robots_out_ptr=d["robots"].data_ptr(),
                                draw_ptr=d["draw"].data_ptr())
        elif name in ("base", "base2"):
            sess[name].run_device(d_sched[done[name]].data_ptr(), n, v_ref_ticks=n)
            done[name] += n
        else:
            sess[name].run_device(0, n)

    every = names + ("kernel",)
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
    # the device's commands are the host's restatement: the three sessions solved the same problems
    for n in ("base2", "commands"):
        assert np.array_equal(res["base"][0], res[n][0]) and np.array_equal(res["base"][1], res[n][1]), n
    assert sess["commands"].scenario_read(mpcq.CV_EPOCH).tolist() == [1] * B
    assert np.array_equal(sess["commands"].scenario_read(mpcq.CV_V_REF), sched[total - 1])
    out = {"bench": "session_scenario_tick", "batch": B, "horizon": N, "ticks": args.ticks, "repeats": args.repeats,
           "warmup": args.warmup, "build": mpcq.build_info().get("src_sha256")}
    for name in names:
        t = sess[name].monitor_read(mpcq.MV_TOTALS)
        out[name] = {"ms_per_tick_median": float(np.median(ms[name])), "ms_per_tick_min": min(ms[name]),
                     "ms_per_tick_max": max(ms[name]), "iters_last_tick": int(res[name][1].sum()),
                     "solved": int(np.isin(res[name][2], (1, 2)).sum()), "episodes": int(t[1])}
    out["full"]["max_epoch"] = int(sess["full"].scenario_read(mpcq.CV_EPOCH).max())
    out["kernel"] = {"us_per_launch_median": 1e3 * float(np.median(ms["kernel"])),
                     "us_per_launch_min": 1e3 * min(ms["kernel"]), "us_per_launch_max": 1e3 * max(ms["kernel"])}
    for name in names[1:]:
        out[f"{name}_over_base"] = out[name]["ms_per_tick_median"] / out["base"]["ms_per_tick_median"]
    print(json.dumps(out))
    for s in sess.values():
        s.close()
    eng.close()


if __name__ == "__main__":
    main()
