"""Throughput of the swing kernel (mpcq_swing_batch) for a whole-tick call.

    python tools/swingbench.py [--batches 1024,65536] [--repeats 5] [--launches 500]

Device-resident inputs (the synthetic batch of mpcq.synth: trot / bound / pace tables at
every phase of their period, so about half the feet swing), one call over substeps
0..k_mpc-1 with feet0 = NULL, timed with device events around ``launches`` back-to-back
asynchronous calls after a warm-up of the same shape; ``repeats`` such windows, the median
and the spread reported.  Prints one JSON line per batch size:

  robot_substeps_per_s   B * k_mpc / time per call
  bytes_per_call         what the call must move: gait, fsteps, frame and state in, the
                         references and the state out (computed from the shapes below)
  bytes_per_s            bytes_per_call / time per call -- an achieved rate of required
                         traffic, not a counter reading
A run without a HIP device fails; there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mpc-tsid_amd"))


def required_bytes(B, k_mpc):
    """Bytes one whole-tick call has to read and write for B robots."""
    reads = B * (20 * 5 + 20 * 13 + 3 + 4 * 40) * 8
    writes = B * (k_mpc * 4 * 9 + 4 * 40) * 8
    return reads + writes


def tables(B, seed=0):
    """gait [B][20][5] and fsteps [B][20][13] of the synthetic batch."""
    from mpcq import synth
    fs = synth.make_batch(B, 16, gaits=synth.GAITS, seed=seed)["fsteps"]
    gait = np.zeros((B, 20, 5))
    gait[:, :, 0] = fs[:, :, 0]
    gait[:, :, 1:] = ~np.isnan(fs[:, :, 1::3]) & (fs[:, :, 0:1] != 0)
    return gait, fs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,65536")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=500)
    args = ap.parse_args()
    import torch
    import mpcq
    if not torch.cuda.is_available():
        raise SystemExit("swingbench needs a HIP device")
    dev = torch.device("cuda", 0)
    eng = mpcq.Engine(16)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    for B in (int(b) for b in args.batches.split(",")):
        rng = np.random.default_rng(1)
        gait, fs = tables(B)
        sw = mpcq.Swing(eng, B)
        k_mpc = int(sw.params.k_mpc)
        frame = np.column_stack([rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(-3, 3, B)])
        d = dict(gait=T(gait), fsteps=T(fs), frame=T(frame), state=T(np.zeros((B, 4, 40))))
        ref = torch.empty((B, k_mpc, 4, 9), dtype=torch.float64, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)

        def call():
            sw.advance_device(d["gait"].data_ptr(), d["fsteps"].data_ptr(), d["frame"].data_ptr(),
                              d["state"].data_ptr(), ref.data_ptr(), 0, k_mpc, status_ptr=status.data_ptr())

        for _ in range(3):  # warm-up of the timed shape
            call()
        stream.synchronize()
        assert not status.cpu().numpy().any()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.launches):
                call()
            e1.record(stream)
            stream.synchronize()
            ms.append(e0.elapsed_time(e1) / args.launches)
        t = float(np.median(ms)) * 1e-3
        nb = required_bytes(B, k_mpc)
        print(json.dumps({
            "bench": "swing_whole_tick", "batch": B, "k_mpc": k_mpc,
            "swing_feet_fraction": float((gait[:, 0, 1:] == 0).mean()),
            "ms_per_call_median": t * 1e3, "ms_per_call_min": min(ms), "ms_per_call_max": max(ms),
            "robot_substeps_per_s": B * k_mpc / t, "bytes_per_call": nb, "bytes_per_s": nb / t,
            "build": mpcq.build_info().get("src_sha256"),
        }))
    eng.close()


if __name__ == "__main__":
    main()
