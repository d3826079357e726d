"""What saving, restoring and forking a session's robots costs (mpcq_session_snapshot_*).

    python tools/snapshotbench.py [--batches 1024,65536] [--horizon 16] [--repeats 5] [--inner 10] [--warmup 4]

Sessions with everything enabled (N = 16, mixed trot / bound / pace, swing, the rigid plant with
a table and a wrench, the monitor with auto-reset, a scenario, a model table), ticked ``warmup``
times, then per batch size, alternating inside every repeat:

  save      mpcq_session_snapshot_save: whole-array device-to-device copies
  restore   mpcq_session_snapshot_restore with map == NULL (the identity): one gather launch, the
            totals' copy and the order launch
  random    the same with a random map on the device (duplicates, no -1)
  fork      mpcq_session_fork(r): save into the session's own snapshot + restore of one row
  memcpy    the yardstick: ONE plain hipMemcpyAsync device to device of the snapshot's byte count
            (for fork: of twice that), in the same process on the same stream

Each figure is a window of ``inner`` back-to-back asynchronous calls between two device events,
divided by ``inner``: median (min - max) over ``repeats`` windows, in microseconds.  Prints one
JSON line.  A run without a HIP device fails; there is no fallback.
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
    ap.add_argument("--batches", default="1024,65536")
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    args = ap.parse_args()
    import torch
    import mpcq
    from mpcq import _lib as L
    from mpcq import synth
    if not torch.cuda.is_available():
        raise SystemExit("snapshotbench needs a HIP device")
    dev = torch.device("cuda", 0)
    N = args.horizon
    eng = mpcq.Engine(N)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    eng.set_stream(stream.cuda_stream)
    hip = L._preload_hip_runtime() or C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    out = {"bench": "session_snapshot", "horizon": N, "repeats": args.repeats, "inner": args.inner,
           "warmup": args.warmup, "build": mpcq.build_info().get("src_sha256"), "batches": {}}
    for B in [int(x) for x in args.batches.split(",")]:
        rng = np.random.default_rng(2)
        gaits = np.stack([synth.gait_table(synth.GAITS[b % len(synth.GAITS)], N) for b in range(B)])
        sess = mpcq.Session(eng, B, gait0=gaits)
        sess.enable_swing()
        sess.enable_plant()
        sess.set_wrench(np.where(np.arange(B)[:, None] % 7 == 0, [4.0, -2.0, 0.0, 0.0, 0.0, 0.1], 0.0))
        sess.set_robots(mpcq.robots(B, mass=rng.uniform(2.3, 2.7, B)))
        sess.set_plant_robots(mpcq.robots(B, mass=rng.uniform(2.2, 2.9, B), mu=rng.uniform(0.6, 1.0, B)))
        sess.enable_monitor(max_ticks=50, auto_reset=1)
        sess.enable_scenario()
        for _ in range(args.warmup):
            sess.tick_device(0)
        snap = sess.snapshot()
        nbytes = snap.nbytes() - 128  # without the blob's header
        d_map = torch.from_numpy(rng.integers(0, B, B).astype(np.int32)).to(dev)
        d_one = torch.full((B,), B // 3, dtype=torch.int32, device=dev)
        y_src = torch.zeros(2 * nbytes, dtype=torch.uint8, device=dev)
        y_dst = torch.empty(2 * nbytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def memcpy(n):
            rc = hip.hipMemcpyAsync(y_dst.data_ptr(), y_src.data_ptr(), n, 3, stream.cuda_stream)  # device to device
            assert rc == 0, rc

        ops = {
            "save": lambda: eng._call("mpcq_session_snapshot_save", sess._h, snap._h, L.FLAG_ASYNC),
            "memcpy": lambda: memcpy(nbytes),
            "restore": lambda: sess.restore_device(snap, 0),
            "random": lambda: sess.restore_device(snap, d_map.data_ptr()),
            "fork": lambda: sess.fork_device(d_one.data_ptr()),
            "memcpy_x2": lambda: memcpy(2 * nbytes),
        }
        us = {n: [] for n in ops}
        for rep in range(args.repeats + 1):  # (repeat 0 is a warm-up of the windows' own shape)
            for name, op in ops.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.inner):
                    op()
                e1.record(stream)
                stream.synchronize()
                if rep:
                    us[name].append(1e3 * e0.elapsed_time(e1) / args.inner)
        res = {"bytes": nbytes, "bytes_per_robot": (nbytes - 64) // B}  # (64: the batch-wide MV_TOTALS)
        for name in ops:
            med = float(np.median(us[name]))
            res[name] = {"us_median": med, "us_min": min(us[name]), "us_max": max(us[name])}
        for name, yard, moved in (("save", "memcpy", 2 * nbytes), ("restore", "memcpy", 2 * nbytes),
                                  ("random", "memcpy", 2 * nbytes), ("fork", "memcpy_x2", 4 * nbytes)):
            res[name]["over_memcpy"] = res[name]["us_median"] / res[yard]["us_median"]
            res[name]["tb_per_s_read_plus_written"] = moved / res[name]["us_median"] * 1e-6
        res["memcpy"]["tb_per_s_read_plus_written"] = 2 * nbytes / res["memcpy"]["us_median"] * 1e-6
        out["batches"][str(B)] = res
        snap.close()
        sess.close()
        del y_src, y_dst
        torch.cuda.empty_cache()
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
