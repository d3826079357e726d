"""What a per-instance weights table (mpcq_set_weights) costs the fused solve.

    python tools/weightbench.py [--batch 1024] [--horizon 16] [--repeats 5] [--launches 20]

A C2-size launch (N = 16, B = 1024 synthetic trot instances, device-resident), timed three ways
on one engine, the three alternating inside every repeat so that clock drift hits them alike:

  none     no table: the engine's mpcq_params (the kernel every caller had before)
  same     a table whose every row equals the engine's values: the same QPs and iteration
           counts as `none` (checked: f0 and iters bit-identical), so only the kernel with the
           row fetch (and the robots table of the context's values it reads with it) differs
  random   the randomised table of the tests' recipe (tests/weight_cases.py, seed 900 + N):
           other QPs, other iteration counts -- a workload figure, not an overhead figure; its
           total iteration count is reported next to it

Each figure is the median over ``repeats`` windows of ``launches`` back-to-back asynchronous
calls between two device events, after a warm-up of the same shape.  Prints one JSON line.
A run without a HIP device fails; there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mpc-tsid_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    args = ap.parse_args()
    import torch
    import mpcq
    import weight_cases
    from mpcq import synth
    if not torch.cuda.is_available():
        raise SystemExit("weightbench needs a HIP device")
    dev = torch.device("cuda", 0)
    B, N = args.batch, args.horizon
    syn = synth.make_batch(B, N, gaits=("trot",), seed=0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    xref, fs = T(syn["xref"]), T(syn["fsteps"])
    f0 = torch.empty((B, 12), dtype=torch.float64, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    it = torch.empty(B, dtype=torch.int32, device=dev)
    eng = mpcq.Engine(N)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    tables = {"none": None, "same": mpcq.weights(B, params=eng.params), "random": weight_cases.make_weights(N, B)}

    def call():
        eng.solve_device(B, xref.data_ptr(), fs.data_ptr(), f0.data_ptr(), st.data_ptr(), it.data_ptr(),
                         asynchronous=True)

    ms = {k: [] for k in tables}
    res = {}
    for rep in range(args.repeats + 1):  # (repeat 0 is the warm-up)
        for name, tab in tables.items():
            eng.set_weights(tab)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.launches):
                call()
            e1.record(stream)
            stream.synchronize()
            if rep:
                ms[name].append(e0.elapsed_time(e1) / args.launches)
            else:
                res[name] = (f0.cpu().numpy(), it.cpu().numpy(), st.cpu().numpy())
    assert np.array_equal(res["none"][0], res["same"][0]) and np.array_equal(res["none"][1], res["same"][1])
    out = {"bench": "weights_table_fused_solve", "batch": B, "horizon": N, "launches": args.launches,
           "repeats": args.repeats, "build": mpcq.build_info().get("src_sha256")}
    for name in tables:
        out[name] = {"ms_per_launch_median": float(np.median(ms[name])), "ms_per_launch_min": min(ms[name]),
                     "ms_per_launch_max": max(ms[name]), "iters_total": int(res[name][1].sum()),
                     "solved": int((res[name][2] == 1).sum())}
    out["same_over_none"] = out["same"]["ms_per_launch_median"] / out["none"]["ms_per_launch_median"]
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
