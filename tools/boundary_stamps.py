"""One check-segment boundary of the N <= 32 ADMM loop, phase by phase (stamps build).

    MPCQ_LIB_VARIANT=stamps python tools/boundary_stamps.py [--N 16] [--copies 256 512] [--iters 2000]

tools/checkcost.py's experiment on a stamps build (csrc/Makefile `stamps`, or a stamps variant of
tools/build_variant.sh with -DMPCQ_STAMPS): copies of one C2 instance, adaptive rho off and
tolerances out of reach, so every configuration runs exactly --iters iterations; once with
check_termination 0 and once with 25.  The stamps accumulate per bucket over the launch, so a
bucket's difference between the two runs, per check, is what one boundary adds to it:

* 4   infeas_cheap up to its publication barrier (from the checked iteration's end)
* 5   update_info, first part: the primal rows (rowA, the first butterfly)
* 8   update_info, second part: the dual columns, the wave reduction, the barrier after it
* 11  update_info, third part (info_combine, its closing barrier) and the decision
* 15  the operands' refill at the top of the next segment (launder, the offsets, load_rhs_ops)
      up to ph_rhs's own barrier: the excess of the segment's first ph_rhs over a plain one
* 3 + 6 + 7 + 9 + 10  the checked (DELTA) iteration's excess over a plain one after that point
      (the constant block's loads, delta_y / delta_x kept)

Cycles are s_memtime's; the launch's own ratio of stamped cycles to kernel time converts them
to nanoseconds.  The stamps themselves cost a few instructions per point, so the sum runs above
tools/checkcost.py's figure on the production build.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mpc-tsid_amd"))
os.environ.setdefault("MPCQ_LIB_VARIANT", "stamps")

ROWS = (("DELTA iteration's excess (3+6+7+9+10)", (3, 6, 7, 9, 10)),
        ("infeas_cheap to its barrier (4)", (4,)),
        ("update_info 1: primal rows (5)", (5,)),
        ("update_info 2: dual columns, reduction, barrier (8)", (8,)),
        ("update_info 3: combine, barrier; decision (11)", (11,)),
        ("refill: launder, offsets, load_rhs_ops to ph_rhs's barrier (15)", (15,)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=16)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--copies", type=int, nargs="+", default=[256, 512])
    a = ap.parse_args()
    import torch
    import mpcq
    dev = torch.device("cuda", 0)
    src = mpcq.synth.make_batch(1024, a.N, gaits=("trot",), seed=2)
    print(f"build {mpcq._lib.build_info().get('src_sha256', '?')}  N={a.N}, {a.iters} iterations, checks every 25 vs none")
    for B in a.copies:
        xr = torch.from_numpy(np.ascontiguousarray(np.repeat(src["xref"][:1], B, axis=0))).to(dev)
        fs = torch.from_numpy(np.ascontiguousarray(np.repeat(src["fsteps"][:1], B, axis=0))).to(dev)
        f0 = torch.empty((B, 12), dtype=torch.float64, device=dev)
        st = torch.empty(B, dtype=torch.int32, device=dev)
        it = torch.empty(B, dtype=torch.int32, device=dev)
        S = {}
        for chk in (0, 25):
            stamps = torch.zeros((B, 16), dtype=torch.int64, device=dev)
            eng = mpcq.Engine(a.N, adaptive_rho=0, max_iter=a.iters, check_termination=chk, eps_abs=1e-30, eps_rel=1e-30)
            mpcq.lib().mpcq_debug_set_stamps(eng._h, C.c_void_p(stamps.data_ptr()))
            for _ in range(2):  # (the second launch's stamps: the first also pays the code's first touch)
                stamps.zero_()
                eng.solve_device(B, xr.data_ptr(), fs.data_ptr(), f0.data_ptr(), st.data_ptr(), it.data_ptr())
                torch.cuda.synchronize()
            assert int(it[0].item()) == a.iters
            S[chk] = np.median(stamps.cpu().numpy().astype(np.float64), axis=0)
            ms = eng.last_kernel_ms()[1]
            if chk:  # cycles per ns, from a resident instance's whole life (B <= 512: no second round)
                ghz = float(S[chk][:13].sum() + S[chk][15]) / (ms * 1e6)
            print(f"  B={B} check every {chk:2d}: kernel {ms:.3f} ms, {1e3 * ms / a.iters:.3f} us per iteration")
            eng.close()
        n_chk = a.iters // 25
        d = (S[25] - S[0]) / n_chk
        tot = 0.0
        for name, bs in ROWS:
            v = float(sum(d[b] for b in bs))
            tot += v
            print(f"  B={B}  {name:66s} {v:7.0f} cycles = {v / ghz:6.0f} ns")
        print(f"  B={B}  {'one boundary, sum':66s} {tot:7.0f} cycles = {tot / ghz:6.0f} ns   ({ghz:.2f} cycles per ns)")


if __name__ == "__main__":
    main()
