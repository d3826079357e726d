#!/usr/bin/env python3
"""Digest of the engine's gfx950 assembly per horizon (CPU only: no GPU, no library load).

Compiles mpcq_engine.hip for each horizon with the flags of the Makefile's production
rule (taken from a dry run of that rule, so a per-horizon exception stays in one place),
plus --cuda-device-only -S, and prints `N sha256 lds_bytes`.  The digest leaves out what
moves with the source text or the LDS size alone: the __hip_cuid_ symbol and the
group_segment_fixed_size / LDSByteSize lines.  lds_bytes lists every distinct size of the
unit's kernels.  Two checkouts whose columns agree have the same device code:

  tools/engine_asm_digest.py 16 32 48 [-DMPCQ_STAMPS] [--src other/csrc/mpcq_engine.hip]

"Another checkout's engine source" means that checkout's csrc/: the engine's quoted includes
(mpcq_internal.h, mpcq_engine_layout.h, _lanes.h, _gj.h, _form.h) resolve next to the source
given, so --src takes the other checkout's headers with it; the flags stay this checkout's.
"""
import argparse
import hashlib
import os
import re
import shlex
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mpc-tsid_amd", "csrc")
DROP = ("__hip_cuid_", "group_segment_fixed_size", "LDSByteSize")


def rule_flags(horizons):
    """{N: the flags of build/engine_nN.o's recipe}, read from make's dry run."""
    out = subprocess.run(["make", "-n", "-W", "mpcq_engine.hip"] + ["build/engine_n%d.o" % n for n in horizons],
                         cwd=CSRC, check=True, capture_output=True, text=True).stdout
    flags = {}
    for line in out.splitlines():
        m = re.search(r"-DMPCQ_ENGINE_N=(\d+)", line)
        if m:
            w = shlex.split(line)
            first = next(i for i, x in enumerate(w) if x.startswith("-"))  # after the compiler driver
            flags[int(m.group(1))] = w[first:w.index("-c")]
    return flags


def digest(n, flags, src, hipcc):
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", "-o", "-", src]
    asm = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    lds = sorted({int(x) for x in re.findall(r"group_segment_fixed_size:\s*(\d+)", asm)})
    kept = "".join(l + "\n" for l in asm.splitlines() if not any(d in l for d in DROP))
    return "%d %s %s" % (n, hashlib.sha256(kept.encode()).hexdigest(), ",".join(map(str, lds)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("horizons", nargs="*", type=int, default=list(range(4, 65)))
    ap.add_argument("-D", dest="defs", action="append", default=[], help="extra -D switch (MPCQ_STAMPS ...)")
    ap.add_argument("--src", default=os.path.join(CSRC, "mpcq_engine.hip"), help="another checkout's engine source (its csrc/ supplies the headers)")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    flags = rule_flags(a.horizons)
    src = os.path.abspath(a.src)
    with ThreadPoolExecutor(max(1, min(16, a.j))) as ex:
        jobs = [ex.submit(digest, n, flags[n] + ["-D" + d for d in a.defs], src, a.hipcc) for n in a.horizons]
        for j in jobs:
            print(j.result(), flush=True)


if __name__ == "__main__":
    sys.exit(main())
