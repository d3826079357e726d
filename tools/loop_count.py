#!/usr/bin/env python3
"""Instruction count of the production kernel's innermost ADMM loop, per class.

    python tools/loop_count.py [--N 16] [--src mpcq_engine.hip] [--asm out.s] [--json]

Compiles the engine for one horizon to gfx950 assembly with the flags the Makefile
gives that horizon's unit (read from `make -n`), finds engine_kernel<N, true, true,
false, false> (the fused solve bench.py launches) and in it the innermost loop that
holds a block barrier and the sweep's s_setprio -- one ADMM iteration: ph_rhs,
the two-ended sweep, ph_recover, the update -- and counts the instructions of every
block of that loop, i.e. the stream wave 0 executes (the other waves skip the sweep
blocks).  Counted before the nop-elision pass (asmpass/nop_elide.py), as the compiler
emits it; the line `after nop_elide` gives the count the assembler sees.

Classes: FP64 VALU (v_*_f64*), other VALU, SALU (s_*: nops, waits, barrier, branches
included), LDS (ds_*), scratch/global (scratch_*, global_*, flat_*, buffer_*).
"""
import argparse
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mpc-tsid_amd", "csrc")
sys.path.insert(0, os.path.join(CSRC, "asmpass"))

CLASSES = ("fp64_valu", "other_valu", "salu", "lds", "scratch_global")


def unit_flags(N):
    """The hipcc arguments of build/engine_n<N>.o, from the Makefile's own recipe."""
    tgt = f"build/engine_n{N}.o"
    out = subprocess.run(["make", "-n", "-s", "-C", CSRC, "-W", "mpcq_engine.hip", tgt],
                         capture_output=True, text=True, check=True).stdout
    for line in out.splitlines():
        w = shlex.split(line)
        if "-c" in w and tgt in w:
            w = w[next(i for i, a in enumerate(w) if a.startswith("-")):]
            i = w.index("-c")
            return w[:i]  # (what follows: -o <object> <source>)
    raise RuntimeError(f"no recipe for {tgt} in `make -n`")


def compile_asm(N, src, dst):
    cmd = ["/opt/rocm/bin/hipcc", *unit_flags(N), f"-I{CSRC}", "--cuda-device-only", "-S", "-o", dst, "-x", "hip", src]
    subprocess.run(cmd, cwd=CSRC, check=True, stderr=subprocess.DEVNULL)


def classify(op):
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("scratch_", "global_", "flat_", "buffer_")):
        return "scratch_global"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "fp64_valu" if "_f64" in op else "other_valu"
    raise ValueError(f"unclassified instruction {op!r}")


def kernel_lines(lines, N):
    tag = f"engine_kernelILi{N}ELb1ELb1ELb0ELb0EE"
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and tag in l and l.split(":")[0].endswith("E"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


LABEL = re.compile(r"^(\.LBB\d+_\d+):")
ANON = re.compile(r"^; %bb\.\d+:")
HDR = re.compile(r"Header=(BB\d+_\d+)")


def loops(klines):
    """{header label: [instruction, ...]} for every innermost loop of the kernel."""
    out, cur, inner = {}, None, set()
    i = 0
    while i < len(klines):
        l = klines[i]
        m = LABEL.match(l)
        if m or ANON.match(l):
            # the block's loop annotation: on the label's line and the comment lines after it
            note = l
            j = i + 1
            while j < len(klines) and klines[j].lstrip().startswith(";") and not ANON.match(klines[j]) \
                    and "#ASM" not in klines[j]:
                note += klines[j]
                j += 1
            if m and "This Inner Loop Header" in note:
                cur = m.group(1)[2:]
                inner.add(cur)
            else:  # (a loop's blocks may be laid out ahead of its header)
                h = HDR.search(note)
                cur = h.group(1) if h else None
            if cur is not None:
                out.setdefault(cur, [])
        else:
            s = l.split(";")[0].strip()
            if s and not s.startswith(".") and not s.endswith(":") and cur is not None:
                out[cur].append(s)
        i += 1
    return {h: ins for h, ins in out.items() if h in inner}


def count(instrs):
    c = dict.fromkeys(CLASSES, 0)
    for s in instrs:
        c[classify(s.split()[0])] += 1
    c["total"] = len(instrs)
    # FP64 operations of the source: clamp_hw's v_max_f64 / v_min_f64 pair is one of them
    # (DESIGN.md's table of the round-6 loop counts 315 this way, 318 instructions)
    ops = [s.split()[0] for s in instrs]
    c["fp64_ops"] = c["fp64_valu"] - sum(1 for a, b in zip(ops, ops[1:]) if a == "v_max_f64" and b == "v_min_f64")
    c["s_nop"] = sum(1 for s in instrs if s.startswith("s_nop"))
    c["s_waitcnt"] = sum(1 for s in instrs if s.startswith("s_waitcnt"))
    return c


def admm_loop(lines, N):
    """(header, instructions) of the ADMM iteration loop of the production kernel."""
    ls = loops(kernel_lines(lines, N))
    best = None
    for h, ins in ls.items():
        # (the sweep raises its wave's priority: the factorisation's loops have barriers too)
        if not any(s.startswith("s_barrier") for s in ins) or not any(s.startswith("s_setprio") for s in ins):
            continue
        f = sum(1 for s in ins if "_f64" in s.split()[0])
        if best is None or f > best[0]:
            best = (f, h, ins)
    if best is None:
        raise RuntimeError("no inner loop with a barrier in the production kernel")
    return best[1], best[2]


def measure(N=16, src=None, asm=None, reuse=False):
    import nop_elide
    src = os.path.abspath(src or os.path.join(CSRC, "mpcq_engine.hip"))
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.abspath(asm) if asm else os.path.join(tmp, f"engine_n{N}.s")
        if not (asm and reuse):
            compile_asm(N, src, s)
        lines = open(s).read().split("\n")
    head, ins = admm_loop(lines, N)
    res = {"N": N, "loop": head, **count(ins)}
    el, _, _ = nop_elide.elide(lines)
    res["after_nop_elide"] = count(admm_loop(el, N)[1])["total"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=16)
    ap.add_argument("--src", default=None, help="engine source (default: csrc/mpcq_engine.hip)")
    ap.add_argument("--asm", default=None, help="keep the assembly here")
    ap.add_argument("--reuse", action="store_true", help="count the assembly already at --asm (no compile)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    r = measure(a.N, a.src, a.asm, a.reuse)
    if a.json:
        print(json.dumps(r))
        return
    print(f"engine_kernel<{a.N}, true, true, false, false>, innermost ADMM loop ({r['loop']}):")
    for k in CLASSES:
        print(f"  {k:15s} {r[k]:5d}" + (f"   ({r['fp64_ops']} operations: a clamp's max / min pair is one)"
                                        if k == "fp64_valu" else ""))
    print(f"  {'total':15s} {r['total']:5d}   (of the SALU: {r['s_nop']} s_nop, {r['s_waitcnt']} s_waitcnt)")
    print(f"  after nop_elide {r['after_nop_elide']:5d}")


if __name__ == "__main__":
    main()
