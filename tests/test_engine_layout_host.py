"""CPU: the engine's layout header (csrc/mpcq_engine_layout.h) for every compiled horizon, under the
address and undefined-behaviour sanitizers: tests/host/engine_layout_check.cpp is compiled as plain
C++17 (nothing preloaded) and checks, at N = 4..64, what an engine unit's static_asserts check for
its own N alone (Work<N> against work_doubles(N), the Smem<N> size bounds) and what no build checks:
the workspace regions, the 16-byte alignments, the SIG / SIGX permutations, the GH / Sm slots, the
prologue's aliases.  The column starts XO / FO it prints are held against the CSC pattern of the
library (mpcq_pattern, no device)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mpc-tsid_amd", "csrc")
HORIZONS = list(range(4, 65))


def _clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("amdclang++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no ROCm clang++")


def _rocm_include(cxx):
    # mpcq_internal.h takes the HIP runtime's declarations (host side only, nothing is called)
    d = os.path.dirname(cxx)
    while d != os.path.dirname(d):
        if os.path.exists(os.path.join(d, "include", "hip", "hip_runtime.h")):
            return os.path.join(d, "include")
        d = os.path.dirname(d)
    pytest.fail("no HIP headers beside " + cxx)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """The check program's output lines, with the sanitizers (without them where their runtime does not link)."""
    out = str(tmp_path_factory.mktemp("engine_layout") / "engine_layout_check")
    cxx = _clangxx()
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + CSRC,
           "-isystem", _rocm_include(cxx), "-o", out, os.path.join(REPO, "tests", "host", "engine_layout_check.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(cmd + san, capture_output=True, text=True)
    if r.returncode != 0 and ("sanitize" in r.stderr or "libclang_rt" in r.stderr):
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([out], capture_output=True, text=True, env=env, timeout=120)
    lines = p.stdout.splitlines()
    failed = [x for x in lines if x.startswith("FAIL")]
    assert p.returncode == 0 and not failed, (p.returncode, failed[:20], p.stderr[-4000:])
    return lines


def test_every_horizon_keeps_the_layout_invariants(report):
    assert [x for x in report if x.startswith("OK ")] == ["OK %d" % n for n in HORIZONS]


def test_layout_header_needs_no_hip(tmp_path):
    """The header alone is plain C++17: no HIP header, no other header of the project."""
    src = tmp_path / "alone.cpp"
    src.write_text('#include "mpcq_engine_layout.h"\n'
                   "static_assert(sizeof(mpcq::Smem<16>) <= 80 * 1024 && mpcq::XO<16>(15, 11) == 461, \"\");\n"
                   "int main() { return mpcq::SLOT<16>(9) == 144 * 9 + 2 ? 0 : 1; }\n")
    out = str(tmp_path / "alone")
    r = subprocess.run([_clangxx(), "-std=c++17", "-Wall", "-Werror", "-nostdinc++", "-I" + CSRC, "-o", out, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert subprocess.run([out]).returncode == 0


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as m
    m.build()
    return m


def test_column_starts_are_the_patterns(report, mpcq):
    starts = {int(w[1]): np.array(w[2:], np.int64) for w in (x.split() for x in report if x.startswith("C "))}
    assert sorted(starts) == HORIZONS
    for N in HORIZONS:
        indptr, _ = mpcq.pattern(N)
        # columns 12 k + i: X_{k+1}[i]; columns 12 N + 12 k + 3 f + c: f_k[3 f + c]
        assert np.array_equal(starts[N], indptr[:24 * N]), N
        assert indptr[24 * N] == 126 * N - 18
