"""CPU: the session layout unit (csrc/mpcq_session_layout.cpp) on its own, under the address and
undefined-behaviour sanitizers: tests/host/session_layout_check.cpp is compiled with it as plain
C++17 (no HIP, nothing preloaded) and answers, for shapes and headers sent on its standard input,
what blob_header, snap_sizes, shape_difference and parse_blob_header say.  The expected answers come
from tests/snapshot_model.py, the blob format restated from include/mpcq.h."""
import itertools
import os
import shutil
import struct
import subprocess

import pytest

import snapshot_model as SM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mpc-tsid_amd", "csrc")
N = 8
# offsets in the header (include/mpcq.h)
VERSION, HN, HB, K_MPC, FLAGS, GROUP_BYTES, TOTAL, CHANNEL_BYTES, DELAY, LATENCY, ESTIMATOR_BYTES = \
    8, 12, 16, 24, 28, 32, 88, 104, 112, 116, 120
GAIT_BYTES, N_GAITS, PAD, DISTURB_BYTES, PAD5 = 128, 136, 140, 144, 152
PART_BYTES_AT = [GROUP_BYTES + 8 * i for i in range(7)] + [CHANNEL_BYTES, ESTIMATOR_BYTES, GAIT_BYTES, DISTURB_BYTES]


def _clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("amdclang++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no ROCm clang++")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """The check program, with the sanitizers (without them where their runtime does not link)."""
    out = str(tmp_path_factory.mktemp("layout") / "session_layout_check")
    cmd = [_clangxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + CSRC, "-o", out,
           os.path.join(REPO, "tests", "host", "session_layout_check.cpp"), os.path.join(CSRC, "mpcq_session_layout.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(cmd + san, capture_output=True, text=True)
    if r.returncode != 0 and ("sanitize" in r.stderr or "libclang_rt" in r.stderr):
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def ask(lines):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        env.pop("LD_PRELOAD", None)
        p = subprocess.run([out], input="".join(x + "\n" for x in lines), capture_output=True, text=True, env=env,
                           timeout=120)
        assert p.returncode == 0, (p.returncode, p.stderr[-4000:])
        answers = p.stdout.splitlines()
        assert len(answers) == len(lines)
        return answers
    return ask


def _mask(parts):
    return 1 | sum(1 << SM.PARTS.index(p) for p in parts)


def _shape_words(B, cfg):
    return f"{B} {cfg.get('k_mpc', 0)} {_mask(cfg.get('parts', ()))} {cfg.get('delay', 0)} {cfg.get('latency', 0)} " \
           f"{cfg.get('n_gaits', 0)}"


def _layout_cmd(B, cfg, have_order, resets):
    return f"L {N} {_shape_words(B, cfg)} {int(have_order)} {int(resets)}"


def _subsets():
    """Every subset of the optional parts, with the parameters its parts need."""
    for r in range(len(SM.OPTIONAL) + 1):
        for parts in itertools.combinations(SM.OPTIONAL, r):
            yield dict(parts=parts, k_mpc=5 if "swing" in parts else 0, delay=3 if "channel" in parts else 0,
                       latency=2 if "channel" in parts else 0, n_gaits=3 if "gait" in parts else 0)


def test_headers_and_arrays_against_the_model(check):
    cases = [(3, cfg, True, False) for cfg in SM.CASES.values()]
    cases += [(1, cfg, i % 2 == 0, i % 3 == 0) for i, cfg in enumerate(_subsets())]
    assert len(cases) == 8 + 2 ** len(SM.OPTIONAL)
    answers = check([_layout_cmd(*c) for c in cases])
    parse = []
    for (B, cfg, have_order, resets), got in zip(cases, answers):
        header, arrays = SM.layout(N, B, have_order=have_order, resets=resets, **cfg)
        h, hexed, a, *items = got.split()
        assert (h, a) == ("H", "A")
        assert bytes.fromhex(hexed) == header, cfg
        listed = [tuple(int(x) for x in it.split(":")) for it in items]
        assert [nb for _, _, nb in listed] == [nb for _, nb in arrays], cfg
        # part by part: the arrays of part gi are the model's, in its order
        present = [p for p in SM.PARTS if p == "main" or p in cfg.get("parts", ())]
        want = [(SM.PARTS.index(p), nb) for p in present for _, nb in SM.arrays_of(p, N, B, cfg.get("k_mpc", 0))]
        assert [(gi, nb) for gi, _, nb in listed] == want, cfg
        parse.append(f"P {N} {struct.unpack_from('<q', header, TOTAL)[0]} {hexed}")
    # and the unit reads every header back as the shape it was made from
    for (B, cfg, have_order, resets), back in zip(cases, check(parse)):
        assert back == f"OK {_shape_words(B, cfg)} {int(have_order)} {int(resets)}", (cfg, back)


def _put(header, fmt, at, value):
    h = bytearray(header)
    struct.pack_into(fmt, h, at, value)
    return bytes(h)


def test_every_condition_of_the_import_check_refuses(check):
    B = 3
    base = {name: SM.layout(N, B, have_order=True, **cfg)[0] for name, cfg in SM.CASES.items()}
    total = {name: struct.unpack_from("<q", h, TOTAL)[0] for name, h in base.items()}
    every, plain, gait, disturb = base["everything"], base["nothing"], base["gait"], base["disturb"]
    flags = lambda h: struct.unpack_from("<I", h, FLAGS)[0]  # noqa: E731
    # (what, header, N, bytes; None: the header's own total)
    bad = [
        ("magic", _put(every, "<B", 3, every[3] ^ 0x20), N, None),
        ("version 0", _put(every, "<I", VERSION, 0), N, None),
        ("version 6", _put(every, "<I", VERSION, 6), N, None),
        ("N + 1", every, N + 1, None),
        ("N - 1", every, N - 1, None),
        ("B 0", _put(every, "<q", HB, 0), N, None),
        ("B 2^31", _put(every, "<q", HB, 2 ** 31), N, None),
        ("k_mpc -1", _put(every, "<i", K_MPC, -1), N, None),
        ("k_mpc 65537", _put(every, "<i", K_MPC, 65537), N, None),
        ("flag bit 12", _put(every, "<I", FLAGS, flags(every) | 1 << 12), N, None),
        ("flag bit 31", _put(every, "<I", FLAGS, flags(every) | 1 << 31), N, None),
        ("swing flag without k_mpc", _put(every, "<i", K_MPC, 0), N, None),
        ("swing flag without k_mpc, plain", _put(plain, "<I", FLAGS, flags(plain) | 4), N, None),
        ("k_mpc without swing flag", _put(plain, "<i", K_MPC, 7), N, None),
        ("version 2 without channel", _put(plain, "<I", VERSION, 2), N, None),
        ("version 4 with disturb", _put(every, "<I", VERSION, 4), N, None),
        ("version 5 without disturb", _put(gait + bytes(16), "<I", VERSION, 5), N, None),
        ("estimator_bytes without estimator", _put(plain, "<q", ESTIMATOR_BYTES, 8), N, None),
        ("channel_bytes without channel", _put(plain, "<q", CHANNEL_BYTES, 8), N, None),
        ("delay without channel", _put(plain, "<i", DELAY, 1), N, None),
        ("latency without channel", _put(plain, "<i", LATENCY, 1), N, None),
        ("delay 9", _put(every, "<i", DELAY, 9), N, None),
        ("latency 5", _put(every, "<i", LATENCY, 5), N, None),
        ("n_gaits 0", _put(gait, "<i", N_GAITS, 0), N, None),
        ("n_gaits 9", _put(gait, "<i", N_GAITS, 9), N, None),
        ("n_gaits without gait", _put(disturb, "<i", N_GAITS, 1), N, None),
        ("pad", _put(gait, "<i", PAD, 1), N, None),
        ("pad5", _put(every, "<q", PAD5, 1), N, None),
        ("total + 8", _put(every, "<q", TOTAL, total["everything"] + 8), N, None),
        ("total - 8", _put(plain, "<q", TOTAL, total["nothing"] - 8), N, None),
        ("bytes - 8", every, N, total["everything"] - 8),
        ("bytes + 1", plain, N, total["nothing"] + 1),
    ]
    for gi, at in enumerate(PART_BYTES_AT):  # each part's byte count, present or not
        for name in ("everything", "disturb"):
            h = base[name]
            have, = struct.unpack_from("<q", h, at)
            bad.append((f"part {gi} + 8 in {name}", _put(h, "<q", at, have + 8), N, None))
            if have:
                bad.append((f"part {gi} - 8 in {name}", _put(h, "<q", at, have - 8), N, None))
    for name, h in base.items():  # fewer bytes than the version's header
        bad.append((f"short header of {name}", h, N, len(h) - 8))
        bad.append((f"no bytes of {name}", h, N, 0))
    good = [(name, h, N, None) for name, h in base.items()]
    cmds = []
    for what, h, n, nbytes in good + bad:
        if nbytes is None:
            nbytes, = struct.unpack_from("<q", h, TOTAL)
        cmds.append(f"P {n} {nbytes} {h.hex()}")
    answers = check(cmds)
    for (what, *_), got in zip(good, answers):
        assert got.startswith("OK "), (what, got)
    for (what, *_), got in zip(bad, answers[len(good):]):
        assert got.startswith("NO ") and len(got) > 8, (what, got)
    by = dict(zip((w for w, *_ in bad), answers[len(good):]))
    assert by["magic"] == "NO not a snapshot blob (magic)"
    assert by["version 6"] == "NO blob format version 6, this library reads 1 to 5"
    assert by["N + 1"] == f"NO the blob is of a context with N = {N}, this one has N = {N + 1}"
    assert by["B 0"].startswith("NO the blob's header is inconsistent (B 0, k_mpc 7, flags 0xffd)")
    assert by["part 2 + 8 in everything"] == f"NO the blob's part 2 has {240 * B + 8} bytes, its shape says {240 * B}"
    assert by["short header of gait"] == "NO 136 bytes are less than a version-4 header"
    assert by["short header of nothing"] == "NO 120 bytes are less than a header"
    assert "(truncated?)" in by["bytes - 8"]


def test_shape_difference_names_the_first_difference(check):
    full = SM.CASES["everything"]
    without = lambda p: dict(full, parts=tuple(q for q in full["parts"] if q != p),  # noqa: E731
                             **({"k_mpc": 0} if p == "swing" else {}),
                             **({"delay": 0, "latency": 0} if p == "channel" else {}),
                             **({"n_gaits": 0} if p == "gait" else {}))
    one_side = {"swing": "the swing arrays exist on one side only", "plant": "the plant arrays exist on one side only",
                "monitor": "the monitor arrays exist on one side only",
                "scenario": "the scenario arrays exist on one side only",
                "robots": "the robots table is in force on one side only",
                "plant_robots": "the plant robots table is in force on one side only",
                "channel": "the channel arrays exist on one side only",
                "estimator": "the estimator arrays exist on one side only",
                "gait": "the gait arrays exist on one side only", "disturb": "the disturb arrays exist on one side only"}
    cases = [(3, full, 3, full, 1, "SAME"), (3, full, 4, full, 0, "SAME"),
             (3, full, 4, full, 1, "DIFF the batch sizes differ (a restore without a map needs the same batch)"),
             (3, full, 3, dict(full, k_mpc=6), 1, "DIFF the swing k_mpc differs"),
             (3, full, 3, dict(full, delay=1), 1,
              "DIFF the channel's delay differs (the rings were filled under another)"),
             (3, full, 3, dict(full, latency=2), 1,
              "DIFF the channel's latency differs (the rings were filled under another)"),
             (3, full, 3, dict(full, n_gaits=3), 1,
              "DIFF the gait library sizes differ (the rows index another library)"),
             # two differences: the earlier part's is named
             (3, dict(full, k_mpc=6), 3, without("plant"), 1, "DIFF the swing k_mpc differs"),
             (3, without("monitor"), 3, dict(full, delay=1), 1, "DIFF the monitor arrays exist on one side only")]
    cases += [(3, full, 3, without(p), 1, "DIFF " + text) for p, text in one_side.items()]
    cases += [(3, without(p), 3, full, 1, "DIFF " + text) for p, text in one_side.items()]
    answers = check([f"D {_shape_words(Ba, a)} {_shape_words(Bb, b)} {batch_too}" for Ba, a, Bb, b, batch_too, _ in cases])
    for (*_, want), got in zip(cases, answers):
        assert got == want
