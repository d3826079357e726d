"""CPU: bench.py's --full / --dump-outputs options -- a plain run leaves the extra legs off,
and the dump is float64, repeatable and bounded."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def test_full_is_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"
    assert a.companion == 1 and a.certify == 1024 and a.cpu_sample > 0  # --full keeps the legs' defaults


def test_dump_outputs_whole(tmp_path):
    import bench
    f0 = np.arange(36, dtype=np.float64).reshape(3, 12)
    st = np.array([1, 2, -2], dtype=np.int32)
    bench.dump_outputs(str(tmp_path / "d"), {"f0": f0, "status": st})
    assert sorted(os.listdir(tmp_path / "d")) == ["f0.npy", "status.npy"]
    got = np.load(tmp_path / "d" / "status.npy")
    assert got.dtype == np.float64 and np.array_equal(got, st)
    assert np.array_equal(np.load(tmp_path / "d" / "f0.npy"), f0)
    bench.dump_outputs(str(tmp_path / "d"), {"f0": f0}, rank=1)
    assert os.path.exists(tmp_path / "d" / "f0_rank1.npy")


def test_dump_outputs_samples_beyond_the_limit(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT", 4096)
    a = np.random.default_rng(1).normal(size=(1000, 7))
    s = np.arange(1000, dtype=np.int32)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "s": s})
    rows = np.load(tmp_path / "x" / "rows.npy").astype(int)
    assert np.array_equal(rows, np.load(tmp_path / "y" / "rows.npy").astype(int))  # the same sample every run
    assert 0 < len(rows) < 1000 and len(set(rows)) == len(rows) and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "x" / "a.npy"), a[rows])
    assert np.array_equal(np.load(tmp_path / "x" / "s.npy"), rows)
    total = sum(os.path.getsize(tmp_path / "x" / f) - 128 for f in os.listdir(tmp_path / "x"))
    assert total <= 4096
