"""CPU: bench.py's command line and its --dump-outputs writer (no GPU needed)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_small_canvas_whole(tmp_path):
    rng = np.random.default_rng(5)
    canvas = rng.integers(0, 256, (40, 90), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path), canvas, {"psnr": 31.5, "ssim_gauss": 0.97})
    got = _load(str(tmp_path))
    assert sorted(got) == ["canvas_col_sums", "canvas_row_sums", "canvas_sample", "canvas_sample_index", "psnr", "ssim_gauss"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["canvas_sample"], canvas.reshape(-1).astype(np.float32))
    assert np.array_equal(got["canvas_sample_index"], np.arange(canvas.size, dtype=np.float64))
    assert np.array_equal(got["canvas_row_sums"], canvas.sum(axis=1, dtype=np.int64))
    assert np.array_equal(got["canvas_col_sums"], canvas.sum(axis=0, dtype=np.int64))
    assert got["psnr"].tolist() == [31.5] and got["ssim_gauss"].tolist() == [0.97]


def test_dump_outputs_sample_is_fixed(tmp_path, monkeypatch):
    """A canvas larger than the sample: the same seeded byte positions every time, values read at those positions."""
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    canvas = np.random.default_rng(6).integers(0, 256, (100, 300), dtype=np.uint8)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, canvas, {})
    bench.dump_outputs(b, canvas, {})
    da, db = _load(a), _load(b)
    assert all(np.array_equal(da[k], db[k]) for k in da)
    idx = da["canvas_sample_index"].astype(np.int64)
    assert idx.size == 1000 and np.all(np.diff(idx) > 0) and idx[-1] < canvas.size
    assert np.array_equal(da["canvas_sample"], canvas.reshape(-1)[idx])


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr and r.stdout == ""
