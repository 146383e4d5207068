"""bench.py's command line: the plain run (headline figure only), --dump-outputs and the --full switch."""

from __future__ import annotations

import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
PLAIN_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "process_group"}


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_writes_float_npy_and_samples_large_arrays(bench, tmp_path, monkeypatch):
    small = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    big = np.arange(1000, dtype=np.float64)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 800)  # 200 f32 / 100 f64 elements
    info = bench.dump_outputs(tmp_path / "a", {"small": small, "big": big})
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["big.npy", "small.npy"]
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    got = np.load(tmp_path / "a" / "big.npy")
    assert got.dtype == np.float64 and got.shape == (100,)
    assert np.all(np.diff(got) > 0) and np.all(big[got.astype(int)] == got)  # distinct elements, in index order
    assert info["arrays"]["big"] == {"saved": [100], "of": [1000]}
    bench.dump_outputs(tmp_path / "b", {"big": big})  # the same sample on every run
    assert np.array_equal(np.load(tmp_path / "b" / "big.npy"), got)
    with pytest.raises(AssertionError):
        bench.dump_outputs(tmp_path / "c", {"ints": np.arange(4)})


def test_profile_json_needs_full(bench, monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--profile-json", "p.json"])
    with pytest.raises(SystemExit) as e:
        bench.parse_args()
    assert e.value.code == 2 and "--full" in capsys.readouterr().err
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--profile-json", "p.json", "--dump-outputs", "d"])
    a = bench.parse_args()
    assert a.full and a.profile_json == "p.json" and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse_args()
    assert not a.full and a.dump_outputs is None


@pytest.mark.gpu
def test_plain_run_prints_headline_only_and_dumps_last_step(device, tmp_path):
    """A plain run on a small shape: the line holds the headline keys and none of the --full legs, `steps` timed
    steps, and the dumped detections are the padded per-image results of the last step, the same from run to run."""
    def run(out):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                            "--batch", "2", "--imgsz", "160", "--dump-outputs", str(out)], capture_output=True,
                           text=True, timeout=110)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        return json.loads(lines[0])

    d = run(tmp_path / "a")
    assert set(d) == PLAIN_KEYS | {"outputs"}
    assert d["steps"] == 5 and d["warmup"] == 2 and d["unit"] == "images/sec" and d["dtype"] == "fp16"
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(2 * 1e3 / d["ms_per_step"], rel=1e-3)
    arrs = {p.stem: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert sorted(arrs) == ["counts", "dets", "keep"]
    dets, keep, counts = arrs["dets"], arrs["keep"], arrs["counts"]
    assert dets.dtype == np.float32 and dets.shape == (2, 300, 6)
    assert keep.dtype == np.float64 and keep.shape == (2, 300) and counts.shape == (2,)
    for i, c in enumerate(counts.astype(int)):
        assert 0 <= c <= 300
        assert np.all(dets[i, c:] == 0) and np.all(keep[i, c:] == -1)
        assert np.all(keep[i, :c] >= 0) and np.all(dets[i, :c, 4] >= 0.25)  # kept anchors above the NMS threshold
        assert np.all(np.diff(dets[i, :c, 4]) <= 0)  # sorted by confidence, as the NMS returns them
    run(tmp_path / "b")
    for name, v in arrs.items():
        assert np.array_equal(np.load(tmp_path / "b" / f"{name}.npy"), v), name
