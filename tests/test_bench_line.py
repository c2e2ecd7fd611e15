"""bench.py's plain run: the headline line alone, exactly --steps timed steps, and --dump-outputs writing what the last
timed step computed (a seeded sample of the crops, bit for bit the oracle's, and every ROI's crop sum)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_and_dumps_the_crops(tmp_path, oracle):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "RROI_BENCH_ONE_DEVICE")}
    d = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["metric"] == "RoIRotate forward ROIs/sec" and r["unit"] == "ROIs/s" and r["higher_is_better"] is True
    assert r["dtype"] == "f32" and r["steps"] == 7 and r["warmup"] == 2 and r["n_gpus"] == 1
    assert r["ms_per_step"] > 0 and abs(r["value"] - 512 / (r["ms_per_step"] * 1e-3)) < 1e-3 * r["value"]
    assert "roofline" not in r and "extra" not in r and "cpu_baseline" not in r     # those are --full's

    sys.path.insert(0, ROOT)
    import bench
    feats, rois = bench.make_inputs(512)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(512, size=bench.DUMP_ROIS, replace=False))
    sample = np.load(d / "crops_sample.npy")
    sums = np.load(d / "crops_sum_per_roi.npy")
    assert sample.dtype == np.float32 and sample.shape == (bench.DUMP_ROIS, 256, 8, 64)
    assert sums.dtype == np.float64 and sums.shape == (512,)
    assert sample.nbytes + sums.nbytes <= 64 << 20
    assert np.array_equal(sample, oracle.forward_c(feats, rois[idx], 8, 64, 0.25, threads=8))
    np.testing.assert_allclose(sums[idx], sample.astype(np.float64).sum(axis=(1, 2, 3)), rtol=1e-9, atol=1e-9)
