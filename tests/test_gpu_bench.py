"""bench.py end to end on the GPU: a plain run times the headline and nothing else (the rest is --full's)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_only(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["MISPEC_BENCH_DETAIL_DIR"] = str(tmp_path)  # (the side file, out of the tree)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--dump-outputs", str(tmp_path / "dump")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["metric"] == "spectrogram frames/sec" and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 5 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(64 * 862 / (d["ms_per_step"] * 1e-3), rel=1e-3)
    # only the timed arithmetic; nothing measured in runs of its own
    assert set(d["paths"]) == {"fft"}
    for k in ("extra", "gather", "roofline_cqt84", "reference_ops_on_this_gpu", "cpu_baseline"):
        assert k not in d, k
    assert d["roofline"]["traffic"] is None and "dominant_kernel" not in d["roofline"]
    y = np.load(tmp_path / "dump" / "stft.npy")
    assert y.dtype == np.float32 and y.size > 0 and np.isfinite(y).all()
