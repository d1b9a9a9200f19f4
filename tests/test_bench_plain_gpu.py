"""bench.py's plain one-GPU run: the headline line and nothing beside it (roofline, segments, host and CPU-baseline figures are
--full's), --steps sets the timed steps, and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_and_dump_outputs(cuda, tmp_path):
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["ms_per_step"] > 0
    assert abs(d["value"] - 2 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-3
    assert not {"roofline", "segments", "host", "host_ms_per_step", "cpu_baseline"} & set(d)
    files = sorted(os.listdir(out))
    arrays = {f[:-4]: np.load(out / f) for f in files}
    assert all(f.endswith(".npy") for f in files)
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for k in ("loss", "rpn_cls", "rpn_loc", "rcnn_cls", "rcnn_loc", "adloss", "dis_patch_loss", "recon_loss"):
        assert np.isfinite(arrays[k]).all(), k
    assert round(float(arrays["loss"]), 4) == d["config"]["final_loss"]
    for net in ("det", "dec", "dis", "dis_patch"):
        a = arrays["param_sample_" + net]
        assert a.ndim == 1 and 0 < a.size <= 1 << 20 and np.isfinite(a).all(), net
