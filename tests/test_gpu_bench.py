"""A plain bench.py run: it times exactly --steps steps, reports ms_per_step, leaves the --full legs out, and with
--dump-outputs writes the last timed step's centroids and assignments."""
import json
import os
import subprocess
import sys

import numpy
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    n, k, d = 200000, 256, 256
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--samples", str(n),
                          "--clusters", str(k), "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path)],
                         cwd=ROOT, capture_output=True, text=True, timeout=500)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0.0
    assert line["value"] == pytest.approx(n / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert not {"verify", "api_kmeans_cuda", "cpu_baseline", "roofline_other_filter"} & set(line)
    assert sorted(os.listdir(tmp_path)) == ["assignments.npy", "centroids.npy"]
    cen = numpy.load(str(tmp_path / "centroids.npy"))
    asg = numpy.load(str(tmp_path / "assignments.npy"))
    assert cen.dtype == numpy.float32 and cen.shape == (k, d) and numpy.isfinite(cen).all()
    assert asg.dtype == numpy.float32 and asg.shape == (n,)
    assert (asg == numpy.floor(asg)).all() and asg.min() >= 0 and asg.max() < k
