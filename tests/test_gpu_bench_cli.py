"""bench.py's plain command line: the result line's contract fields, --steps as the number of timed steps, and --dump-outputs
writing the last timed step's arrays -- identical from run to run on the seeded inputs.  Each run is a fresh child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args), cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_the_steps_asked_for_and_dumps_the_same_outputs_twice(tmp_path):
    B, N, K, W = 64, 12, 7, 2
    runs = []
    for i in range(2):
        d = tmp_path / ("out%d" % i)
        j = _bench("--batch", str(B), "--feat", str(N), "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(d))
        assert j["steps"] == K and j["warmup"] == W and j["unit"] == "EKF steps/s" and j["dtype"] == "f64"
        assert j["higher_is_better"] is True and j["value"] > 0 and j["ms_per_step"] > 0
        assert abs(j["value"] - B * 1e3 / j["ms_per_step"]) <= 1e-6 * j["value"]
        assert j["timed_work"]["updates"] == K * B * N and j["nan_filters"] == 0
        assert "cpu_baseline" not in j and "configs" not in j and "no_prewarm" not in j     # the legs of --full
        runs.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = runs
    assert sorted(a) == ["covariance", "result", "state"]
    assert a["state"].shape == (B, 17 + 5 * N) and a["covariance"].shape == (B, 16 + 3 * N, 16 + 3 * N) and a["result"].shape == (B, N)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert np.isfinite(a["state"]).all() and np.isfinite(a["covariance"]).all()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
