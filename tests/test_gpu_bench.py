"""bench.py as a build is measured with it: a plain run times exactly --steps steps in one block and adds nothing beside the headline,
--dump-outputs writes the same fields from run to run (two builds can be compared output for output), and --full still adds the
repeated blocks and the probes of the roofline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "2048"] + list(args),
                       capture_output=True, text=True, timeout=500, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
@pytest.mark.timeout(600, method="thread")
def test_plain_run_times_the_steps_asked_for_and_dumps_the_same_fields_every_time(lbhip, tmp_path):
    runs = []
    for r in range(2):
        d = tmp_path / ("run%d" % r)
        line = _bench("--steps", "40", "--warmup", "8", "--dump-outputs", str(d))
        assert line["steps"] == 40 and line["timing"]["blocks"] == 1 and line["timing"]["block_steps"] == 40
        assert line["ms_per_step"] > 0 and line["health"]["n_nonfinite"] == 0
        for k in ("cpu_baseline", "other_configs", "copy_GBps", "slabs"):
            assert k not in line, k
        assert line["roofline"]["plain_launch_ms"] is None and line["roofline"]["six_step_kernel"] is None
        runs.append({k: np.load(str(d / (k + ".npy"))) for k in ("f", "rho", "u", "v")})
    a, b = runs
    assert a["f"].shape == (1 << 20, 9) and all(a[k].shape == (1 << 20,) for k in ("rho", "u", "v"))
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k
    # the same cells in every file: rho is the zeroth moment of the populations
    np.testing.assert_allclose(a["f"].astype(np.float64).sum(axis=1), a["rho"], rtol=0, atol=1e-5)
    assert abs(float(a["rho"].mean()) - 1.0) < 1e-3 and float(np.abs(a["u"]).max()) > 0.01


@pytest.mark.gpu
@pytest.mark.timeout(600, method="thread")
def test_full_run_adds_the_repeated_blocks_and_the_roofline_probes(lbhip):
    line = _bench("--steps", "21", "--warmup", "7", "--full", "--no-cpu-baseline", "--no-other-configs", "--min-timed-s", "0.05")
    t = line["timing"]
    assert line["steps"] == 21 and t["blocks"] >= 5 and t["min_ms_per_step"] <= t["median_ms_per_step"] <= t["max_ms_per_step"]
    assert line["copy_GBps"]["plain"] > 0 and line["copy_GBps"]["nontemporal"] > 0
