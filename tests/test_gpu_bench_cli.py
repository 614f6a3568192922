"""GPU: bench.py's command line. A plain run prints one result line whose ms_per_step is the
time of one of the --steps timed steps and takes none of the --full measurements;
--dump-outputs writes the last timed step's rays, which equal the oracle's trace of the same
seeded pupil bit for bit (the parity of tests/test_gpu_parity.py, through the benchmark)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import REPO

pytestmark = pytest.mark.gpu

RAYS = 4099  # odd, more than one block


def test_plain_run_line_and_dumped_outputs(tmp_path):
    out_dir = tmp_path / "outputs"
    p = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3",
         "--warmup", "1", "--ramp-steps", "0", "--rays", str(RAYS),
         "--dump-outputs", str(out_dir)],
        cwd=REPO, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(line)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    S = line["config"]["surfaces"]
    assert abs(line["value"] - RAYS * S / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    assert line["cpu_baseline"] is None  # the CPU leg is --full's

    from optiland_pr_amd import _abi
    from optiland_pr_amd.distribution import RandomDistribution
    from optiland_pr_amd.lowering import lower_surface_group, segment_params
    from optiland_pr_amd.samples import DoubleGauss
    from oracle import trace_np

    assert sorted(os.listdir(out_dir)) == sorted(f"{a}.npy" for a in _abi.RAY_FIELDS)
    got = {a: np.load(out_dir / f"{a}.npy") for a in _abi.RAY_FIELDS}
    lens = DoubleGauss()
    table = lower_surface_group(lens.surface_group, [0.5876])
    d = RandomDistribution(seed=0)
    d.generate_points(RAYS)
    seg = segment_params(lens, 0.0, 1.0, 0)
    ref = trace_np.trace_segment(
        table, trace_np.generate_rays(seg, np.asarray(d.x), np.asarray(d.y)), 0).rays
    for a in ("x", "y", "z", "L", "M", "N", "opd"):
        assert got[a].dtype == np.float64 and got[a].shape == (RAYS,)
        np.testing.assert_array_equal(got[a], getattr(ref, a), err_msg=a)
    np.testing.assert_allclose(got["i"], ref.i, rtol=1e-12)
