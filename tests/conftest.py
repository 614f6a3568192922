"""pytest configuration: the `gpu` marker and shared fixtures.

-m "not gpu" runs here (no GPU): oracle vs golden vectors, host logic, C-ABI exports.
-m gpu runs on the MI355X box: the HIP path against the oracle and the golden vectors.
"""

import glob
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

GOLDEN = os.path.join(REPO, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (HIP) device")


@pytest.fixture(scope="session")
def golden_index():
    with open(os.path.join(GOLDEN, "index.json")) as f:
        return json.load(f)


def load_golden(name):
    """The arrays of <name>.npz, joined with those a case too large for one file keeps split
    along their leading axis in <name>.part0.npz, <name>.part1.npz, ..."""
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))
    parts = [np.load(p, allow_pickle=False)
             for p in sorted(glob.glob(os.path.join(GOLDEN, f"{name}.part[0-9].npz")))]
    if parts:
        for k in parts[0].files:
            g[k] = np.concatenate([p[k] for p in parts])
    return g
