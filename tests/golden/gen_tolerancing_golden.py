"""Tolerancing golden vectors: the REFERENCE's MonteCarlo and SensitivityAnalysis
(optiland/tolerancing) with the NumPy backend on the Cooke triplet.

Test infrastructure only, run in the build container (never on the GPU box):

    PYTHONPATH=tests/golden/shims:<reference checkout> PYTHONDONTWRITEBYTECODE=1 \\
        python tests/golden/gen_tolerancing_golden.py

Writes tests/golden/tolerancing.npz, arrays "<case>/<name>":

  A  MonteCarlo.run(64): one rms_spot_size operand per field (image surface, 6 hexapolar
     rings, 0.55 um) under five perturbations (CASE_A below). "A/columns" holds the
     DataFrame's column names in order, "A/<column>" each column [64]; every one of the 64 x 8
     values is asserted finite here, so no test may drop a trial.
  B  SensitivityAnalysis over radius of surface 1, RangeSampler(22.0, 22.05, 5), field
     (0, 1): "B/columns", "B/perturbation_type" (str), "B/perturbation_value" and the operand
     column.

monte_carlo.py imports seaborn, which only its view_* methods use: an empty stand-in module
is registered before the import.
"""

from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True
sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

import optiland.backend as be  # noqa: E402
from optiland.samples.objectives import CookeTriplet  # noqa: E402
from optiland.tolerancing.core import Tolerancing  # noqa: E402
from optiland.tolerancing.monte_carlo import MonteCarlo  # noqa: E402
from optiland.tolerancing.perturbation import DistributionSampler, RangeSampler  # noqa: E402
from optiland.tolerancing.sensitivity_analysis import SensitivityAnalysis  # noqa: E402

be.set_backend("numpy")

WAVELENGTH = 0.55
NUM_RAYS = 6
TRIALS = 64


def operand_data(lens, field):
    return {"optic": lens, "surface_number": -1, "Hx": field[0], "Hy": field[1],
            "num_rays": NUM_RAYS, "wavelength": WAVELENGTH, "distribution": "hexapolar"}


def case_a():
    lens = CookeTriplet()
    t = Tolerancing(lens)
    for field in lens.fields.get_field_coords():
        t.add_operand("rms_spot_size", operand_data(lens, field))
    r1 = float(lens.surface_group.radii[1])
    t.add_perturbation("radius", DistributionSampler("normal", seed=1, loc=r1, scale=0.05),
                       surface_number=1)
    t.add_perturbation("thickness", DistributionSampler("uniform", seed=2, low=3.2, high=3.3),
                       surface_number=1)
    t.add_perturbation("tilt", DistributionSampler("normal", seed=3, loc=0.0, scale=1e-3),
                       surface_number=3, axis="x")
    t.add_perturbation("decenter", DistributionSampler("normal", seed=4, loc=0.0, scale=0.02),
                       surface_number=4, axis="y")
    t.add_perturbation("index", DistributionSampler("normal", seed=5, loc=1.6, scale=1e-3),
                       surface_number=1, wavelength=WAVELENGTH)
    mc = MonteCarlo(t)
    mc.run(TRIALS)
    df = mc.get_results()
    out = {"columns": np.array(list(df.columns)), "nominal_radius": np.float64(r1),
           "fields": np.asarray(lens.fields.get_field_coords(), dtype=np.float64),
           "targets": np.array([op.target for op in t.operands], dtype=np.float64)}
    assert df.shape == (TRIALS, 8), df.shape
    for c in df.columns:
        col = np.asarray(df[c], dtype=np.float64)
        assert col.shape == (TRIALS,) and np.all(np.isfinite(col)), c
        out[c] = col
    return out


def case_b():
    lens = CookeTriplet()
    t = Tolerancing(lens)
    t.add_operand("rms_spot_size", operand_data(lens, (0, 1)))
    t.add_perturbation("radius", RangeSampler(22.0, 22.05, 5), surface_number=1)
    sa = SensitivityAnalysis(t)
    sa.run()
    df = sa.get_results()
    out = {"columns": np.array(list(df.columns))}
    assert df.shape == (5, 3), df.shape
    out["perturbation_type"] = np.array([str(v) for v in df["perturbation_type"]])
    for c in df.columns[1:]:
        col = np.asarray(df[c], dtype=np.float64)
        assert np.all(np.isfinite(col)), c
        out[c] = col
    return out


def main():
    arrays = {}
    for key, fn in (("A", case_a), ("B", case_b)):
        for name, v in fn().items():
            arrays[f"{key}/{name}"] = v
            print(key, name, np.asarray(v).shape)
    np.savez_compressed(os.path.join(HERE, "tolerancing.npz"), **arrays)


if __name__ == "__main__":
    main()
