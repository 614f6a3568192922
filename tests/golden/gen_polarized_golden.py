"""Polarization / coating golden vectors: the REFERENCE's PolarizedRays, FresnelCoating and
SimpleCoating traced on the CPU for the cases of polarized_cases.py.

Test infrastructure only, run in the build container (never on the GPU box):

    PYTHONPATH=tests/golden/shims:<reference checkout> PYTHONDONTWRITEBYTECODE=1 \
        python tests/golden/gen_polarized_golden.py

Writes tests/golden/polarized.npz, keys "<case>/<trace>/<name>" and
"<case>/<trace>/<state>/i": x y z L M N opd (state-independent), p_re / p_im [N, 3, 3] and
the per-surface minimum non-zero |k0 x k1| (smin) from the first state that carries P, and
per state the returned intensity `i` and surface_group.intensity (`si`).

Asserted here: no (ray, surface) has 0 < |k0 x k1| < 1e-8 (there the reference's own s axis
is rounding noise), and at most 10 % of a case's rays are NaN.
"""

from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import optiland.backend as be  # noqa: E402
from optiland import apodization, coatings, materials, optic  # noqa: E402
from optiland.physical_apertures import RadialAperture  # noqa: E402
from optiland.rays import PolarizedRays, create_polarization  # noqa: E402
from optiland.samples.objectives import CookeTriplet  # noqa: E402

import polarized_cases as pc  # noqa: E402

be.set_backend("numpy")


class NS:
    Optic = optic.Optic
    IdealMaterial = materials.IdealMaterial
    FresnelCoating = coatings.FresnelCoating
    SimpleCoating = coatings.SimpleCoating
    GaussianApodization = apodization.GaussianApodization


NS.CookeTriplet = CookeTriplet
NS.RadialAperture = RadialAperture

# |k0 x k1| of every PolarizedRays.update call, in surface order (recorded around the
# reference's method, which is left as it is)
_MAGS = []
_update = PolarizedRays.update


def _recording_update(self, jones_matrix=None):
    k0 = np.stack([self.L0, self.M0, self.N0]).T
    k1 = np.stack([self.L, self.M, self.N]).T
    _MAGS.append(np.linalg.norm(np.cross(k0, k1), axis=1))
    return _update(self, jones_matrix)


PolarizedRays.update = _recording_update


def main():
    out = {}
    for case, spec in pc.CASES.items():
        for tag, kind, args in spec["traces"]:
            base = f"{case}/{tag}"
            geom_done = False
            for state in spec["states"]:
                lens = pc.build(spec["lens"], NS)
                lens.set_polarization("ignore" if state == "ignore"
                                      else create_polarization(state))
                _MAGS.clear()
                rays = lens.trace(*args, "hexapolar") if kind == "trace" \
                    else lens.trace_generic(*(np.array(a) if isinstance(a, list) else a
                                              for a in args))
                n = rays.x.size
                nan = np.isnan(rays.x) | np.isnan(rays.L)
                assert nan.sum() <= 0.1 * n, (case, tag, int(nan.sum()))
                for m in _MAGS:
                    assert not np.any((m > 0) & (m < 1e-8)), (case, tag, state)
                if not geom_done:
                    for a in ("x", "y", "z", "L", "M", "N", "opd"):
                        out[f"{base}/{a}"] = np.asarray(getattr(rays, a), dtype=np.float64)
                if isinstance(rays, PolarizedRays) and f"{base}/p_re" not in out:
                    p = np.asarray(rays.p, dtype=np.complex128)
                    out[f"{base}/p_re"] = np.ascontiguousarray(p.real)
                    out[f"{base}/p_im"] = np.ascontiguousarray(p.imag)
                    out[f"{base}/smin"] = np.array(
                        [np.min(m[m > 0]) if np.any(m > 0) else 0.0 for m in _MAGS])
                geom_done = True
                out[f"{base}/{state}/i"] = np.asarray(rays.i, dtype=np.float64)
                out[f"{base}/{state}/si"] = np.asarray(lens.surface_group.intensity,
                                                       dtype=np.float64)
                print(base, state, n, "nan", int(nan.sum()), "i", float(np.nanmin(rays.i)),
                      float(np.nanmax(rays.i)))
    i1 = out["cooke_fresnel/f1/unpolarized/i"]
    # the known figures of this case, to three decimals
    assert i1.size == 127 and round(i1.min(), 3) == 0.656 and round(i1.max(), 3) == 0.732
    np.savez_compressed(os.path.join(HERE, "polarized.npz"), **out)


if __name__ == "__main__":
    main()
