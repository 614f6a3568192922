"""Huygens-Fresnel PSF golden vectors: the REFERENCE's HuygensPSF
(optiland/psf/huygens_fresnel.py, its NumbaSummation loop of
psf/huygens_fresnel_strategies.py:97-172) on small images and pupils of the sample lenses.

Test infrastructure only, run in the build container (never on the GPU box):

    PYTHONPATH=tests/golden/shims:/root/reference PYTHONDONTWRITEBYTECODE=1 \
        python tests/golden/gen_huygens_golden.py

(tests/golden/shims/numba.py stands in for numba: @njit(parallel=True) is the identity and
prange is range, so the reference's double loop runs as the plain Python it is.)

Writes tests/golden/huygens.npz, arrays "<case>/<name>". Per case: the image grids the
reference summed over (image_x / y / z, global frame), the pupil it summed (pupil_x / y / z,
amp, opd_mm), radius, wavelength_mm, the raw ideal peak `norm`, the reference's psf,
pixel_pitch, cx, cy, strehl and working_fno, and ref_self_diff: the largest difference
between the reference's psf and the same sum recomputed here with vectorised NumPy in
another association order (the same factors per term, np.sum's pairwise tree over the pupil)
-- the reference's own floating-point noise floor, asserted to sit a factor 100 inside the
tests' bound

    atol = 100 * 2 * 8 * (2 pi R_max / wavelength_mm) * 2**-53      (PSF units, ideal peak 100)
"""

from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

import optiland.backend as be  # noqa: E402
from optiland.psf import HuygensPSF  # noqa: E402
from optiland.samples.objectives import CookeTriplet, DoubleGauss  # noqa: E402

be.set_backend("numpy")

CASES = {  # name -> (lens builder, field, wavelength um, num_rays, image_size, keywords)
    "cooke_00": (CookeTriplet, (0, 0), 0.55, 16, 15, {}),
    "cooke_01": (CookeTriplet, (0, 1), 0.55, 16, 16, {}),
    "dg_007": (DoubleGauss, (0, 0.7), 0.5876, 20, 16, {}),
    "cooke_pitch": (CookeTriplet, (0, 0.7), 0.48, 16, 9,
                    {"pixel_pitch": 0.001, "remove_tilt": True}),
    "cooke_oversample": (CookeTriplet, (0, 0), 0.55, 16, 8, {"oversample": 2.0}),
}


class Recording(HuygensPSF):
    """The reference class, keeping the image grid and the normalisation it used."""

    def _get_image_coordinates(self):
        self.coords = super()._get_image_coordinates()
        return self.coords

    def _get_normalization(self):
        self.norm = super()._get_normalization()
        return self.norm


def distances(ix, iy, iz, px, py, pz):
    return np.sqrt((ix.reshape(-1, 1) - px) ** 2 + (iy.reshape(-1, 1) - py) ** 2
                   + (iz.reshape(-1, 1) - pz) ** 2)


def bound(r_max, wavelength_mm):
    return 100.0 * 2.0 * 8.0 * (2.0 * np.pi * r_max / wavelength_mm) * 2.0 ** -53


def vectorised_raw(ix, iy, iz, px, py, pz, amp, opd, wavelength_mm, rp):
    """|field|^2 by whole-array NumPy: the reference's factors per term
    (huygens_fresnel_strategies.py:143-166), added by np.sum's pairwise tree over the pupil
    where the reference's loop adds them one after the other."""
    k = 2.0 * np.pi / wavelength_mm
    dx, dy, dz = ix.reshape(-1, 1) - px, iy.reshape(-1, 1) - py, iz.reshape(-1, 1) - pz
    R = np.sqrt(dx * dx + dy * dy + dz * dz)
    wave = np.exp(1j * k * R) / R
    obliq = 0.5 * (1.0 + (dx * (px / rp) + dy * (py / rp) + dz * (pz / rp)) / R)
    field = np.sum(amp * np.exp(-1j * k * opd) * wave * obliq, axis=1)
    return (field.real ** 2 + field.imag ** 2).reshape(ix.shape)


def main():
    arrays = {}
    for key, (builder, field, wl, num_rays, image_size, kw) in CASES.items():
        p = Recording(builder(), field, wl, num_rays=num_rays, image_size=image_size, **kw)
        d = p.get_data(p.fields[0], p.wavelengths[0])
        wavelength_mm = wl * 1e-3
        ix, iy, iz = (np.asarray(c, dtype=np.float64) for c in p.coords)
        pupil = [np.asarray(getattr(d, a), dtype=np.float64)
                 for a in ("pupil_x", "pupil_y", "pupil_z", "intensity")]
        opd_mm = np.asarray(d.opd, dtype=np.float64) * wavelength_mm
        assert np.all(pupil[3] > 0), f"{key}: vignetted pupil points"
        psf = np.asarray(p.psf, dtype=np.float64)
        norm = float(p.norm)
        again = vectorised_raw(ix, iy, iz, *pupil, opd_mm, wavelength_mm, float(d.radius))
        self_diff = float(np.max(np.abs(again / norm * 100.0 - psf)))
        atol = bound(float(np.max(distances(ix, iy, iz, *pupil[:3]))), wavelength_mm)
        assert self_diff < atol / 100.0, (key, self_diff, atol)
        out = dict(image_x=ix, image_y=iy, image_z=iz, pupil_x=pupil[0], pupil_y=pupil[1],
                   pupil_z=pupil[2], amp=pupil[3], opd_mm=opd_mm, radius=float(d.radius),
                   wavelength_mm=wavelength_mm, norm=norm, psf=psf,
                   pixel_pitch=float(p.pixel_pitch), cx=float(p.cx), cy=float(p.cy),
                   strehl=float(p.strehl_ratio()), working_fno=float(p._get_working_FNO()),
                   ref_self_diff=self_diff)
        for name, v in out.items():
            arrays[f"{key}/{name}"] = np.asarray(v, dtype=np.float64)
        print(f"{key}: {pupil[0].size} pupil points, strehl {out['strehl']:.6f}, "
              f"self diff {self_diff:.3g}, atol {atol:.3g}")
    np.savez_compressed(os.path.join(HERE, "huygens.npz"), **arrays)


if __name__ == "__main__":
    main()
