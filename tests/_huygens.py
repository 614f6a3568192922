"""Shared by tests/test_huygens_cpu.py and tests/test_gpu_huygens.py: the fixture
(tests/golden/huygens.npz, written by tests/golden/gen_huygens_golden.py from the
reference's HuygensPSF), the error bound, and the synthetic chunk-edge problems with their
NumPy restatement.

The bound (PSF units: the ideal peak is 100). Each term's phase carries a few fp64 roundings
of a quantity of size k R_max = 2 pi R_max / lambda, so |d field| <= c k R_max 2^-53
sum |A_j|, and for PSF <= 100: |d PSF| <= 200 c k R_max 2^-53 with c = 8 (the difference,
the sum of squares, the sqrt, the subtraction of opd, the division by lambda, the
reduction). Relative tolerance 0. Every test computes it from its own arrays.
"""

import functools
import os

import numpy as np

from optiland_pr_amd import _abi

CASES = ("cooke_00", "cooke_01", "dg_007", "cooke_pitch", "cooke_oversample")
IMAGE = ("image_x", "image_y", "image_z")
PUPIL = ("pupil_x", "pupil_y", "pupil_z", "amp", "opd_mm")
CHUNK = _abi.HUYGENS_CHUNK
PUPIL_SIZES = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
IMAGE_SIZES = (1, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def fixture():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "huygens.npz")
    g = np.load(path, allow_pickle=False)
    out = {}
    for k in g.files:
        case, name = k.split("/")
        a = g[k]
        a.setflags(write=False)
        out.setdefault(case, {})[name] = a
    return out


def r_max(image, pupil):
    d2 = sum((np.reshape(i, (-1, 1)) - p) ** 2 for i, p in zip(image, pupil[:3], strict=True))
    return float(np.sqrt(np.max(d2)))


def r_min(image, pupil):
    d2 = sum((np.reshape(i, (-1, 1)) - p) ** 2 for i, p in zip(image, pupil[:3], strict=True))
    return float(np.sqrt(np.min(d2)))


def bound(image, pupil, wavelength_mm):
    return 100.0 * 2.0 * 8.0 * (2.0 * np.pi * r_max(image, pupil) / wavelength_mm) * 2.0 ** -53


def case_arrays(case):
    c = fixture()[case]
    image = [c[a] for a in IMAGE]
    pupil = [c[a] for a in PUPIL]
    return c, image, pupil, bound(image, pupil, float(c["wavelength_mm"]))


# -- synthetic problems at the chunk and tile edges ------------------------------------
RP = 50.0
WAVELENGTH_MM = 0.55e-3


@functools.lru_cache(maxsize=None)
def synthetic(n_image, n_pupil):
    """Seeded: n_pupil points on the sphere of radius 50 mm about the origin (a cap of
    +-6 mm behind the image), a fifth of them with amp == 0, OPDs of a few waves; n_image
    points within +-20 um of the origin. -> (image[3], pupil[5], expected raw |field|^2,
    scale = (sum amp / R_min)^2, atol in units of 100 / scale)."""
    g = np.random.default_rng(1000 * n_image + n_pupil)
    u = g.uniform(-6.0, 6.0, n_pupil)
    v = g.uniform(-6.0, 6.0, n_pupil)
    w = -np.sqrt(RP * RP - u * u - v * v)
    amp = g.uniform(0.2, 1.0, n_pupil)
    amp[g.random(n_pupil) < 0.2] = 0.0
    opd = g.uniform(-3.0, 3.0, n_pupil) * WAVELENGTH_MM
    image = [g.uniform(-0.02, 0.02, n_image) for _ in range(3)]
    pupil = [u, v, w, amp, opd]
    expected = restatement(image, pupil, WAVELENGTH_MM, RP)
    scale = float((np.sum(amp) / r_min(image, pupil)) ** 2)
    for a in (*image, *pupil, expected):
        a.setflags(write=False)
    return image, pupil, expected, scale, bound(image, pupil, WAVELENGTH_MM)


def restatement(image, pupil, wavelength_mm, rp):
    """The Huygens-Fresnel sum in whole-array NumPy (huygens_fresnel_strategies.py:124-171
    restated): |sum_j amp_j (1 + cos theta) / 2 exp(i k (R - opd_j)) / R|^2, the phase
    reduced to a fraction of a cycle before the exponential, pairwise sums."""
    x, y, z = (np.reshape(a, (-1, 1)) for a in image)
    u, v, w, amp, opd = pupil
    dx, dy, dz = x - u, y - v, z - w
    R = np.sqrt(dx * dx + dy * dy + dz * dz)
    cos_t = (dx * u + dy * v + dz * w) / (rp * R)
    t = (R - opd) / wavelength_mm
    field = np.sum(amp * 0.5 * (1.0 + cos_t) / R * np.exp(2j * np.pi * (t - np.rint(t))),
                   axis=1)
    return field.real ** 2 + field.imag ** 2
