"""The BSDF golden cases, shared by gen_bsdf_golden.py (run against the reference) and the
tests (run against this package): builders take a namespace NS with Optic, IdealMaterial,
LambertianBSDF and GaussianBSDF, so the same calls build the lens on either side."""

from __future__ import annotations

import numpy as np

N_RAYS = 257
SURFACE_INDEX = 3  # counter word 2 of the step-level cases

# step-level cases: name -> (normal kind, bsdf spec)
STEP_CASES = {
    f"{nrm}_{tag}": (nrm, spec)
    for nrm in ("plane", "conic")
    for tag, spec in (("lambertian", ("LambertianBSDF",)), ("gauss005", ("GaussianBSDF", 0.05)),
                      ("gauss05", ("GaussianBSDF", 0.5)))
}
CONIC = dict(radius=50.0, conic=-0.5)

LENS_WAVELENGTH = 0.55
LENS_FIELD = (0.0, 0.5)
LENS_SIGMA = 0.05


def make_bsdf(spec, NS):
    return getattr(NS, spec[0])(*spec[1:])


def step_directions():
    """257 unit directions: incidences from normal to 85 degrees over all azimuths, ray 255
    with L >= 0.999 (the other auxiliary vector) and ray 256 NaN."""
    k = np.arange(N_RAYS, dtype=np.float64)
    theta = np.radians(85.0) * k / (N_RAYS - 3)
    phi = 2.399963229728653 * k  # the golden angle
    L = np.sin(theta) * np.cos(phi)
    M = np.sin(theta) * np.sin(phi)
    N = np.cos(theta)
    L[255], M[255] = 0.9995, 0.0
    N[255] = np.sqrt(1.0 - 0.9995 ** 2)
    L[256] = np.nan
    return L, M, N


def step_points():
    """(x, y) of the 257 points whose conic normals the step cases use (radius <= 20)."""
    k = np.arange(N_RAYS, dtype=np.float64)
    r = 20.0 * np.sqrt((k + 0.5) / N_RAYS)
    phi = 2.399963229728653 * k + 1.0
    return r * np.cos(phi), r * np.sin(phi)


def lens_pupil():
    """257 pupil points inside the 0.95 disk."""
    k = np.arange(N_RAYS, dtype=np.float64)
    r = 0.95 * np.sqrt((k + 0.5) / N_RAYS)
    phi = 2.399963229728653 * k
    return r * np.cos(phi), r * np.sin(phi)


def build_lens(NS):
    """A singlet whose back surface carries a Gaussian BSDF, then a Lambertian plane mirror.
    (The mirror's raw normal is (0, 0, 1), so its scattered rays leave towards +z: the image
    plane lies behind it.)"""
    lens = NS.Optic()
    glass = NS.IdealMaterial(n=1.5)
    lens.add_surface(index=0, radius=np.inf, thickness=np.inf)
    lens.add_surface(index=1, radius=50.0, thickness=5.0, material=glass, is_stop=True)
    lens.add_surface(index=2, radius=-50.0, thickness=20.0,
                     bsdf=NS.GaussianBSDF(LENS_SIGMA))
    lens.add_surface(index=3, radius=np.inf, thickness=10.0, material="mirror",
                     bsdf=NS.LambertianBSDF())
    lens.add_surface(index=4)
    lens.set_aperture(aperture_type="EPD", value=10.0)
    lens.set_field_type(field_type="angle")
    lens.add_field(y=0.0)
    lens.add_field(y=5.0)
    lens.add_wavelength(value=LENS_WAVELENGTH, is_primary=True)
    return lens
