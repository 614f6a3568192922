"""Lenses of the ORT_LENS_PLAIN tests: the sample objectives that lower plain, and one lens
per reason not to (test_lowering_plain_cpu.py, test_gpu_closed_plain.py)."""
import numpy as np

PLAIN = {"DoubleGauss": 0.5876, "CookeTriplet": 0.55, "ReverseTelephoto": 0.5876}
NOT_PLAIN = ("radial_aperture", "aperture_program", "mirror", "recorded", "decentred",
             "conic_without_inv_r2")

_MIRROR = [
    dict(radius=np.inf, thickness=np.inf),
    dict(radius=40.0, thickness=5.0, material="SK16", is_stop=True),
    dict(radius=np.inf, thickness=30.0),
    dict(radius=-120.0, thickness=-25.0, material="mirror"),
    dict(),
]
# |R| = 2^151 is outside the range in which the host forms inv_r2 (2^-150 .. 2^150)
_FLAT_SINGLET = [
    dict(radius=np.inf, thickness=np.inf),
    dict(radius=2.0**151, thickness=3.0, material="SK16", is_stop=True),
    dict(radius=-50.0, thickness=40.0),
    dict(),
]


def _optic(rows):
    from optiland_pr_amd.optic import Optic

    lens = Optic()
    for i, row in enumerate(rows):
        lens.add_surface(index=i, **row)
    lens.set_aperture(aperture_type="EPD", value=10)
    lens.set_field_type(field_type="angle")
    lens.add_field(y=0)
    lens.add_wavelength(value=0.55, is_primary=True)
    return lens


def build(name):
    """PLAIN name -> (lens, wavelength); NOT_PLAIN name -> (lens, wavelength, record)."""
    from optiland_pr_amd import samples
    from optiland_pr_amd.apertures import RadialAperture, RectangularAperture

    if name in PLAIN:
        return getattr(samples, name)(), PLAIN[name]
    if name == "radial_aperture":
        lens = samples.CookeTriplet()
        lens.surface_group.surfaces[3].aperture = RadialAperture(r_max=4.5)
        lens.invalidate()
    elif name == "aperture_program":
        lens = samples.CookeTriplet()
        lens.surface_group.surfaces[2].aperture = RectangularAperture(-4.0, 4.0, -3.0, 3.5)
        lens.invalidate()
    elif name == "mirror":
        lens = _optic(_MIRROR)
    elif name == "recorded":
        lens = samples.CookeTriplet()
    elif name == "decentred":
        lens = samples.DecenteredTriplet()
    elif name == "conic_without_inv_r2":
        lens = _optic(_FLAT_SINGLET)
    else:
        raise KeyError(name)
    return lens, 0.55, name == "recorded"
