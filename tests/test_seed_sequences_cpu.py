"""The reciprocal seed of the plain closed-form kernel's conic normal (ort_fastpath.h
normal_conic_rcp<true>), restated operation for operation with an exact fma
(fractions.Fraction, rounded once), and the lowering that feeds it. No GPU.

(2 / R) h: 1 / (R sqrt(1 - q)) seeded from the Goldschmidt root's h and the host's
RN(2 / R); v_rsq is modelled as (1 + e0) / sqrt(x) rounded, e0 = +-2^-20. Each quotient
formed from such a reciprocal must be NumPy's division, bit for bit.
"""
from fractions import Fraction

import numpy as np
import pytest

from tests._fast_sequences import fma, numerators, quot, sqrt_h
from tests._plain_lenses import NOT_PLAIN, PLAIN, build


def test_two_inv_r_h_quotients_are_ieee():
    rng = np.random.default_rng(9)
    xs = [1.0, float(np.nextafter(1.0, 0.0)), 0.75, 0.5, 0.25, 2.0**-10, 2.0**-40,
          2.0**-40 * (1 + 2.0**-52), 2.0**-53]
    xs += [float(v) for v in rng.uniform(0.0, 1.0, 40)]
    radii = [22.01359, -435.76044, 1.0, -1.0, 3.0, 2.0**150, -(2.0**150), 2.0**-150,
             -(2.0**-150), 2.0**150 * (1 - 2.0**-53), 2.0**-150 * (1 + 2.0**-52)]
    radii += [float(v) for v in numerators(rng, 12) if 2.0**-150 <= abs(v) <= 2.0**150]
    for x in xs:
        for e0 in (2.0**-20, -(2.0**-20)):
            g, h = sqrt_h(x, e0)
            assert g == float(np.sqrt(np.float64(x))), (x, e0)
            for R in radii:
                denom = R * g
                two_inv_r = float(np.float64(2.0) / np.float64(R))
                y0 = two_inv_r * h
                # the seed's error, the bound written at normal_conic_rcp
                assert abs(Fraction(denom) * Fraction(y0) - 1) < Fraction(1, 2**39), (x, R)
                e = fma(-denom, y0, 1.0)
                y = fma(y0, e, y0)
                assert abs(Fraction(denom) * Fraction(y) - 1) <= Fraction(1, 2**52), (x, R)
                for n in numerators(rng, 6):
                    n = float(n)
                    exp = float(np.float64(n) / np.float64(denom))  # |exp| in 2^-451 .. 2^478
                    assert quot(n, denom, y) == exp, (x, e0, R, n)


# ---- the lowering -----------------------------------------------------------------------

def _table(lens, wl, record=False):
    from optiland_pr_amd.lowering import lower_surface_group

    return lower_surface_group(lens.surface_group, [wl], record=record)


def _check_two_inv_r(t):
    from optiland_pr_amd import _abi

    s = t.surfaces
    has = (s["flags"] & _abi.SURF_INV_R2) != 0
    bit = (s["flags"] & _abi.SURF_TWO_INV_R) != 0
    np.testing.assert_array_equal(bit, has)
    assert np.all(s["geometry"][has] == _abi.GEOM_STANDARD)
    np.testing.assert_array_equal(s["norm_radius"][has], np.float64(2.0) / s["radius"][has])
    return has


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_lowering_writes_two_inv_r(name):
    from optiland_pr_amd import _abi

    lens, wl = build(name)
    t = _table(lens, wl)
    has = _check_two_inv_r(t)
    assert has.any()
    assert t.frame_flags == _abi.LENS_AXIAL | _abi.LENS_PLAIN
    # surfaces without ORT_SURF_INV_R2 (planes, infinite radii) keep the geometry's value
    for i in np.flatnonzero(~has):
        g = lens.surface_group.surfaces[i + 1].geometry
        assert t.surfaces["norm_radius"][i] == g.lower_params()[4]


@pytest.mark.parametrize("case", NOT_PLAIN)
def test_lowering_of_other_lenses(case):
    from optiland_pr_amd import _abi

    lens, wl, record = build(case)
    t = _table(lens, wl, record)
    _check_two_inv_r(t)
    if case == "conic_without_inv_r2":  # |R| = 2^151: neither bit, and 1.0 as before
        assert t.surfaces["flags"][0] & (_abi.SURF_INV_R2 | _abi.SURF_TWO_INV_R) == 0
        assert t.surfaces["norm_radius"][0] == 1.0
        assert not t.frame_flags & _abi.LENS_PLAIN


@pytest.mark.parametrize("name", ["ReverseTelephotoAsphere", "ForbesSinglets"])
def test_newton_surfaces_keep_norm_radius(name):
    """A Newton surface has neither bit and its own normalisation radius; the finite
    spheres beside it, if any, have both."""
    from optiland_pr_amd import _abi, samples

    lens = getattr(samples, name)()
    t = _table(lens, 0.5876)
    _check_two_inv_r(t)
    newton = np.flatnonzero(np.isin(t.surfaces["geometry"], _abi.NEWTON_GEOMETRIES))
    assert newton.size
    for i in newton:
        g = lens.surface_group.surfaces[i + 1].geometry
        assert t.surfaces["norm_radius"][i] == g.lower_params()[4]


def test_header_and_python_agree():
    import os
    import re

    from optiland_pr_amd import _abi

    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "optiland_rt.h")).read()
    assert re.search(r"ORT_SURF_TWO_INV_R = 1u << (\d+)", text).group(1) == "10"
    assert _abi.SURF_TWO_INV_R == 1 << 10
    assert _abi.ABI_VERSION == int(re.search(r"#define ORT_ABI_VERSION (\d+)", text).group(1)) == 21
    assert _abi.SURFACE.itemsize == 176
