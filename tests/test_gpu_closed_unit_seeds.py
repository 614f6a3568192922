"""The plain closed-form kernels' fast pass (generated rays on ORT_LENS_PLAIN lenses) with
the conic normal's 1 / denom seeded from (2 / R) h (ORT_SURF_TWO_INV_R,
normal_conic_rcp<true>), against ORT_OPT_EXACT -- the same kernel with every lane sent
through the generic exact re-trace -- and against the NumPy oracle.

Default launch vs ORT_OPT_EXACT: the same bits in all eight outputs, NaN payloads and
signed zeros included. Against the oracle (at most 4,099 rays of a case): the same NaN
masks, values and zero signs; the intensity to rtol 1e-12, as everywhere in the suite.

Not checked here: which pass a lane took (the closed-form kernel reports no `bad` lanes);
profiles/r10_closed_unit_seeds.md sets the default launch's kernel time beside the exact
launch's. test_seed_sequences_cpu.py runs the seeded sequence with an exact fma.
"""
import dataclasses

import numpy as np
import pytest

from tests._closed import (CONIC, HALF_BALL, N_ORACLE, check_generated, launch, optic,
                           pupils_fixture, same_bits, scaled_singlet)
from tests._closed import torch  # noqa: F401
from tests._plain_lenses import PLAIN, build

pytestmark = pytest.mark.gpu

# one seed of 2^16 random pupil points and the uniform 129 grid, whose centre column and row
# are +0 (sdiv0's zero numerator over the seeded divisor)
pupils = pupils_fixture(1 << 16, seeds=(4,), grids=(129,))


@pytest.mark.parametrize("hy", [0.0, 0.7, 1.0])
@pytest.mark.parametrize("name", sorted(PLAIN))
def test_sample_objectives(torch, pupils, name, hy):
    from optiland_pr_amd import _abi
    from optiland_pr_amd.lowering import segment_params
    from optiland_pr_amd.raytrace import lens_for

    lens, wl = build(name)
    dl = lens_for(lens, [wl])
    f = dl.table.surfaces["flags"]
    assert np.any(f & _abi.SURF_TWO_INV_R)
    seg = segment_params(lens, 0.0, hy, 0)
    for pname, (px, py) in pupils.items():
        check_generated(torch, dl, seg, px, py, f"{name} hy={hy} {pname}", wl)


@pytest.mark.parametrize("hy", [0.0, 1.0])
def test_conic_constants(torch, pupils, hy):
    """k != 0 on three of six spheres: the normal's seed meets 1 + k."""
    from optiland_pr_amd.lowering import segment_params
    from optiland_pr_amd.raytrace import lens_for

    lens = optic(CONIC, fields=(0.0, 10.0))
    dl = lens_for(lens, [0.55])
    assert np.count_nonzero(dl.table.surfaces["conic"]) == 3
    px, py = pupils["seed4"]
    check_generated(torch, dl, segment_params(lens, 0.0, hy, 0), px[:8192], py[:8192],
                    f"conic hy={hy}")
    px, py = pupils["uniform129"]
    check_generated(torch, dl, segment_params(lens, 0.0, hy, 0), px, py, f"conic grid hy={hy}")


@pytest.mark.parametrize("hy", [0.0, 1.0])
@pytest.mark.parametrize("exp", [140, -140, 150, -150])
def test_scaled_singlet(torch, pupils, exp, hy):
    """Every length, the aperture included, times 2^+-140; and times 2^+-150, where |R| is
    at the ends of the ORT_SURF_INV_R2 range and 2 / R is 2^-+149."""
    from optiland_pr_amd import _abi
    from optiland_pr_amd.raytrace import lens_for

    scale = 2.0**exp
    lens, seg = scaled_singlet(scale, hy)
    dl = lens_for(lens, [0.55])
    s = dl.table.surfaces
    assert np.all(s["flags"][:2] & _abi.SURF_TWO_INV_R)
    np.testing.assert_array_equal(s["norm_radius"][:2], [2.0 / scale, -2.0 / scale])
    px, py = pupils["seed4"]
    check_generated(torch, dl, seg, px[:N_ORACLE], py[:N_ORACLE], f"singlet 2^{exp} hy={hy}")


@pytest.mark.parametrize("which", ["all", "every_other"])
@pytest.mark.parametrize("name", sorted(PLAIN))
def test_tables_without_the_bit(torch, pupils, name, which):
    """The same lowered table with ORT_SURF_TWO_INV_R cleared on every surface, and on
    every other surface (another producer's table: shared_div(denom)): the same bits."""
    from optiland_pr_amd import _abi
    from optiland_pr_amd.lowering import segment_params
    from optiland_pr_amd.raytrace import DeviceLens, lens_for

    lens, wl = build(name)
    dl = lens_for(lens, [wl])
    surfaces = dl.table.surfaces.copy()
    step = 1 if which == "all" else 2
    surfaces["flags"][::step] &= ~_abi.SURF_TWO_INV_R
    assert np.any(surfaces["flags"] != dl.table.surfaces["flags"])
    off = DeviceLens(dataclasses.replace(dl.table, surfaces=surfaces))
    assert off.c.frame_flags == dl.c.frame_flags
    seg = segment_params(lens, 0.0, 0.7, 0)
    px, py = pupils["uniform129"]
    same_bits(launch(torch, dl, seg, px, py, False, wl),
              launch(torch, off, seg, px, py, False, wl), f"{name} bit cleared on {which}")
    check_generated(torch, off, seg, px[:N_ORACLE], py[:N_ORACLE], f"{name} cleared {which}", wl)


def test_rim_and_vertex_hits(torch):
    """A singlet whose front radius is EPD / 2, on axis: the ray of pupil point (px, py)
    meets the front sphere at r = |p| R, so 1 - q = 1 - |p|^2. |p| = sqrt(1 - 2^-j),
    j = 10 .. 40, with its neighbours (steep normals: most of these rays are totally
    reflected or miss the back surface, and NaNs compare too), |p| > 1 (misses: NaN on
    both), the vertex through +-0, and a fan of ordinary rays that pass."""
    from optiland_pr_amd.lowering import segment_params
    from optiland_pr_amd.raytrace import lens_for

    lens = optic(HALF_BALL)
    dl = lens_for(lens, [0.55])
    seg = segment_params(lens, 0.0, 0.0, 0)
    assert float(seg["epd"]) == 2.0 * 5.0 and float(seg["x_off"]) == 0.0
    pts = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)]
    n_vertex = len(pts)
    fan = np.linspace(-0.6, 0.6, 41)
    pts += [(float(v), 0.0) for v in fan] + [(0.0, float(v)) for v in fan]
    pts += [(float(v) * 0.6, float(v) * 0.8) for v in fan]
    n_pass = len(pts)
    for j in (10, 20, 30, 36, 40):
        p = np.sqrt(1.0 - 2.0**-j)
        for h in (p, np.nextafter(p, 0.0), np.nextafter(p, 2.0)):
            for cx, cy in ((1.0, 0.0), (0.0, -1.0), (0.6, 0.8), (-1.0, 0.0)):
                pts.append((h * cx, h * cy))
    for p in (1.0, np.nextafter(1.0, 2.0), 1.0 + 2.0**-20, 1.5):
        pts += [(p, 0.0), (0.0, -p), (-p * 0.6, p * 0.8)]
    px, py = (np.array(c, dtype=np.float64) for c in zip(*pts))
    got = check_generated(torch, dl, seg, px, py, "rim and vertex", min_finite=0.0)
    assert np.isfinite(got["x"][n_vertex:n_pass]).all()  # the fan passes
    assert np.isfinite(got["x"][:n_vertex]).any()
    assert np.isnan(got["x"][px * px + py * py > 1.0 + 2.0**-19]).all()  # the misses
