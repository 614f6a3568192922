"""The plain closed-form kernels' sphere branches (k == 0 in the fast pass: the norm's root
seeded from sqrt(1 - q), 1 / a from 2 - a, sqrt(1 - v) without its lower-bound test)
against ORT_OPT_EXACT -- every lane through the generic exact re-trace -- and the NumPy
oracle, bit for bit, with the checks of test_gpu_closed_unit_seeds.py (_check_generated:
all eight outputs, NaN payloads and signed zeros included; at least half of the rays of
every case finite).

Ray counts 1, 63, 64, 65, 257 and 4,099 put the last wave at every fill; the mixed lens
runs the k == 0 and the k != 0 branch in one surface loop; the rim hits walk 1 - q down to
2^-53 and past 0. test_sphere_norm_seed_cpu.py runs the sequences with an exact fma.
"""
import dataclasses

import numpy as np
import pytest

from tests._plain_lenses import PLAIN, build
from tests.test_gpu_closed_unit_seeds import (_CONIC, _check_generated, _launch, _optic,  # noqa: F401
                                              _same_bits, _scaled_singlet, pupils, torch)

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 257, 4099)


@pytest.mark.parametrize("hy", [0.0, 0.7, 1.0])
@pytest.mark.parametrize("name", sorted(PLAIN))
def test_sample_objectives_at_wave_edges(torch, pupils, name, hy):
    from optiland_pr_amd.lowering import segment_params
    from optiland_pr_amd.raytrace import lens_for

    lens, wl = build(name)
    dl = lens_for(lens, [wl])
    assert np.any(dl.table.surfaces["conic"] == 0.0)
    seg = segment_params(lens, 0.0, hy, 0)
    px, py = pupils["seed4"]
    for n in COUNTS:
        _check_generated(torch, dl, seg, px[:n], py[:n], f"{name} hy={hy} n={n}", wl)


@pytest.mark.parametrize("hy", [0.0, 1.0])
def test_spheres_and_conics_in_one_lens(torch, pupils, hy):
    """Three spheres and three k != 0 conics, alternating: both branches of the normal and
    of the quadratic in every wave's surface loop."""
    from optiland_pr_amd.lowering import segment_params
    from optiland_pr_amd.raytrace import lens_for

    lens = _optic(_CONIC, fields=(0.0, 10.0))
    dl = lens_for(lens, [0.55])
    k = dl.table.surfaces["conic"][:6]
    assert np.count_nonzero(k) == 3 and np.count_nonzero(k == 0.0) == 3
    seg = segment_params(lens, 0.0, hy, 0)
    px, py = pupils["seed4"]
    for n in COUNTS:
        _check_generated(torch, dl, seg, px[:n], py[:n], f"mixed hy={hy} n={n}")
    px, py = pupils["uniform129"]
    _check_generated(torch, dl, seg, px, py, f"mixed grid hy={hy}")


@pytest.mark.parametrize("hy", [0.0, 1.0])
@pytest.mark.parametrize("exp", [140, -140])
def test_scaled_singlets(torch, pupils, exp, hy):
    from optiland_pr_amd.raytrace import lens_for

    lens, seg = _scaled_singlet(2.0**exp, hy)
    dl = lens_for(lens, [0.55])
    assert np.all(dl.table.surfaces["conic"][:2] == 0.0)
    px, py = pupils["seed4"]
    for n in (65, 4099):
        _check_generated(torch, dl, seg, px[:n], py[:n], f"singlet 2^{exp} hy={hy} n={n}")


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_tables_without_the_bit(torch, pupils, name):
    """ORT_SURF_TWO_INV_R cleared on every surface, and on every other one: those spheres
    keep v_rsq(X); the same bits as with the bit."""
    from optiland_pr_amd import _abi
    from optiland_pr_amd.lowering import segment_params
    from optiland_pr_amd.raytrace import DeviceLens, lens_for

    lens, wl = build(name)
    dl = lens_for(lens, [wl])
    seg = segment_params(lens, 0.0, 0.7, 0)
    px, py = (c[:4099] for c in pupils["seed4"])
    with_bit = _launch(torch, dl, seg, px, py, False, wl)
    for step in (1, 2):
        surfaces = dl.table.surfaces.copy()
        surfaces["flags"][::step] &= ~_abi.SURF_TWO_INV_R
        assert np.any(surfaces["flags"] != dl.table.surfaces["flags"])
        off = DeviceLens(dataclasses.replace(dl.table, surfaces=surfaces))
        assert off.c.frame_flags == dl.c.frame_flags
        _same_bits(with_bit, _launch(torch, off, seg, px, py, False, wl), f"{name} step {step}")
        _check_generated(torch, off, seg, px, py, f"{name} cleared, step {step}", wl)


def test_vertex_and_rim_hits(torch):
    """A singlet whose front radius is EPD / 2, on axis: pupil point p meets the front
    sphere at r = |p| R, so 1 - q = 1 - |p|^2. |p| = sqrt(1 - 2^-j) with its neighbours for
    j = 10 .. 53 (1 - q down to its last positive values), |p| >= 1 (1 - q <= 0: NaN on both
    launches), the vertex through +-0, and fans of ordinary rays, which are the finite
    half of the case."""
    from optiland_pr_amd.lowering import segment_params
    from optiland_pr_amd.raytrace import lens_for

    rows = [
        dict(radius=np.inf, thickness=np.inf),
        dict(radius=5.0, thickness=6.0, material="SK16", is_stop=True),
        dict(radius=-40.0, thickness=20.0),
        dict(),
    ]
    lens = _optic(rows)
    dl = lens_for(lens, [0.55])
    seg = segment_params(lens, 0.0, 0.0, 0)
    assert float(seg["epd"]) == 2.0 * 5.0 and float(seg["x_off"]) == 0.0
    pts = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)]
    n_vertex = len(pts)
    fan = np.linspace(-0.6, 0.6, 81)
    pts += [(float(v), 0.0) for v in fan] + [(0.0, float(v)) for v in fan]
    pts += [(float(v) * 0.6, float(v) * 0.8) for v in fan]
    n_pass = len(pts)
    for j in (10, 20, 30, 36, 40, 46, 50, 52, 53):
        p = np.sqrt(1.0 - 2.0**-j)
        for h in (p, np.nextafter(p, 0.0), np.nextafter(p, 2.0)):
            for cx, cy in ((1.0, 0.0), (0.0, -1.0), (0.6, 0.8), (-1.0, 0.0)):
                pts.append((h * cx, h * cy))
    for p in (1.0, np.nextafter(1.0, 2.0), 1.0 + 2.0**-20, 1.5):
        pts += [(p, 0.0), (0.0, -p), (-p * 0.6, p * 0.8)]
    px, py = (np.array(c, dtype=np.float64) for c in zip(*pts))
    got = _check_generated(torch, dl, seg, px, py, "vertex and rim")
    assert np.isfinite(got["x"][n_vertex:n_pass]).all()  # the fans pass
    assert np.isfinite(got["x"][:n_vertex]).all()
    assert np.isnan(got["x"][px * px + py * py > 1.0 + 2.0**-19]).all()  # the misses
