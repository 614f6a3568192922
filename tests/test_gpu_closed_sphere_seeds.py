"""The plain closed-form kernels' sphere branches (k == 0 in the fast pass: the norm's root
seeded from sqrt(1 - q), 1 / a from 2 - a, sqrt(1 - v) without its lower-bound test)
against ORT_OPT_EXACT -- every lane through the generic exact re-trace -- and the NumPy
oracle, bit for bit, with the checks of test_gpu_closed_unit_seeds.py (check_generated:
all eight outputs, NaN payloads and signed zeros included; at least half of the rays of
every case finite).

Ray counts 1, 63, 64, 65, 257 and 4,099 put the last wave at every fill; the mixed lens
runs the k == 0 and the k != 0 branch in one surface loop; the rim hits walk 1 - q down to
2^-53 and past 0. test_sphere_norm_seed_cpu.py runs the sequences with an exact fma.
"""
import dataclasses

import numpy as np
import pytest

from tests._closed import (CONIC, check_generated, launch, optic, pupils_fixture, same_bits,
                           scaled_singlets_case, vertex_and_rim_case)
from tests._closed import torch  # noqa: F401
from tests._plain_lenses import PLAIN, build

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 257, 4099)
pupils = pupils_fixture(1 << 16, seeds=(4,), grids=(129,))  # test_gpu_closed_unit_seeds.py's


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
        check_generated(torch, dl, seg, px[:n], py[:n], f"{name} hy={hy} n={n}", wl)


@pytest.mark.parametrize("hy", [0.0, 1.0])
def test_spheres_and_conics_in_one_lens(torch, pupils, hy):
    """Three spheres and three k != 0 conics, alternating: both branches of the normal and
    of the quadratic in every wave's surface loop."""
    from optiland_pr_amd.lowering import segment_params
    from optiland_pr_amd.raytrace import lens_for

    lens = optic(CONIC, fields=(0.0, 10.0))
    dl = lens_for(lens, [0.55])
    k = dl.table.surfaces["conic"][:6]
    assert np.count_nonzero(k) == 3 and np.count_nonzero(k == 0.0) == 3
    seg = segment_params(lens, 0.0, hy, 0)
    px, py = pupils["seed4"]
    for n in COUNTS:
        check_generated(torch, dl, seg, px[:n], py[:n], f"mixed hy={hy} n={n}")
    px, py = pupils["uniform129"]
    check_generated(torch, dl, seg, px, py, f"mixed grid hy={hy}")


@pytest.mark.parametrize("hy", [0.0, 1.0])
@pytest.mark.parametrize("exp", [140, -140])
def test_scaled_singlets(torch, pupils, exp, hy):
    scaled_singlets_case(torch, pupils, exp, hy, check_generated)


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
    with_bit = launch(torch, dl, seg, px, py, False, wl)
    for step in (1, 2):
        surfaces = dl.table.surfaces.copy()
        surfaces["flags"][::step] &= ~_abi.SURF_TWO_INV_R
        assert np.any(surfaces["flags"] != dl.table.surfaces["flags"])
        off = DeviceLens(dataclasses.replace(dl.table, surfaces=surfaces))
        assert off.c.frame_flags == dl.c.frame_flags
        same_bits(with_bit, launch(torch, off, seg, px, py, False, wl), f"{name} step {step}")
        check_generated(torch, off, seg, px, py, f"{name} cleared, step {step}", wl)


def test_vertex_and_rim_hits(torch):
    """A singlet whose front radius is EPD / 2, on axis: pupil point p meets the front
    sphere at r = |p| R, so 1 - q = 1 - |p|^2. |p| = sqrt(1 - 2^-j) with its neighbours for
    j = 10 .. 53 (1 - q down to its last positive values), |p| >= 1 (1 - q <= 0: NaN on both
    launches), the vertex through +-0, and fans of ordinary rays, which are the finite
    half of the case."""
    vertex_and_rim_case(torch, check_generated)
