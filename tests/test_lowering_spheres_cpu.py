"""ORT_LENS_SPHERES in the lowered lens's form_flags: set for the sample objectives, clear
as soon as one of its conditions fails -- a surface that is neither a plane nor a standard
surface, a conic constant other than 0.0, an infinite-radius standard surface, a standard
surface without ORT_SURF_TWO_INV_R -- and clear whenever ORT_LENS_PLAIN is. No GPU.

The bit has a word of its own (ort_lens.form_flags, the former `reserved`): frame_flags
stays ORT_LENS_AXIAL | ORT_LENS_PLAIN for the sample objectives, as every caller and test
that compares it whole expects."""
import dataclasses

import numpy as np
import pytest

from tests._plain_lenses import NOT_PLAIN, PLAIN, build


def _table(lens, wl, record=False):
    from optiland_pr_amd.lowering import lower_surface_group

    return lower_surface_group(lens.surface_group, [wl], record=record)


def _rows(conic=0.0, flat=False, r151=False):
    """A cemented doublet; one surface varied."""
    return [
        dict(radius=np.inf, thickness=np.inf),
        dict(radius=60.0, thickness=4.0, material="SK16", is_stop=True, conic=conic),
        dict(radius=np.inf if flat else (2.0**151 if r151 else -45.0), thickness=2.0,
             material=("F2", "schott")),
        dict(radius=-120.0, thickness=80.0),
        dict(),
    ]


def _optic(rows):
    from tests._plain_lenses import _optic as make

    return make(rows)


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_sample_objectives_are_all_spheres(name):
    from optiland_pr_amd import _abi

    lens, wl = build(name)
    t = _table(lens, wl)
    assert t.form_flags == _abi.LENS_SPHERES
    assert t.frame_flags == _abi.LENS_AXIAL | _abi.LENS_PLAIN  # the bit is not in this word


def test_the_doublet_itself_is_all_spheres():
    from optiland_pr_amd import _abi

    t = _table(_optic(_rows()), 0.55)
    assert t.frame_flags & _abi.LENS_PLAIN and t.form_flags == _abi.LENS_SPHERES
    std = t.surfaces["geometry"] == _abi.GEOM_STANDARD
    assert std.sum() == 3 and np.any(t.surfaces["geometry"] == _abi.GEOM_PLANE)


def test_a_conic_constant_clears_the_bit():
    from optiland_pr_amd import _abi

    for k in (-0.5, 5e-324, -1.0):
        t = _table(_optic(_rows(conic=k)), 0.55)
        assert t.frame_flags & _abi.LENS_PLAIN, k  # still plain: only the new bit goes
        assert t.form_flags == 0, k
    # -0.0 == 0.0: 1 + k is 1.0 and k N^2 terms do not exist in the sphere branch the plain
    # form already takes for it
    assert _table(_optic(_rows(conic=-0.0)), 0.55).form_flags == _abi.LENS_SPHERES


def test_an_infinite_radius_standard_surface_clears_the_bit():
    from optiland_pr_amd import _abi

    t = _table(_optic(_rows(flat=True)), 0.55)
    s = t.surfaces
    flat = (s["geometry"] == _abi.GEOM_STANDARD) & ((s["flags"] & _abi.SURF_RADIUS_INF) != 0)
    if not flat.any():  # the lowering turned it into a plane: make it a standard surface
        s = s.copy()
        i = int(np.flatnonzero(np.isinf(s["radius"]))[0])
        s["geometry"][i] = _abi.GEOM_STANDARD
        s["flags"][i] |= _abi.SURF_RADIUS_INF
        t = dataclasses.replace(t, surfaces=s)
    assert t.frame_flags & _abi.LENS_PLAIN
    assert t.form_flags == 0


def test_a_surface_without_two_inv_r_clears_the_bit():
    from optiland_pr_amd import _abi

    t = _table(_optic(_rows()), 0.55)
    std = np.flatnonzero(t.surfaces["geometry"] == _abi.GEOM_STANDARD)
    for i in std:
        s = t.surfaces.copy()
        s["flags"][i] &= ~_abi.SURF_TWO_INV_R
        off = dataclasses.replace(t, surfaces=s)
        assert off.frame_flags & _abi.LENS_PLAIN
        assert off.form_flags == 0, i


def test_another_geometry_clears_the_bit():
    """A geometry id beyond plane / standard: not plain, so not all spheres either."""
    from optiland_pr_amd import _abi

    t = _table(_optic(_rows()), 0.55)
    s = t.surfaces.copy()
    s["geometry"][0] = _abi.GEOM_EVEN_ASPHERE
    off = dataclasses.replace(t, surfaces=s)
    assert not off.frame_flags & _abi.LENS_PLAIN
    assert off.form_flags == 0


@pytest.mark.parametrize("case", NOT_PLAIN)
def test_cleared_whenever_plain_is(case):
    from optiland_pr_amd import _abi

    lens, wl, record = build(case)
    t = _table(lens, wl, record)
    if t.frame_flags & _abi.LENS_PLAIN:  # decentred: plain by the rule, all spheres too
        assert case == "decentred"
        assert not t.frame_flags & _abi.LENS_AXIAL  # which keeps it off the plain kernels
        return
    assert t.form_flags == 0


def test_header_and_python_agree():
    import os
    import re

    from optiland_pr_amd import _abi, _native

    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "optiland_rt.h")).read()
    assert re.search(r"ORT_LENS_SPHERES = 1u << (\d+)", text).group(1) == "0"
    assert _abi.LENS_SPHERES == 1 << 0
    assert re.search(r"uint32_t form_flags;", text)
    names = [f[0] for f in _native.ort_lens._fields_]
    assert names[-2:] == ["frame_flags", "form_flags"]
    import ctypes

    assert ctypes.sizeof(_native.ort_lens) == 112  # the struct did not grow
