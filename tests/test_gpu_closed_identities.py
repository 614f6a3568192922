"""The closed-form kernel's fast pass after its exact identities (ort_fastpath.h
distance_conic_folded: powers of two folded out of the quadratic, x x - 2R z for
(0 - 2R z) + x x; ort_kernels.h closed_surfaces: x + 0.0 / y + 0.0 only at the first traced
surface, the range failures carried as a wave mask) against ORT_OPT_EXACT -- the same
kernel with every lane sent through its exact re-trace (trace_closed_kernel ORs
KArgs.exact_only into the lane's `bad`), so every stored value comes from ort_core.h's
per-operation sequences -- and against the oracle.

Every case is 100 rays: two waves, the second one partial. Default launch vs ORT_OPT_EXACT:
the same bits in every output, NaN payloads and signed zeros included. Against the oracle:
the same NaN masks, values and zero signs; the intensity to rtol 1e-12, as everywhere in the
suite (the device's exp is not NumPy's).
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "z", "L", "M", "N", "i", "opd")
N_RAYS = 100  # 64 + 36


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need the MI355X (torch.cuda.is_available() is False)")
    from optiland_pr_amd import _native

    _native.load()
    return t


def _optic(rows, scale=1.0):
    """A centred lens from add_surface rows; radii and thicknesses times scale."""
    from optiland_pr_amd.optic import Optic

    lens = Optic()
    for i, row in enumerate(rows):
        kw = dict(row)
        for key in ("radius", "thickness"):
            if key in kw and np.isfinite(kw[key]):
                kw[key] = kw[key] * scale
        lens.add_surface(index=i, **kw)
    lens.set_aperture(aperture_type="EPD", value=10)
    lens.set_field_type(field_type="angle")
    lens.add_field(y=0)
    lens.add_wavelength(value=0.55, is_primary=True)
    return lens


_TRIPLET = [
    dict(radius=np.inf, thickness=np.inf),
    dict(radius=22.01359, thickness=3.25896, material="SK16"),
    dict(radius=-435.76044, thickness=6.00755),
    dict(radius=-22.21328, thickness=0.99997, material=("F2", "schott")),
    dict(radius=20.29192, thickness=4.75041, is_stop=True),
    dict(radius=79.68360, thickness=2.95208, material="SK16"),
    dict(radius=-18.39533, thickness=42.20778),
    dict(),
]
_CONIC = [dict(r) for r in _TRIPLET]
_CONIC[1]["conic"] = -0.6
_CONIC[4]["conic"] = 0.8
_CONIC[6]["conic"] = 1.2
_MIRROR = [
    dict(radius=np.inf, thickness=np.inf),
    dict(radius=40.0, thickness=5.0, material="SK16"),
    dict(radius=np.inf, thickness=30.0),
    dict(radius=-120.0, thickness=-25.0, material="mirror"),
    dict(),
]

# name -> (lens factory, wavelength, first traced surface, scale of every length).
# The lowered table starts at the first surface behind the object: 0 is the front sphere;
# DoubleGauss 3 and the mirror lens's 1 are planes, CookeTriplet 6 is the image plane.
CASES = {
    "dg_sphere_first": (lambda: _sample("DoubleGauss"), 0.5876, 0, 1.0),
    "dg_plane_first": (lambda: _sample("DoubleGauss"), 0.5876, 3, 1.0),
    "cooke_sphere_first": (lambda: _sample("CookeTriplet"), 0.55, 0, 1.0),
    "cooke_plane_first": (lambda: _sample("CookeTriplet"), 0.55, 6, 1.0),
    "conic": (lambda: _optic(_CONIC), 0.55, 0, 1.0),
    "conic_from_second": (lambda: _optic(_CONIC), 0.55, 1, 1.0),
    "mirror": (lambda: _optic(_MIRROR), 0.55, 0, 1.0),
    "mirror_plane_first": (lambda: _optic(_MIRROR), 0.55, 1, 1.0),
    "scaled_up": (lambda: _optic(_TRIPLET, 2.0**140), 0.55, 0, 2.0**140),
    "scaled_down": (lambda: _optic(_TRIPLET, 2.0**-140), 0.55, 0, 2.0**-140),
}


def _sample(name):
    from optiland_pr_amd import samples

    return getattr(samples, name)()


def _rays(scale):
    """5 x 5 positions (both zeros, tiny, moderate) x 4 directions (on the axis with +0
    and with -0 cosines, two tilted), starting 10 in front of the first vertex."""
    pos = [0.0, -0.0, 1.5, -2.25, 1e-3]
    dirs = [(0.0, 0.0), (-0.0, -0.0), (0.05, -0.03), (-0.02, 0.0)]
    rows = []
    for x, y, (L, M) in itertools.product(pos, pos, dirs):
        rows.append((x * scale, y * scale, -10.0 * scale, L, M, np.sqrt(1.0 - L * L - M * M)))
    cols = [np.array(c, dtype=np.float64) for c in zip(*rows)]
    assert cols[0].size == N_RAYS
    return cols


def _same_bits(got, exp, what):
    for a in FIELDS:
        g, e = np.asarray(got[a]), np.asarray(exp[a])
        np.testing.assert_array_equal(g.view(np.uint64), e.view(np.uint64), err_msg=f"{what} {a}")


def _same_as_oracle(got, ref, what):
    for a in FIELDS:
        g, r = np.asarray(got[a]), np.asarray(getattr(ref, a))
        np.testing.assert_array_equal(np.isnan(g), np.isnan(r), err_msg=f"{what} {a} NaN")
        ok = ~np.isnan(r)
        if a == "i":
            with np.errstate(all="ignore"):
                np.testing.assert_allclose(g[ok], r[ok], rtol=1e-12, atol=0)
            continue
        np.testing.assert_array_equal(g[ok], r[ok], err_msg=f"{what} {a}")
        np.testing.assert_array_equal(np.signbit(g[ok]), np.signbit(r[ok]),
                                      err_msg=f"{what} sign of {a}")


@pytest.mark.parametrize("case", sorted(CASES))
def test_caller_rays_fast_equals_exact_and_oracle(torch, case):
    """The caller-supplied-ray path (no F_GEN): rays entering with x, y = +0 / -0, on the
    axis, through a first traced surface that is a plane or a sphere, conics with k != 0, a
    reflective sphere, and a lens with every length (and the rays) scaled by 2^+-140."""
    from oracle import trace_np
    from optiland_pr_amd.raytrace import RealRays, lens_for, trace_rays

    make, wl, start, scale = CASES[case]
    dl = lens_for(make(), [wl])
    x, y, z, L, M, N = _rays(scale)
    outs = {}
    for exact in (False, True):
        rin = RealRays(x, y, z, L, M, N, 1.0, wl)
        rout = RealRays.empty(N_RAYS, wl)
        trace_rays(dl, rin, rout, start_surface=start, exact_only=exact)
        torch.cuda.synchronize()
        outs[exact] = rout.numpy()
    _same_bits(outs[False], outs[True], case)
    with np.errstate(all="ignore"):
        ref = trace_np.trace_segment(
            dl.table, trace_np.Rays(x.copy(), y.copy(), z.copy(), L.copy(), M.copy(), N.copy(),
                                    np.ones(N_RAYS)), 0, start=start).rays
    _same_as_oracle(outs[False], ref, case)
    assert np.isfinite(outs[False]["x"]).sum() > N_RAYS // 2  # the case traces real rays


@pytest.mark.parametrize("lens_name", ["CookeTriplet", "DoubleGauss"])
def test_generated_rays_fast_equals_exact_and_oracle(torch, lens_name):
    """The F_GEN path (the benchmark's kernel): a 10 x 10 pupil whose samples include +0
    and -0 in both coordinates, on the axis and at full field."""
    from oracle import trace_np
    from optiland_pr_amd.lowering import segment_params
    from optiland_pr_amd.raytrace import RealRays, lens_for, trace_pupil

    lens = _sample(lens_name)
    wl = 0.55 if lens_name == "CookeTriplet" else 0.5876
    dl = lens_for(lens, [wl])
    g = np.array([0.0, -0.0, 0.3, -0.3, 0.6, -0.6, 0.85, -0.85, 1e-3, -1e-3])
    px, py = (c.reshape(-1).copy() for c in np.meshgrid(g, g))
    assert px.size == N_RAYS
    for hx, hy in ((0.0, 0.0), (0.0, 1.0)):
        seg = np.stack([segment_params(lens, hx, hy, 0)])
        outs = {}
        for exact in (False, True):
            out = RealRays.empty(N_RAYS, wl)
            trace_pupil(dl, seg, torch.as_tensor(px, device="cuda"),
                        torch.as_tensor(py, device="cuda"), out, N_RAYS, N_RAYS, N_RAYS,
                        exact_only=exact)
            torch.cuda.synchronize()
            outs[exact] = out.numpy()
        what = f"{lens_name} ({hx},{hy})"
        _same_bits(outs[False], outs[True], what)
        with np.errstate(all="ignore"):
            ref = trace_np.trace_segment(dl.table, trace_np.generate_rays(seg[0], px, py), 0).rays
        _same_as_oracle(outs[False], ref, what)
