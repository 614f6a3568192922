"""The closed-form kernel's fast pass with its reciprocals seeded from the square roots
beside them (ort_fastpath.h: sqrt_untested_h + shared_div_ge1_seeded for the conic normal's
magnitude, sqrt_h + shared_div_seeded for the generated ray's norm), against
ORT_OPT_EXACT -- the same kernel with every lane sent through its exact re-trace, whose
divisions are ort_core.h's own v_rcp-based sequences -- and against the NumPy oracle.

Default launch vs ORT_OPT_EXACT: the same bits in all eight outputs, NaN payloads and
signed zeros included. Against the oracle (at most 4,099 rays of a case): the same NaN
masks, values and zero signs; the intensity to rtol 1e-12, as everywhere in the suite.

Not checked here: the share of lanes that take the exact re-trace. The closed-form kernel
has no hook that reports its `bad` lanes (ORT_FAST_PROBE is the Newton kernel's), so a fast
pass that flagged every lane would pass these comparisons; profiles/r08_closed_seeds.md sets
the default launch's kernel time beside the exact launch's instead.
"""
import numpy as np
import pytest

from tests._closed import (CONIC, MIRROR, N_ORACLE, TRIPLET, optic, pupils_fixture, same_as_oracle,
                           same_bits)
from tests._closed import torch  # noqa: F401

pytestmark = pytest.mark.gpu

# ---- generated rays (F_GEN, the benchmark's kernel) ------------------------------------

# three seeds of 2^18 random pupil points, the uniform 128 grid, and the uniform 129 grid,
# whose centre column and row are +0
pupils = pupils_fixture(1 << 18, seeds=(1, 2, 3), grids=(128, 129))


@pytest.mark.parametrize("hy", [0.0, 0.7, 1.0])
@pytest.mark.parametrize("lens_name", ["DoubleGauss", "CookeTriplet", "ReverseTelephoto"])
def test_generated_rays_fast_equals_exact_and_oracle(torch, pupils, lens_name, hy):
    from oracle import trace_np
    from optiland_pr_amd import samples
    from optiland_pr_amd.lowering import segment_params
    from optiland_pr_amd.raytrace import RealRays, lens_for, trace_pupil

    lens = getattr(samples, lens_name)()
    wl = 0.55 if lens_name == "CookeTriplet" else 0.5876
    dl = lens_for(lens, [wl])
    seg = np.stack([segment_params(lens, 0.0, hy, 0)])
    for name, (px, py) in pupils.items():
        n = px.size
        pxd, pyd = torch.as_tensor(px, device="cuda"), torch.as_tensor(py, device="cuda")
        outs = {}
        for exact in (False, True):
            out = RealRays.empty(n, wl)
            trace_pupil(dl, seg, pxd, pyd, out, n, n, n, exact_only=exact)
            torch.cuda.synchronize()
            outs[exact] = out.numpy()
        what = f"{lens_name} hy={hy} {name}"
        same_bits(outs[False], outs[True], what)
        sel = np.arange(N_ORACLE) * (n // N_ORACLE)
        with np.errstate(all="ignore"):
            ref = trace_np.trace_segment(
                dl.table, trace_np.generate_rays(seg[0], px[sel], py[sel]), 0).rays
        same_as_oracle(outs[False], ref, what, sel)
        assert np.isfinite(outs[False]["x"]).mean() > 0.5  # the case traces real rays


# ---- caller rays (ort_trace_sequential) ------------------------------------------------

def _optic(rows, scale=1.0):
    """A centred lens from add_surface rows; radii and thicknesses times scale, the
    entrance pupil diameter 10 at every scale (caller rays: no pupil)."""
    return optic(rows, scale, scale_epd=False)


# unit radii: scaled by s, the front radius is s itself
_SINGLET = [
    dict(radius=np.inf, thickness=np.inf),
    dict(radius=1.0, thickness=0.25, material="SK16"),
    dict(radius=-1.0, thickness=2.0),
    dict(),
]


def _random_rays(n, length, seed):
    """n rays over a disc of radius 0.12 `length`, starting 0.5 `length` in front of the
    first vertex, direction cosines up to 0.05 off the axis, normalised by NumPy."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.12, 0.12, n) * length
    y = rng.uniform(-0.12, 0.12, n) * length
    z = np.full(n, -0.5 * length)
    L = rng.uniform(-0.05, 0.05, n)
    M = rng.uniform(-0.05, 0.05, n)
    return x, y, z, L, M, np.sqrt(1.0 - L * L - M * M)


def _check_caller_rays(torch, lens, cols, what, wl=0.55, min_finite=0.5):
    from oracle import trace_np
    from optiland_pr_amd.raytrace import RealRays, lens_for, trace_rays

    dl = lens_for(lens, [wl])
    x, y, z, L, M, N = (np.ascontiguousarray(c, dtype=np.float64) for c in cols)
    n = x.size
    outs = {}
    for exact in (False, True):
        rin = RealRays(x, y, z, L, M, N, 1.0, wl)
        rout = RealRays.empty(n, wl)
        trace_rays(dl, rin, rout, exact_only=exact)
        torch.cuda.synchronize()
        outs[exact] = rout.numpy()
    same_bits(outs[False], outs[True], what)
    with np.errstate(all="ignore"):
        ref = trace_np.trace_segment(
            dl.table, trace_np.Rays(x.copy(), y.copy(), z.copy(), L.copy(), M.copy(), N.copy(),
                                    np.ones(n)), 0).rays
    same_as_oracle(outs[False], ref, what)
    assert np.isfinite(outs[False]["x"]).mean() >= min_finite, what
    return outs[False]


LENSES = {
    "conic": (CONIC, 1.0),
    "mirror": (MIRROR, 1.0),
    "scaled_up": (TRIPLET, 2.0**140),
    "scaled_down": (TRIPLET, 2.0**-140),
}


@pytest.mark.parametrize("case", sorted(LENSES))
def test_conic_mirror_and_scaled_lenses(torch, case):
    """k != 0, a reflective sphere, and every length times 2^+-140: the normal's magnitude
    is seeded on each."""
    rows, scale = LENSES[case]
    _check_caller_rays(torch, _optic(rows, scale), _random_rays(N_ORACLE, 20.0 * scale, 11),
                       case)


@pytest.mark.parametrize("factor", [1.0 + 2.0**-31, 1.0 + 2.0**-29, 0.5, 3.0])
def test_scaled_directions(torch, factor):
    """Directions times `factor` (L^2 + M^2 + N^2 off 1 by 2^-30, 2^-28, or far off): the
    seeded magnitude meets normals of rays the reference traces unnormalised. All stay on
    the fast pass here; which pass a lane took cannot be observed, only its bits."""
    x, y, z, L, M, N = _random_rays(N_ORACLE, 20.0, 12)
    _check_caller_rays(torch, _optic(TRIPLET), (x, y, z, L * factor, M * factor, N * factor),
                       f"directions x {factor!r}")


@pytest.mark.parametrize("radius", [2.0**150, 2.0**150 * (1 + 2.0**-52), 2.0**-150,
                                    2.0**-150 * (1 - 2.0**-53)],
                         ids=["2^150", "above_2^150", "2^-150", "below_2^-150"])
def test_radius_range_ends(torch, radius):
    """|R| at both ends of 2^-150 <= |R| <= 2^150, the range in which the host sets
    ORT_SURF_INV_R2 and the surface takes normal_conic_rcp with its seeded magnitude, and
    one ulp beyond each (R^2 leaves [2^-300, 2^300]: normal_conic, unchanged code)."""
    _check_caller_rays(torch, _optic(_SINGLET, radius), _random_rays(N_ORACLE, radius, 13),
                       f"R = {radius!r}")


def test_vertex_and_rim_hits(torch):
    """Hits at the vertex (1 - q = 1, mag = 1: g = 1 and h = 1/2 are exact, the seeds
    exact reciprocals) and near the rim of the front sphere, 1 - q from 2^-10 down to 2^-40
    (steep normals; most of these rays miss a later surface or are totally reflected, and
    NaNs compare too)."""
    R = 22.01359
    rows = []
    for zero in (0.0, -0.0):  # on the axis, through the vertex
        rows.append((zero, zero, -10.0, 0.0, 0.0, 1.0))
        rows.append((0.0, zero, -10.0, zero, 0.0, 1.0))
    for L, M in ((0.05, -0.03), (-0.02, 0.0), (0.0, 0.04)):  # aimed at the vertex
        N = np.sqrt(1.0 - L * L - M * M)
        t = 10.0 / N
        rows.append((-t * L, -t * M, -10.0, L, M, N))
    for j in (10, 20, 30, 36, 40):  # parallel to the axis at r = R sqrt(1 - 2^-j)
        r = R * np.sqrt(1.0 - 2.0**-j)
        for h in (r, np.nextafter(r, 0.0), np.nextafter(r, np.inf)):
            for cx, cy in ((1.0, 0.0), (0.0, -1.0), (0.6, 0.8)):
                rows.append((h * cx, h * cy, -10.0, 0.0, 0.0, 1.0))
    cols = [np.array(c, dtype=np.float64) for c in zip(*rows)]
    got = _check_caller_rays(torch, _optic(TRIPLET), cols, "vertex and rim", min_finite=0.0)
    # vertex rays trace through (not all: the oracle, too, gives NaN for some zero patterns)
    assert np.isfinite(got["x"][:11]).any()
