"""ort_trace_ensemble on the MI355X: every variant's rays bit for bit those of ort_trace_pupil
on that variant alone, the per-(variant, pair) rms rows against the extended-precision
references and bounds of tests/_reductions.py, determinism, NaN containment, the refusal of
lenses outside its scope, MonteCarlo through it against the reference's fixture, and
torch.library.opcheck on torch.ops.ort.trace_ensemble.

Shapes: V in {1, 2, 3}, P in {1, 3}, n_pupil in {1, 7, 255, 256, 257, 513} (one lane, a
partial wave, the edges of the 256-ray chunk, three chunks with a one-ray tail)."""

import math

import numpy as np
import pytest

from tests import _reductions as R
from tests import _tolerancing as TT

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 3, 7), (3, 1, 255), (2, 1, 256), (3, 3, 257), (1, 3, 513)]
LENSES = ("cooke_axial", "cooke_tilted", "mirror")
WL = 0.55


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("needs the MI355X")
    import optiland_pr_amd.ops  # noqa: F401  (registers torch.ops.ort)

    R.WORST.clear()
    yield torch
    print("\nlargest error / bound on the device:\n" + R.report())


def mirror_lens():
    """A singlet of an absorbing glass (k > 0) behind a radial aperture, then a conic mirror."""
    from optiland_pr_amd import IdealMaterial, Optic
    from optiland_pr_amd.apertures import RadialAperture

    lens = Optic()
    lens.add_surface(index=0, radius=np.inf, thickness=np.inf)
    lens.add_surface(index=1, radius=60.0, thickness=4.0, material=IdealMaterial(1.5, 2e-5),
                     is_stop=True)
    lens.add_surface(index=2, radius=-200.0, thickness=30.0)
    lens.add_surface(index=3, radius=-80.0, conic=-0.7, thickness=-25.0, material="mirror")
    lens.add_surface(index=4)
    lens.set_aperture(aperture_type="EPD", value=10)
    lens.set_field_type(field_type="angle")
    lens.add_field(y=0)
    lens.add_field(y=2)
    lens.add_field(y=3)
    lens.add_wavelength(value=WL, is_primary=True)
    lens.surface_group.surfaces[1].aperture = RadialAperture(r_max=4.0)
    return lens


def tolerancing_of(kind):
    """A Tolerancing with the perturbations of the lens kind and three trials' values."""
    from optiland_pr_amd import tolerancing as T
    from optiland_pr_amd.samples import CookeTriplet

    S = T.ScalarSampler(0.0)
    if kind == "mirror":
        t = T.Tolerancing(mirror_lens())
        t.add_perturbation("radius", S, surface_number=3)
        t.add_perturbation("conic", S, surface_number=3)
        return t, [[-80.0, -0.7], [-80.4, -0.65], [-79.5, -0.8]]
    t = T.Tolerancing(CookeTriplet())
    t.add_perturbation("radius", S, surface_number=1)
    t.add_perturbation("thickness", S, surface_number=1)
    if kind == "cooke_axial":
        return t, [[22.01359, 3.25896], [22.06, 3.21], [21.97, 3.3]]
    t.add_perturbation("tilt", S, surface_number=3, axis="x")
    t.add_perturbation("decenter", S, surface_number=4, axis="y")
    # variant 0 untilted (no rotation ops in its block), 1 and 2 tilted and decentred
    return t, [[22.01359, 3.25896, None, None], [22.06, 3.21, 1.5e-3, 0.03],
               [21.97, 3.3, -2e-3, -0.02]]


def lowered(t, trials, pairs):
    out = []
    for values in trials:
        t.reset()
        for p, v in zip(t.perturbations, values, strict=True):
            if v is not None:
                p.set(v)
        out.append(t.lower_variant(pairs))
    t.reset()
    return out


def pupil(n):
    g = np.random.default_rng(1000 + n)
    r, a = 0.95 * np.sqrt(g.uniform(0, 1, n)), g.uniform(0, 2 * np.pi, n)
    return r * np.cos(a), r * np.sin(a)


def run_ensemble(torch, variants, P, px, py, want_rays=True):
    """-> stats [V][P][5], rays [8][V P n] (numpy), the workspace rows [V P chunks][4]."""
    from optiland_pr_amd import _calls, tolerancing as T
    from optiland_pr_amd.raytrace import get_device

    dev = get_device()
    ens = T.EnsembleTable([tb for tb, _ in variants])
    segs = np.stack([s for _, s in variants])
    lens, ft = ens.tensors(dev)
    pxd, pyd = (torch.from_numpy(v.copy()).to(dev) for v in (px, py))
    stats, rays, _ = T.trace_ensemble(lens, ens.meta(P), ft, T._bytes_tensor(segs).to(dev),
                                      None, pxd, pyd, want_rays)
    if rays is None:
        rays = torch.empty((8, 0), dtype=torch.float64)
    chunks = -(-px.size // 256)
    ws = _calls._WORKSPACES[("ensemble", dev)]
    rows = ws[:len(variants) * P * chunks * 32].view(torch.float64).reshape(-1, 4)
    return stats.cpu().numpy(), rays.cpu().numpy(), rows.cpu().numpy().copy()


def trace_alone(torch, table, segs, px, py):
    """ort_trace_pupil of one variant: rays [8][P n]."""
    from optiland_pr_amd import _abi, raytrace

    dev = raytrace.get_device()
    dl = raytrace.DeviceLens(table, dev)
    n_p, n = px.size, px.size * len(segs)
    out = raytrace.RealRays.empty(n, WL, device=dev)
    pxd, pyd = (torch.from_numpy(v.copy()).to(dev) for v in (px, py))
    raytrace.trace_pupil(dl, segs, pxd, pyd, out, n, n_p, n)
    return np.stack([getattr(out, a).cpu().numpy() for a in _abi.RAY_FIELDS])


def pairs_of(t, P):
    return [(hx, hy, WL) for hx, hy in t.optic.fields.get_field_coords()][:P]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("V,P,n", SHAPES)
@pytest.mark.parametrize("kind", LENSES)
def test_rays_are_trace_pupils_and_stats_meet_the_bounds(gpu, kind, V, P, n):
    torch = gpu
    t, trials = tolerancing_of(kind)
    variants = lowered(t, trials[:V], pairs_of(t, P))
    px, py = pupil(n)
    stats, rays, rows = run_ensemble(torch, variants, P, px, py)
    rays = rays.reshape(8, V, P * n)
    for v, (table, segs) in enumerate(variants):
        alone = trace_alone(torch, table, segs, px, py)
        nan = np.isnan(alone)
        assert np.array_equal(np.isnan(rays[:, v]), nan), (kind, v)
        assert np.array_equal(bits(rays[:, v])[~nan], bits(alone)[~nan]), (kind, v)
    if kind != "mirror":
        assert not np.isnan(rays).any()
    # the chunk rows against the rays, then the finish against the kernel's own rows
    chunks = -(-n // 256)
    x, y = rays[0].reshape(V * P, n), rays[1].reshape(V * P, n)
    rows = rows.reshape(V * P, chunks, 4)
    k = R.chain(256)
    for q in range(V * P):
        if np.isnan(x[q]).any() or np.isnan(y[q]).any():  # a clipped pair keeps its rays;
            assert math.isnan(stats.reshape(-1, 5)[q, 3])  # only a missed ray is NaN
            continue
        for c in range(chunks):
            sl = slice(c * 256, min(n, (c + 1) * 256))
            r = R.spot_reference(x[q, sl][None], y[q, sl][None], None, 1, 1, 0, k)[0]
            assert rows[q, c, 0] == r.n
            R.check("ensemble row sum", rows[q, c, 1], r.sx, r.b_sx)
            R.check("ensemble row sum", rows[q, c, 2], r.sy, r.b_sy)
            R.check("ensemble row M2", rows[q, c, 3], r.s2, r.b_s2)
        R.check_finish("ensemble finish", stats.reshape(-1, 5)[q], R.finish_reference(rows[q]))
    # without rays_out: the same stats bits; a second run: the same bits
    stats2, rays2, _ = run_ensemble(torch, variants, P, px, py, want_rays=False)
    assert rays2.shape == (8, 0)
    assert np.array_equal(bits(stats2[..., :4]), bits(stats[..., :4]))
    stats3, rays3, _ = run_ensemble(torch, variants, P, px, py)
    assert np.array_equal(bits(stats3[..., :4]), bits(stats[..., :4]))
    assert np.array_equal(np.isnan(rays3), np.isnan(rays.reshape(8, -1)))
    assert np.array_equal(bits(np.nan_to_num(rays3)), bits(np.nan_to_num(rays.reshape(8, -1))))
    assert np.isnan(stats[..., 4]).all()


def test_a_missing_variant_is_nan_alone(gpu):
    """Surface 1 at R = 5.2 mm under a 10 mm entrance pupil: the marginal rays miss the
    sphere (checked on the host build: NaN in every pair of that variant -- some of the
    on-axis pair's rays, not all -- and none elsewhere)."""
    import torch as _t

    from optiland_pr_amd import host
    from optiland_pr_amd import tolerancing as T

    torch = gpu
    t, _ = tolerancing_of("cooke_axial")
    # radii only: a thickness set and reset moves the vertices by rounding (the reference's
    # set_thickness arithmetic), which would make variant 2 depend on variant 1's history
    good = lowered(t, [[22.01359, None], [22.06, None], [21.97, None]], pairs_of(t, 3))
    bad = lowered(t, [[22.01359, None], [5.2, None], [21.97, None]], pairs_of(t, 3))
    for v in (0, 2):
        assert good[v][0].fingerprint() == bad[v][0].fingerprint()
        assert good[v][1].tobytes() == bad[v][1].tobytes()
    px, py = T._pupil_points("hexapolar", 6)
    for v, (table, segs) in enumerate(bad):
        outs, _ = host.trace_pupil(host.HostLens(table), T._bytes_tensor(segs),
                                   _t.from_numpy(px), _t.from_numpy(py), 3 * px.size, px.size,
                                   False)
        miss = np.isnan(outs[0].numpy()).reshape(3, -1)
        assert (miss.any(axis=1).all() and not miss[0].all()) if v == 1 else not miss.any()
    s_good, _, _ = run_ensemble(torch, good, 3, px, py)
    s_bad, r_bad, _ = run_ensemble(torch, bad, 3, px, py)
    assert np.isnan(s_bad[1, :, 3]).all() and np.isnan(s_bad[1, :, 1]).all()
    assert np.all(s_bad[1, :, 0] == px.size)  # every ray counts
    for v in (0, 2):
        assert np.array_equal(bits(s_bad[v, :, :4]), bits(s_good[v, :, :4]))
        assert not np.isnan(r_bad.reshape(8, 3, -1)[:, v]).any()


def test_unsupported_lenses_are_refused_and_fall_back(gpu):
    from optiland_pr_amd import _abi
    from optiland_pr_amd import tolerancing as T
    from optiland_pr_amd.raytrace import get_device
    from optiland_pr_amd.samples import ReverseTelephotoAsphere

    torch = gpu
    dev = get_device()
    t, trials = tolerancing_of("cooke_axial")
    variants = lowered(t, trials[:1], pairs_of(t, 1))
    ens = T.EnsembleTable([variants[0][0]])
    lens, ft = ens.tensors(dev)
    px, py = (torch.from_numpy(v.copy()).to(dev) for v in pupil(7))
    seg = T._bytes_tensor(np.stack([variants[0][1]])).to(dev)
    meta = ens.meta(1)
    for field, value in ((4, meta[4] | 1 << _abi.GEOM_EVEN_ASPHERE),
                         (5, meta[5] | 1 << _abi.IA_THIN_LENS)):
        refused = list(meta)
        refused[field] = value
        with pytest.raises(RuntimeError, match="ort_trace_ensemble failed: ORT_ERR_ARG"):
            T.trace_ensemble(lens, refused, ft, seg, None, px, py)
    # an even-asphere lens through MonteCarlo: the per-trial loop's values
    cols = {}
    for batched in (True, False):
        lens_a = ReverseTelephotoAsphere()
        ta = T.Tolerancing(lens_a)
        ta.add_operand("rms_spot_size", {"optic": lens_a, "surface_number": -1, "Hx": 0.0,
                                         "Hy": 0.7, "num_rays": 3, "wavelength": 0.55,
                                         "distribution": "hexapolar"})
        r1 = float(lens_a.surface_group.radii[1])
        ta.add_perturbation("radius", T.DistributionSampler("normal", seed=1, loc=r1,
                                                            scale=1e-3 * abs(r1)),
                            surface_number=1)
        mc = T.MonteCarlo(ta)
        mc.run(3, batched=batched)
        assert ta.timing["mode"] == "loop"
        cols[batched] = mc.results
    assert list(cols[True]) == list(cols[False])
    for c in cols[True]:
        assert np.all(np.isfinite(cols[True][c]))
        assert cols[True][c].tobytes() == cols[False][c].tobytes(), c


def test_monte_carlo_case_a_on_the_device(gpu):
    from optiland_pr_amd import tolerancing as T

    golden = TT.fixture()
    cols = [str(c) for c in golden["A/columns"]]
    t = TT.case_a()
    mc = T.MonteCarlo(t)
    mc.run(TT.TRIALS, batched=True)
    assert t.timing["mode"] == "ensemble"
    assert list(mc.results) == cols
    for c in cols[:5]:
        assert mc.results[c].tobytes() == golden[f"A/{c}"].tobytes(), c
    trials = [[golden[f"A/{c}"][i] for c in cols[:5]] for i in range(TT.TRIALS)]
    got = np.stack([mc.results[c] for c in cols[5:]], axis=1)
    want = np.stack([golden[f"A/{c}"] for c in cols[5:]], axis=1)
    worst = TT.check_against_fixture("A ensemble", t, trials, got, want, TT.K_ENSEMBLE)
    print("worst error / bound, case A through the ensemble launch:", worst)


def test_opcheck(gpu):
    from optiland_pr_amd import tolerancing as T
    from optiland_pr_amd.raytrace import get_device

    torch = gpu
    dev = get_device()
    t, trials = tolerancing_of("cooke_tilted")
    variants = lowered(t, trials[:2], pairs_of(t, 3))
    ens = T.EnsembleTable([tb for tb, _ in variants])
    lens, ft = ens.tensors(dev)
    px, py = (torch.from_numpy(v.copy()).to(dev) for v in pupil(7))
    seg = T._bytes_tensor(np.stack([s for _, s in variants])).to(dev)
    ref, ref_rays, _ = T.trace_ensemble(lens, ens.meta(3), ft, seg, None, px, py, True)
    for want_rays in (False, True):
        stats, rays = torch.ops.ort.trace_ensemble(lens, ens.meta(3), ft, seg, None, px, py,
                                                   want_rays)
        assert stats.shape == (2, 3, 4) and torch.equal(stats, ref[..., :4])
        assert torch.equal(rays, ref_rays) if want_rays else rays.shape == (8, 0)
        res = torch.library.opcheck(torch.ops.ort.trace_ensemble.default,
                                    (lens, ens.meta(3), ft, seg, None, px, py, want_rays))
        assert all(v == "SUCCESS" for v in res.values()), res
