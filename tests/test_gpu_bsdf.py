"""BSDF surface scattering on the MI355X (trace_kernel<F_SCAT> and bsdf_scatter_kernel,
csrc/ort_k_trace_scat.hip): both goldens of tests/golden/bsdf.npz, launch-shape and
split-batch identities of the counter-based random stream, a Newton surface under the verify
re-trace, the non-BSDF records against the plain kernels, one moment check and
IncoherentIrradiance. Tolerances: tests/_bsdf.py."""

import types

import numpy as np
import pytest
import torch

from optiland_pr_amd import _abi, materials, optic, raytrace, scatter
from optiland_pr_amd.apertures import RectangularAperture
from optiland_pr_amd.irradiance import IncoherentIrradiance
from tests import _bsdf as B

pytestmark = pytest.mark.gpu


def _dev():
    return raytrace.get_device()


@pytest.mark.parametrize("name", list(B.cases.STEP_CASES))
def test_device_step_against_reference(name):
    B.check_step_case(name, _dev())


def _golden_trace(lens=None):
    if lens is None:
        lens = B.lens_and_inputs()[0]
    g = B.fixture()
    d = types.SimpleNamespace(x=g["lens/px"], y=g["lens/py"])
    return lens, lens.trace(*B.cases.LENS_FIELD, B.cases.LENS_WAVELENGTH, None, d)


def test_device_lens_against_reference():
    lens, rays = _golden_trace()
    assert rays.x.is_cuda
    B.check_lens_rays([getattr(rays, a) for a in _abi.RAY_FIELDS])
    # trace_generic (one segment per ray) is the same trace
    g = B.fixture()
    n = len(g["lens/px"])
    hx, hy = B.cases.LENS_FIELD
    gen = lens.trace_generic(np.full(n, hx), np.full(n, hy), g["lens/px"], g["lens/py"],
                             B.cases.LENS_WAVELENGTH)
    for a in _abi.RAY_FIELDS:
        assert torch.equal(getattr(gen, a), getattr(rays, a)), a


def _trace_n(lens, dlens, segs, px, py, ray_offset=0):
    n = len(px)
    out = raytrace.RealRays.empty(n, B.cases.LENS_WAVELENGTH, device=dlens.device)
    raytrace.trace_pupil(dlens, segs, torch.as_tensor(px.copy(), device=dlens.device),
                         torch.as_tensor(py.copy(), device=dlens.device), out, n, max(n, 1),
                         max(n, 1), ray_offset=ray_offset)
    return [getattr(out, a) for a in _abi.RAY_FIELDS]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_batch_sizes_run_to_run_and_split(n):
    lens, segs, px, py = B.lens_and_inputs()
    px, py = px[:n], py[:n]
    dlens = raytrace.lens_for(lens, [B.cases.LENS_WAVELENGTH])
    a = _trace_n(lens, dlens, segs, px, py)
    b = _trace_n(lens, dlens, segs, px, py)
    for x, y in zip(a, b, strict=True):
        assert torch.equal(x, y)
    g = B.fixture()  # the first n rays of the golden trace: ray r draws as ray r
    for f, x in zip(_abi.RAY_FIELDS, a, strict=True):
        tol = B.TOL_DIR if f in ("L", "M", "N", "i") else B.TOL_POS
        assert np.max(np.abs(x.cpu().numpy() - g[f"lens/{f}"][:n])) <= tol
    for split in (64, 100):
        if split >= n:
            continue
        lo = _trace_n(lens, dlens, segs, px[:split], py[:split])
        hi = _trace_n(lens, dlens, segs, px[split:], py[split:], ray_offset=split)
        for w, p, q in zip(a, lo, hi, strict=True):
            assert torch.equal(w, torch.cat([p, q]))


def _asphere_lens():
    lens = optic.Optic()
    lens.add_surface(index=0, radius=np.inf, thickness=np.inf)
    lens.add_surface(index=1, surface_type="even_asphere", radius=40.0, conic=0.0,
                     coefficients=[1e-4, -2e-6, 1e-8], thickness=5.0,
                     material=materials.IdealMaterial(n=1.5), is_stop=True,
                     bsdf=scatter.GaussianBSDF(0.02))
    lens.add_surface(index=2, radius=-60.0, thickness=30.0)
    lens.add_surface(index=3)
    lens.set_aperture(aperture_type="EPD", value=12.0)
    lens.set_field_type(field_type="angle")
    lens.add_field(y=0.0)
    lens.add_field(y=4.0)
    lens.add_wavelength(value=0.55, is_primary=True)
    lens.scatter_seed = 11
    return lens


def test_newton_surface_verify_retrace_draws_the_same_numbers():
    lens = _asphere_lens()
    dlens = raytrace.lens_for(lens, [0.55])
    assert dlens.newton and dlens.table.has_bsdf
    first = lens.trace(0.0, 1.0, 0.55, 6, "hexapolar")
    settled = np.array(dlens.last_schedule)
    # a schedule two updates too long on the Newton surface: the verify step finds the
    # earlier stop index, corrects the schedule and traces again
    wrong = settled[0].copy()
    for s in dlens.newton:
        wrong[s] += 2
    dlens.sched_cache.clear()
    dlens.sched_cache["_default"] = wrong
    again = lens.trace(0.0, 1.0, 0.55, 6, "hexapolar")
    assert np.array_equal(np.array(dlens.last_schedule), settled)  # re-traced on `settled`
    assert not np.array_equal(wrong, settled[0])
    third = lens.trace(0.0, 1.0, 0.55, 6, "hexapolar")  # the corrected schedule up front
    for a in _abi.RAY_FIELDS:
        assert torch.equal(getattr(third, a), getattr(again, a)), a
    for a in _abi.RAY_FIELDS:
        x, y = getattr(first, a), getattr(again, a)
        assert torch.equal(x, y), a
    assert not torch.isnan(first.L).any()


def _plain(lens):
    for s in lens.surface_group.surfaces:
        s.interaction_model.bsdf = None
    return lens


def test_non_bsdf_surface_records_are_the_plain_kernels():
    lens = B.lens_and_inputs()[0]
    lens.surface_group.record = "all"
    _golden_trace(lens)
    sg = lens.surface_group
    got = [[getattr(s, a).clone() for a in ("x", "y", "z", "L", "M", "N", "intensity", "opd")]
           for s in sg.surfaces]
    plain = _plain(B.lens_and_inputs()[0])
    plain.surface_group.record = "all"
    _golden_trace(plain)
    ref = [[getattr(s, a) for a in ("x", "y", "z", "L", "M", "N", "intensity", "opd")]
           for s in plain.surface_group.surfaces]
    for k in (0, 1):  # the object surface and surface 1: before any BSDF
        for x, y in zip(got[k], ref[k], strict=True):
            assert torch.equal(x, y)
    for f in (0, 1, 2, 6, 7):  # surface 2 scatters: hit point, intensity and opd do not move
        assert torch.equal(got[2][f], ref[2][f])
    assert not torch.equal(got[2][3], ref[2][3])
    # an Optic without BSDFs takes the plain kernels, a BSDF Optic the F_SCAT family
    assert not raytrace.lens_for(plain, [B.cases.LENS_WAVELENGTH]).table.has_bsdf


def test_all_none_table_on_the_scatter_kernels_is_the_plain_trace():
    """trace_kernel<F_SCAT> on a table without BSDFs against the closed-form kernels."""
    import ctypes as C

    from optiland_pr_amd import _calls, _native
    from optiland_pr_amd._calls import addr

    lens, segs, px, py = B.lens_and_inputs()
    plain = _plain(lens)
    dlens = raytrace.lens_for(plain, [B.cases.LENS_WAVELENGTH])
    ref = _trace_n(plain, dlens, segs, px, py)
    n = len(px)
    dev = dlens.device
    outs = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(8)]
    scat, keep = scatter.scatter_struct(dlens)
    seg_dev = raytrace.upload_segments(segs, dev)
    batch = _calls.pupil_batch(n, n, n, seg_dev, False, dlens.apod)
    opt = _native.ort_options(_abi.NEWTON_SCHEDULE, 0, None)
    out_c = _calls.rays_struct(outs)
    pxt, pyt = torch.as_tensor(px.copy(), device=dev), torch.as_tensor(py.copy(), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _native.load().ort_trace_pupil_scatter(
        C.byref(dlens.c), addr(pxt), addr(pyt), C.byref(out_c), C.byref(batch), C.byref(opt),
        None, None, addr(status), C.byref(scat), raytrace._stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    for a, b in zip(ref, outs, strict=True):
        assert torch.equal(a, b)
    del keep


def test_lambertian_moments_at_normal_incidence():
    """65,536 rays along the normal of a Lambertian plane: (L, M) is the disk point, so
    r^2 = L^2 + M^2 is uniform on (0, 1]: mean 1/2, variance 1/12. The mean of n samples
    lies within 6 standard errors, 6 / sqrt(12 n), of 1/2."""
    n = 65536
    dev = _dev()
    zero = torch.zeros(n, dtype=torch.float64, device=dev)
    one = torch.ones(n, dtype=torch.float64, device=dev)
    L, M, N = scatter.bsdf_scatter(zero, zero, one, zero, zero, one, scatter.LambertianBSDF(),
                                   seed=2024, surface_index=1)
    r2 = (L * L + M * M).cpu().numpy()
    mean, var = float(r2.mean()), float(r2.var())
    print("mean", mean, "variance", var)
    assert abs(mean - 0.5) <= 6.0 / np.sqrt(12.0 * n)
    # the sample variance of a uniform: standard error sqrt((1/80 - 1/144) / n), 6 of them
    assert abs(var - 1.0 / 12.0) <= 6.0 * np.sqrt((1.0 / 80.0 - 1.0 / 144.0) / n)
    assert torch.all(N >= 0) and float((L * L + M * M + N * N - 1).abs().max()) < 1e-14


def test_incoherent_irradiance_conserves_the_landed_power():
    lens = B.lens_and_inputs()[0]
    lens.surface_group.surfaces[-1].aperture = RectangularAperture(-6.0, 6.0, -6.0, 6.0)
    g = B.fixture()
    d = types.SimpleNamespace(x=g["lens/px"], y=g["lens/py"])
    irr = IncoherentIrradiance(lens, num_rays=None, res=(32, 32), fields=[B.cases.LENS_FIELD],
                               wavelengths=[B.cases.LENS_WAVELENGTH], distribution=d)
    img, xe, ye = irr.data[0][0]
    area = (xe[1] - xe[0]) * (ye[1] - ye[0])
    rays = lens.trace(*B.cases.LENS_FIELD, B.cases.LENS_WAVELENGTH, None, d)
    x, y, i = (getattr(rays, a).cpu().numpy() for a in ("x", "y", "i"))
    landed = (x >= -6) & (x <= 6) & (y >= -6) & (y <= 6)
    assert 0 < landed.sum() < len(x)  # the Lambertian mirror sends some rays past the detector
    total = float(img.sum().item()) * area
    print("binned power", total, "landed power", float(i[landed].sum()))
    # tests/_irradiance.py's bound summed over the pixels: n roundings to the fixed-point
    # quantum (2^-53 or finer for n = 257 contributions of at most 1; 2^-52 taken) and the
    # fp64 sums on either side, plus the division and multiplication by the pixel area
    n, s = len(x), float(np.abs(i[landed]).sum())
    assert abs(total - float(i[landed].sum())) <= n * 2.0 ** -52 + (n + 4) * 2.0 ** -53 * s


def test_attempt_cap_raises_naming_surface_and_sigma():
    lens = B.lens_and_inputs()[0]
    lens.surface_group.surfaces[2].interaction_model.bsdf = scatter.GaussianBSDF(50.0)
    lens.scatter_max_attempts = 1
    with pytest.raises(scatter.ScatterAttemptsError,
                       match=r"surface 2 \(GaussianBSDF, sigma=50\.0\)"):
        _golden_trace(lens)


def test_python_refusals_on_the_device_paths():
    from optiland_pr_amd import distributed
    from optiland_pr_amd.polarization import create_polarization

    lens = B.lens_and_inputs()[0]
    with pytest.raises(ValueError, match="not traced sharded"):
        distributed.trace_sharded(lens, [B.cases.LENS_FIELD], [B.cases.LENS_WAVELENGTH],
                                  np.zeros(4), np.zeros(4))
    lens.set_polarization(create_polarization("unpolarized"))
    with pytest.raises(ValueError, match="BSDF"):
        _golden_trace(lens)


def test_spot_diagram_on_a_bsdf_lens():
    """SpotDiagram on the golden lens (no Newton surface: its fused trace + statistics path)
    against Optic.trace + spot_statistics, and against the plain lens's statistics."""
    from optiland_pr_amd.analysis import SpotDiagram, spot_statistics

    lens = B.lens_and_inputs()[0]
    g = B.fixture()
    d = types.SimpleNamespace(x=g["lens/px"], y=g["lens/py"])
    spot = SpotDiagram(lens, fields=[B.cases.LENS_FIELD],
                       wavelengths=[B.cases.LENS_WAVELENGTH], distribution=d)
    rays = lens.trace(*B.cases.LENS_FIELD, B.cases.LENS_WAVELENGTH, None, d)
    for a in _abi.RAY_FIELDS:  # the same seed, the same ray numbers: the same trace
        assert torch.equal(getattr(spot.rays, a), getattr(rays, a)), a
    ref = spot_statistics(rays, 1, 1, len(d.x), 0, lens.image_surface)
    assert torch.equal(spot._stats, ref)
    assert float(spot.rms_spot_radius()[0][0]) > 0.1  # scattered: millimetres, not microns
    assert spot.data[0][0].x.numel() == len(d.x)
    plain = SpotDiagram(_plain(B.lens_and_inputs()[0]), fields=[B.cases.LENS_FIELD],
                        wavelengths=[B.cases.LENS_WAVELENGTH], distribution=d)
    assert not torch.equal(plain._stats, spot._stats)


def _op_args():
    from optiland_pr_amd import ops

    lens, segs, px, py = B.lens_and_inputs()
    dlens = raytrace.lens_for(lens, [B.cases.LENS_WAVELENGTH])
    dev = dlens.device
    pxt, pyt = torch.as_tensor(px.copy(), device=dev), torch.as_tensor(py.copy(), device=dev)
    n = len(px)
    return lens, dlens, segs, ops.scatter_args(dlens, segs, pxt, pyt, n, n)


def test_ops_on_the_device_key():
    from optiland_pr_amd import ops

    lens, dlens, segs, args = _op_args()
    rays = torch.ops.ort.trace_pupil_scatter(*args)
    assert rays.is_cuda
    B.check_lens_rays(list(rays.unbind(0)))
    ref = _golden_trace(lens)[1]
    for k, a in enumerate(_abi.RAY_FIELDS):
        assert torch.equal(rays[k], getattr(ref, a)), a
    # resident rays: the generated rays through the sequential op are the pupil op's trace
    n = rays.shape[1]
    rays0 = raytrace.RealRays.empty(n, B.cases.LENS_WAVELENGTH, device=dlens.device)
    raytrace.generate_rays(segs, args[7], args[8], rays0, n, n)
    rin = torch.stack([getattr(rays0, a) for a in _abi.RAY_FIELDS])
    seq = torch.ops.ort.trace_sequential_scatter(*ops.sequential_scatter_args(dlens, rin))
    assert torch.equal(seq, rays)
    # the step op against the fixture
    name = "conic_gauss05"
    ins = B.step_inputs(name, dlens.device)
    kind, sigma = B.cases.make_bsdf(B.cases.STEP_CASES[name][1], B.NS).lower()
    g = B.fixture()
    out = torch.ops.ort.bsdf_scatter(torch.stack(ins[:3]), torch.stack(ins[3:]), kind, sigma,
                                     int(g[f"step/{name}/seed"]),
                                     [B.cases.SURFACE_INDEX, 0, scatter.DEFAULT_MAX_ATTEMPTS])
    for k, f in enumerate(("oL", "oM", "oN")):
        assert np.nanmax(np.abs(out[k].cpu().numpy() - g[f"step/{name}/{f}"])) <= B.TOL_DIR


@pytest.mark.parametrize("which", ["pupil", "sequential", "step"])
def test_opcheck_on_the_device_key(which):
    from optiland_pr_amd import ops

    _, dlens, segs, args = _op_args()
    if which == "pupil":
        op = torch.ops.ort.trace_pupil_scatter
    elif which == "sequential":
        op = torch.ops.ort.trace_sequential_scatter
        n = args[-1][0]
        rays0 = raytrace.RealRays.empty(n, B.cases.LENS_WAVELENGTH, device=dlens.device)
        raytrace.generate_rays(segs, args[7], args[8], rays0, n, n)
        args = ops.sequential_scatter_args(
            dlens, torch.stack([getattr(rays0, a) for a in _abi.RAY_FIELDS]))
    else:
        op = torch.ops.ort.bsdf_scatter
        ins = [t[:200].clone() for t in B.step_inputs("plane_gauss005", dlens.device)]
        args = (torch.stack(ins[:3]), torch.stack(ins[3:]), _abi.BSDF_GAUSSIAN, 0.05, 1,
                [B.cases.SURFACE_INDEX, 0, scatter.DEFAULT_MAX_ATTEMPTS])
    res = torch.library.opcheck(op.default, args)
    assert all(v == "SUCCESS" for v in res.values()), res


def test_requesting_gradients_raises():
    lens = B.lens_and_inputs()[0]
    t = torch.tensor(50.0, dtype=torch.float64, requires_grad=True)
    lens.set_radius(t, 1)
    with pytest.raises(NotImplementedError, match="no derivative"):
        _golden_trace(lens)
    with torch.no_grad():  # without a gradient request the same lens traces
        rays = _golden_trace(lens)[1]
    assert not rays.x.requires_grad and not torch.isnan(rays.x).any()
