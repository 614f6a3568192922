"""IncoherentIrradiance on the MI355X: the fixed-point binning kernels (ort_irradiance_bin, the
CUDA key of torch.ops.ort.irradiance_bin) against the host build bit for bit -- at the ray
counts around a wave, a workgroup and a grid-stride round, at the resolutions around the
LDS-tile threshold -- their invariance under permutation and stream, the drop / NaN rules,
the reference's maps (tests/golden/irradiance.npz) within tests/_irradiance.py's bound,
IncoherentIrradiance end to end and autograd from a lens parameter to an irradiance loss."""

import numpy as np
import pytest
import torch

from tests import _irradiance as R

pytestmark = pytest.mark.gpu

ROW = 128  # pixels per row of the threshold images: TILE = 128 * 128


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs the MI355X")
    return torch.device("cuda")


def both(arrays, mode, gpu, area=None):
    """The op on the device and on the CPU key -> (device result on the host, host result)."""
    d = torch.ops.ort.irradiance_bin(*R.tensors(arrays, gpu), mode, area)
    h = torch.ops.ort.irradiance_bin(*R.tensors(arrays), mode, area)
    assert d.is_cuda and d.dtype == torch.float64 and d.shape == h.shape
    return d.cpu(), h


@pytest.mark.parametrize("mode", [R.HIST, R.BILINEAR])
@pytest.mark.parametrize("n", R.N_SIZES)
def test_ray_counts_device_equals_host(gpu, n, mode):
    """n around one wave (64), one workgroup's quarter (256) and one grid-stride round of the
    binning kernel (1024 threads x 512 workgroups): map and VJP, the same bits as the host."""
    arrays = R.synthetic(n, 9, 7)
    d, h = both(arrays, mode, gpu)
    assert torch.equal(d, h)
    if n:
        assert float(h.abs().sum()) > 0
    if mode == R.BILINEAR:
        g = torch.as_tensor(np.random.default_rng(n).uniform(-1, 1, (7, 9)))
        dv = torch.ops.ort.irradiance_bin_vjp(*R.tensors(arrays, gpu), g.to(gpu), 0.25)
        hv = torch.ops.ort.irradiance_bin_vjp(*R.tensors(arrays), g, 0.25)
        for a, b in zip(dv, hv, strict=True):
            assert a.shape == (n,) and torch.equal(a.cpu(), b)


@pytest.mark.parametrize("mode,res", [
    (R.HIST, (1, 1)), (R.HIST, (2, 3)), (R.BILINEAR, (2, 2)),
    (R.HIST, (ROW, ROW - 1)), (R.HIST, (ROW, ROW)), (R.HIST, (ROW, ROW + 1)),
    (R.BILINEAR, (ROW - 1, ROW)), (R.BILINEAR, (ROW, ROW)), (R.BILINEAR, (ROW + 1, ROW))])
def test_resolutions_device_equals_host(gpu, mode, res):
    """The smallest grids of each mode, and the LDS-tile threshold (16,384 pixels) minus one
    pixel row, at it (the last image summed in LDS) and plus one row (the first summed with
    L2 atomics)."""
    assert ROW * ROW == R.TILE
    arrays = R.synthetic(70001, *res)
    d, h = both(arrays, mode, gpu)
    assert torch.equal(d, h) and float(h.abs().sum()) > 0


@pytest.mark.parametrize("res", [(9, 7), (ROW + 1, ROW)])
@pytest.mark.parametrize("mode", [R.HIST, R.BILINEAR])
def test_all_rays_in_one_pixel(gpu, mode, res):
    """10^5 rays at one point (whole waves on one address: the cross-lane sum), in LDS and in
    L2: the device equals the host, and with unit powers the pixel holds exactly 10^5."""
    n = 100000
    _, _, p, xe, ye = R.synthetic(n, *res)
    x = np.full(n, (xe[3] + xe[4]) / 2 + 0.01)
    y = np.full(n, (ye[2] + ye[3]) / 2 + 0.01)
    d, h = both((x, y, np.abs(p), xe, ye), mode, gpu)
    assert torch.equal(d, h)
    if mode == R.HIST:
        ones, _ = both((x, y, np.ones(n), xe, ye), mode, gpu, 1.0)
        assert float(ones[3, 2]) == n and float(ones.sum()) == n


@pytest.mark.parametrize("res", [(9, 7), (ROW + 1, ROW)])
@pytest.mark.parametrize("mode", [R.HIST, R.BILINEAR])
def test_permutation_and_second_stream_give_identical_bits(gpu, mode, res):
    x, y, p, xe, ye = R.synthetic(150001, *res)
    perm = np.random.default_rng(4).permutation(x.size)
    a = torch.ops.ort.irradiance_bin(*R.tensors((x, y, p, xe, ye), gpu), mode)
    b = torch.ops.ort.irradiance_bin(*R.tensors((x[perm], y[perm], p[perm], xe, ye), gpu), mode)
    ts = R.tensors((x, y, p, xe, ye), gpu)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = torch.ops.ort.irradiance_bin(*ts, mode)
    side.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and float(a.abs().sum()) > 0


def test_nan_and_dropped_rays(gpu):
    xe, ye = R.edges_linspace(3), R.edges_linspace(2)
    cx, cy = (xe[:-1] + xe[1:]) / 2, (ye[:-1] + ye[1:]) / 2
    x = np.array([cx[0], cx[0], cx[1], cx[2], np.nan, cx[1], xe[-1] + 1, cx[2], xe[-1]])
    y = np.array([cy[0], cy[0], cy[1], cy[1], cy[0], np.nan, cy[0], cy[0], ye[-1]])
    p = np.array([1.0, -2.0, np.nan, np.inf, 1.0, 1.0, 1.0, 0.0, 0.5])
    d, h = both((x, y, p, xe, ye), R.HIST, gpu, 1.0)
    want = np.zeros((3, 2))
    want[0, 0] = 1.0
    want[2, 1] = np.nan  # 0.5 on the last edges and the infinite power: NaN (reference: inf)
    assert np.array_equal(d.numpy(), want, equal_nan=True)
    assert np.array_equal(h.numpy(), want, equal_nan=True)
    d, h = both((x, y, p, xe, ye), R.BILINEAR, gpu, 1.0)
    assert np.array_equal(d.numpy(), h.numpy(), equal_nan=True) and np.isnan(d.numpy()).any()


@pytest.mark.parametrize("case", R.CASES + (R.GRAD_CASE,))
def test_goldens_within_bound(gpu, case):
    c = R.fixture()[case]
    x, y, p, xe, ye = (c[k] for k in ("x", "y", "power", "x_edges", "y_edges"))
    area = float(c["pixel_area"])
    if case == R.GRAD_CASE:
        tx, ty, tp, txe, tye = R.tensors((x, y, p, xe, ye))
        _, _, mag = R.bilinear_ref(tx, ty, tp, txe, tye, area)
        cmax = float((R.bilinear_parts(tx, ty, txe, tye)[2] * tp[:, None]).abs().max())
        mode, mag = R.BILINEAR, mag.numpy()
    else:
        kept = (R.pixel_index(xe, x) >= 0) & (R.pixel_index(ye, y) >= 0) & (p > 0)
        mode, mag, cmax = R.HIST, R.abs_sums(x, y, p, xe, ye), p[kept].max()
    d, h = both((x, y, p, xe, ye), mode, gpu, area)
    assert torch.equal(d, h)
    R.assert_within(d.numpy(), c["irr"], R.bound(c["counts"], mag, x.size, cmax, area), case)


@pytest.mark.parametrize("case", ["res_8x6", "px_size", "user_rays", "apodised"])
def test_class_end_to_end(gpu, case):
    """IncoherentIrradiance on the fixture's lens: trace, localise, bin. The traced image
    points agree with the reference's to a few ulp of their size, which can move a ray across
    a pixel edge and carry into the power: every pixel within the golden bound, plus the power
    of the rays that sit within 1e-12 mm of an edge (none in these cases unless a ray is
    traced onto one), plus 64 ulp of the pixel's summed power for the traced intensities."""
    from optiland_pr_amd import IncoherentIrradiance
    from optiland_pr_amd.raytrace import RealRays

    c = R.fixture()[case]
    s = R.spec(c)
    lens = R.build_lens(case)
    kw = {}
    if R.RECIPES[case][1] == "user":
        ux, uy, up = R.user_rays_arrays()
        z = np.zeros_like(ux)
        kw["user_initial_rays"] = RealRays(ux, uy, z - 5.0, z, z, z + 1.0, up,
                                           z + s["wavelength"])
    a = IncoherentIrradiance(lens, num_rays=s["num_rays"],
                             res=(3, 3) if s["px_size"] else s["npix"], px_size=s["px_size"],
                             fields=[s["field"]], wavelengths=[s["wavelength"]],
                             distribution=R.RECIPES[case][0], **kw)
    irr, xe, ye = a.data[0][0]
    assert irr.is_cuda and tuple(irr.shape) == c["irr"].shape == (a.npix_x, a.npix_y)
    assert np.array_equal(xe, c["x_edges"]) and np.array_equal(ye, c["y_edges"])
    x, y, p, area = c["x"], c["y"], c["power"], float(c["pixel_area"])
    kept = (R.pixel_index(xe, x) >= 0) & (R.pixel_index(ye, y) >= 0) & (p > 0)
    atol = R.bound(c["counts"], R.abs_sums(x, y, p, xe, ye), x.size, p[kept].max(), area)
    near = np.zeros_like(c["irr"])
    for e, v, axis in ((xe, x, 0), (ye, y, 1)):
        close = np.min(np.abs(v[:, None] - e[None, :]), axis=1) < 1e-12
        near += np.abs(p[close]).sum() / area
    # the traced power itself carries the trace's rounding (a few ulp per ray)
    atol = atol + near + 64 * 2.0 ** -53 * R.abs_sums(x, y, p, xe, ye) / area
    R.assert_within(irr.cpu().numpy(), c["irr"], atol, case)
    assert float(a.peak_irradiance()[0][0]) == float(irr.max())


def test_autograd_from_a_lens_parameter(gpu):
    """d loss / d (the first radius of the Cooke triplet) through optic.trace (ort::trace_pupil's
    VJP), localize_points and the bilinear map, loss = 1e-6 sum(irr * ramp), against a central
    finite difference of the same loss.

    Step and tolerance, measured on the CPU key first: the fixture's traced points moved along
    their radial directions, x + t u, y + t v, the same loss through the host build. The loss
    is piecewise quadratic in t, so the central difference has no truncation error of its
    own; it agreed with the op's VJP (911.8666456921) to 3.7e-14, 1.1e-13, 2.6e-12, 1.2e-11,
    5.5e-10 relative at steps of 1e-5 ... 1e-9 mm: pure rounding, ~2^-53 |loss| / (h |g|).
    Through the lens the step is 1e-6 of the radius (2.2e-5 mm): truncation ~ (1e-6)^2 times
    the trace's third-order sensitivity, and the trace's own rounding (~1e-14 mm per image
    point, ~1e-11 in the loss) divided by the step is ~1e-8 of the derivative at most. rtol =
    1e-6 leaves two orders of margin over that and is four orders below any missing or
    misplaced term."""
    from optiland_pr_amd import IncoherentIrradiance

    lens = R.build_lens(R.GRAD_CASE)
    r0 = float(lens.surface_group.surfaces[1].geometry.radius)
    ramp = torch.as_tensor(np.add.outer(np.linspace(-1, 1, 5), 0.5 * np.linspace(0, 1, 6) ** 2),
                           device=gpu)

    def loss_at(radius):
        lens.set_radius(radius, 1)
        a = IncoherentIrradiance(lens, num_rays=7, res=(6, 5), fields=[(0.0, 0.0)],
                                 wavelengths=[0.55], distribution="hexapolar",
                                 differentiable=True)
        irr = a.data[0][0][0]
        assert tuple(irr.shape) == (5, 6)  # [ny, nx]
        return (irr * ramp).sum() * 1e-6

    r = torch.tensor(r0, dtype=torch.float64, requires_grad=True)
    loss = loss_at(r)
    assert loss.requires_grad
    loss.backward()
    g = float(r.grad)
    h = 1e-6 * abs(r0)
    fd = (float(loss_at(r0 + h)) - float(loss_at(r0 - h))) / (2 * h)
    print(f"d loss / d radius: autograd {g:.12g}, central difference {fd:.12g}, "
          f"relative difference {abs(g - fd) / abs(fd):.3g}")
    assert g != 0.0
    assert abs(g - fd) <= 1e-6 * abs(fd)
