"""IncoherentIrradiance's binning on the CPU: the host build (ort_host_irradiance_bin, the CPU
key of torch.ops.ort.irradiance_bin) against NumPy / torch restatements of the reference's two
paths and against the reference's own maps (tests/golden/irradiance.npz): pixel choice,
values within the derived bound (tests/_irradiance.py), order independence, the VJP, argument
checks, and the class with the trace replaced by the fixture's traced rays (the trace itself
needs the device; tests/test_gpu_irradiance.py runs the class end to end)."""

import os
import re
import types

import numpy as np
import pytest
import torch

from optiland_pr_amd import _abi, host
from tests import _irradiance as R
from tests.conftest import REPO

EDGE_KINDS = {"linspace": R.edges_linspace, "arange": R.edges_arange,
              "nonuniform": R.edges_nonuniform}


def op(x, y, p, xe, ye, mode, area=None):
    return torch.ops.ort.irradiance_bin(*R.tensors((x, y, p, xe, ye)), mode, area)


def probes(edges):
    """Values on every edge, one ulp either side, between, outside and NaN."""
    e = np.asarray(edges)
    v = [e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), (e[:-1] + e[1:]) / 2,
         [e[0] - 1.0, e[-1] + 1.0, -np.inf, np.inf, np.nan]]
    return np.concatenate([np.asarray(a, dtype=float) for a in v])


@pytest.mark.parametrize("kind", sorted(EDGE_KINDS))
@pytest.mark.parametrize("nb", [1, 2, 13])
def test_pixel_index_is_searchsorted(kind, nb):
    """One ray per call, so the single non-zero pixel is that ray's pixel: identical to
    searchsorted(side='right') - 1 with the last edge in the last bin, along x and along y."""
    e = EDGE_KINDS[kind](nb)
    assert np.all(np.diff(e) > 0) and len(e) == nb + 1
    other = np.array([0.0, 1.0])
    v = probes(e)
    want = R.pixel_index(e, v)
    assert (want == nb - 1).sum() >= 2 and (want == -1).sum() >= 5  # last edge; dropped
    one, half = np.array([1.0]), np.array([0.5])
    for val, k in zip(v, want, strict=True):
        mx = op(np.array([val]), half, one, e, other, R.HIST, 1.0).numpy()
        my = op(half, np.array([val]), one, other, e, R.HIST, 1.0).numpy()
        assert mx.shape == (nb, 1) and my.shape == (1, nb)
        expect = np.zeros(nb)
        if k >= 0:
            expect[k] = 1.0
        assert np.array_equal(mx[:, 0], expect), (kind, val, k)
        assert np.array_equal(my[0, :], expect), (kind, val, k)


@pytest.mark.parametrize("kind", sorted(EDGE_KINDS))
def test_unit_powers_bit_equal_numpy(kind):
    g = np.random.default_rng(5)
    xe, ye = EDGE_KINDS[kind](11), EDGE_KINDS[kind](7)
    x = np.concatenate([g.uniform(xe[0] - 0.1, xe[-1] + 0.1, 4000), probes(xe)])
    y = np.concatenate([g.uniform(ye[0] - 0.1, ye[-1] + 0.1, 4000),
                        np.resize(probes(ye), probes(xe).size)])
    p = np.ones_like(x)
    want, _, _ = np.histogram2d(x, y, bins=[xe, ye])
    got = op(x, y, p, xe, ye, R.HIST, 1.0).numpy()
    assert want.sum() > 2000 and np.array_equal(got, want)
    area = (xe[1] - xe[0]) * (ye[1] - ye[0])
    assert np.array_equal(op(x, y, p, xe, ye, R.HIST).numpy(), want / area)  # the default area


def test_general_powers_within_bound():
    x, y, p, xe, ye = R.synthetic(20000, 9, 5)
    area = (xe[1] - xe[0]) * (ye[1] - ye[0])
    want = R.histogram_ref(x, y, p, xe, ye, area)
    got = op(x, y, p, xe, ye, R.HIST).numpy()
    atol = R.bound(R.histogram_counts(x, y, p, xe, ye), R.abs_sums(x, y, p, xe, ye), x.size,
                   p.max(), area)
    R.assert_within(got, want, atol, "synthetic 20000 rays")
    assert np.all(got[want > 0] > 0)


@pytest.mark.parametrize("case", R.CASES)
def test_golden_maps_host_and_cpu_key(case):
    c = R.fixture()[case]
    x, y, p, xe, ye = (c[k] for k in ("x", "y", "power", "x_edges", "y_edges"))
    area = float(c["pixel_area"])
    assert np.array_equal(R.histogram_ref(x, y, p, xe, ye, area), c["irr"])
    kept = R.pixel_index(xe, x) >= 0
    kept &= (R.pixel_index(ye, y) >= 0) & (p > 0)
    atol = R.bound(c["counts"], R.abs_sums(x, y, p, xe, ye), x.size, p[kept].max(), area)
    got = op(x, y, p, xe, ye, R.HIST, area)
    assert got.dtype == torch.float64 and tuple(got.shape) == c["irr"].shape
    R.assert_within(got.numpy(), c["irr"], atol, case)
    direct = host.irradiance_bin(*R.tensors((x, y, p, xe, ye)), R.HIST, area)
    assert torch.equal(direct.reshape(got.shape), got)


def test_bilinear_map_and_vjp_against_reference_gradients():
    """The reference's torch-backend grad_mode run: its map and torch autograd's gradients of
    sum(irr * mask). Gradient tolerance: each of g_x, g_y, g_power is a sum of four products
    of O(1) weights with |mask| <= 1 entries, so 32 ulp of its scale (|p| dw / area resp.
    1 / area) covers both sides' roundings."""
    c = R.fixture()[R.GRAD_CASE]
    x, y, p, xe, ye = (c[k] for k in ("x", "y", "power", "x_edges", "y_edges"))
    area = float(c["pixel_area"])
    tx, ty, tp, txe, tye = R.tensors((x, y, p, xe, ye))
    ref, cnt, mag = R.bilinear_ref(tx, ty, tp, txe, tye, area)
    assert np.array_equal(ref.numpy(), c["irr"]) and np.array_equal(cnt.numpy(), c["counts"])
    _, _, w = R.bilinear_parts(tx, ty, txe, tye)
    cmax = float((w * tp[:, None]).detach().abs().max())
    for t in (tx, ty, tp):
        t.requires_grad_(True)
    got = torch.ops.ort.irradiance_bin(tx, ty, tp, txe, tye, R.BILINEAR, area)
    assert tuple(got.shape) == (len(ye) - 1, len(xe) - 1) == c["irr"].shape
    R.assert_within(got.detach().numpy(), c["irr"],
                    R.bound(c["counts"], mag.numpy(), x.size, cmax, area), "grad_mode map")
    (got * torch.as_tensor(np.array(c["mask"]))).sum().backward()
    dw = 1.0 / min(np.diff(xe).min(), np.diff(ye).min())
    scale = {"grad_x": np.abs(p).max() * dw / area, "grad_y": np.abs(p).max() * dw / area,
             "grad_power": 1.0 / area}
    for name, t in (("grad_x", tx), ("grad_y", ty), ("grad_power", tp)):
        d = np.max(np.abs(t.grad.numpy() - c[name]))
        print(f"{name}: max |d| = {d:.3g}, tolerance {32 * 2.0 ** -53 * scale[name]:.3g}")
        assert d <= 32 * 2.0 ** -53 * scale[name], name


def test_bilinear_matches_torch_restatement_on_probes():
    """Points on every pixel centre, one ulp either side, outside the centres (extrapolated
    weights) and at random: the map against the reference's formulas, the VJP against torch
    autograd through them."""
    g = np.random.default_rng(11)
    for kind in sorted(EDGE_KINDS):
        xe, ye = EDGE_KINDS[kind](6), EDGE_KINDS[kind](4)
        xc, yc = (xe[:-1] + xe[1:]) / 2, (ye[:-1] + ye[1:]) / 2
        x = np.concatenate([xc, np.nextafter(xc, -np.inf), np.nextafter(xc, np.inf),
                            [xe[0] - 0.3, xe[-1] + 0.3], g.uniform(xe[0], xe[-1], 300)])
        y = np.concatenate([g.uniform(ye[0], ye[-1], x.size - 3 * yc.size), yc,
                            np.nextafter(yc, -np.inf), np.nextafter(yc, np.inf)])
        p = g.uniform(-1.0, 1.0, x.size) / 3.0  # no power filter in this mode
        tx, ty, tp, txe, tye = R.tensors((x, y, p, xe, ye))
        area = 0.37
        for t in (tx, ty, tp):
            t.requires_grad_(True)
        ref, cnt, mag = R.bilinear_ref(tx, ty, tp, txe, tye, area)
        _, _, w = R.bilinear_parts(tx, ty, txe, tye)
        cmax = float((w * tp[:, None]).detach().abs().max())
        got = torch.ops.ort.irradiance_bin(tx, ty, tp, txe, tye, R.BILINEAR, area)
        R.assert_within(got.detach().numpy(), ref.detach().numpy(),
                        R.bound(cnt.numpy(), mag.numpy(), x.size, cmax, area), kind)
        mask = torch.as_tensor(g.uniform(-1.0, 1.0, tuple(ref.shape)))
        want = torch.autograd.grad((ref * mask).sum(), (tx, ty, tp))
        have = torch.autograd.grad((got * mask).sum(), (tx, ty, tp))
        for a, b in zip(have, want, strict=True):
            tol = 64 * 2.0 ** -53 * float(b.abs().max() + a.abs().max())
            assert float((a - b).abs().max()) <= tol


def test_gradcheck_bilinear_away_from_centres():
    """Rays a quarter of a pixel off the centres: no cell changes within gradcheck's step."""
    xe, ye = R.edges_linspace(5), R.edges_arange(4)
    xc, yc = (xe[:-1] + xe[1:]) / 2, (ye[:-1] + ye[1:]) / 2
    gx, gy = np.meshgrid(xc[:-1] + 0.25 * np.diff(xc), yc[:-1] + 0.3 * np.diff(yc))
    x, y = gx.reshape(-1), gy.reshape(-1)
    p = np.linspace(0.2, 1.1, x.size)
    tx, ty, tp, txe, tye = R.tensors((x, y, p, xe, ye))
    for t in (tx, ty, tp):
        t.requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda a, b, c: torch.ops.ort.irradiance_bin(a, b, c, txe, tye, R.BILINEAR, 0.5),
        (tx, ty, tp), eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("mode", [R.HIST, R.BILINEAR])
def test_permutation_gives_identical_bits(mode):
    x, y, p, xe, ye = R.synthetic(30000, 7, 6)
    perm = np.random.default_rng(2).permutation(x.size)
    a = op(x, y, p, xe, ye, mode)
    b = op(x[perm], y[perm], p[perm], xe, ye, mode)
    assert torch.equal(a, b) and float(a.abs().sum()) > 0
    lib = host._native.load_host()
    lib.ort_host_set_threads(1)  # the value does not depend on the thread count either
    try:
        assert torch.equal(op(x, y, p, xe, ye, mode), a)
    finally:
        lib.ort_host_set_threads(0)


def test_two_to_the_twenty_rays_of_cmax_sum_exactly():
    """n = 2^20 contributions of cmax in one pixel: L = 20, so a contribution keeps 62 - 20 =
    42 bits below its leading one; a cmax of 40 significant bits is held exactly and the sum
    n * cmax (exact in fp64) comes back without overflow or rounding."""
    n = 1 << 20
    cmax = float(np.ldexp(np.floor(np.ldexp(0.7, 40)), -40))
    xe, ye = R.edges_linspace(3), R.edges_linspace(2)
    x = np.full(n, (xe[1] + xe[2]) / 2)
    y = np.full(n, (ye[0] + ye[1]) / 2)
    got = op(x, y, np.full(n, cmax), xe, ye, R.HIST, 1.0).numpy()
    want = np.zeros((3, 2))
    want[1, 0] = n * cmax
    assert np.array_equal(got, want)
    assert R.exponent(n, cmax) == 62 - 0 - 20


def test_dropped_and_non_finite_rays():
    xe, ye = R.edges_linspace(3), R.edges_linspace(2)
    cx, cy = (xe[:-1] + xe[1:]) / 2, (ye[:-1] + ye[1:]) / 2
    x = np.array([cx[0], cx[0], cx[1], cx[2], np.nan, cx[1], xe[-1] + 1, cx[2]])
    y = np.array([cy[0], cy[0], cy[1], cy[1], cy[0], np.nan, cy[0], cy[0]])
    p = np.array([1.0, -2.0, np.nan, np.inf, 1.0, 1.0, 1.0, 0.0])
    got = op(x, y, p, xe, ye, R.HIST, 1.0).numpy()
    want = np.zeros((3, 2))
    want[0, 0] = 1.0
    want[2, 1] = np.nan  # the infinite power: NaN here, +inf in the reference
    assert np.array_equal(got, want, equal_nan=True)
    # bilinear: a NaN coordinate or power poisons its four pixels and nothing else
    x = np.array([cx[0] + 0.1, np.nan, cx[1] + 0.1])
    y = np.array([cy[0] + 0.1, cy[0], cy[0] + 0.1])
    p = np.array([1.0, 1.0, np.nan])
    got = op(x, y, p, xe, ye, R.BILINEAR, 1.0).numpy()
    assert got.shape == (2, 3) and np.isnan(got[:, 1:]).all() and np.isfinite(got[:, 0]).all()
    empty = np.zeros(0)
    assert np.array_equal(op(empty, empty, empty, xe, ye, R.HIST).numpy(), np.zeros((3, 2)))
    assert np.array_equal(op(empty, empty, empty, xe, ye, R.BILINEAR).numpy(), np.zeros((2, 3)))


def test_histogram_refuses_grad_and_names_bilinear():
    x, y, p, xe, ye = R.tensors(R.synthetic(10, 3, 3))
    x.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="BIN_BILINEAR"):
        torch.ops.ort.irradiance_bin(x, y, p, xe, ye, R.HIST)
    assert torch.ops.ort.irradiance_bin(x.detach(), y, p, xe, ye, R.HIST).shape == (3, 3)


def test_argument_errors():
    x, y, p, xe, ye = R.tensors(R.synthetic(10, 3, 3))
    f = torch.ops.ort.irradiance_bin
    with pytest.raises(ValueError, match="float64"):
        f(x.float(), y, p, xe, ye, R.HIST)
    with pytest.raises(ValueError, match="lengths"):
        f(x[:5], y, p, xe, ye, R.HIST)
    with pytest.raises(ValueError, match="strictly increasing"):
        f(x, y, p, xe.flip(0), ye, R.HIST)
    with pytest.raises(ValueError, match="strictly increasing"):
        f(x, y, p, xe, torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64), R.HIST)
    with pytest.raises(ValueError, match="mode"):
        f(x, y, p, xe, ye, 2)
    with pytest.raises(ValueError, match="at least 2"):
        f(x, y, p, xe[:2], ye, R.BILINEAR)
    with pytest.raises(ValueError, match="at least 1"):
        f(x, y, p, xe[:1], ye, R.HIST)
    with pytest.raises(ValueError, match="exceed"):
        f(x, y, p, torch.zeros(8194, dtype=torch.float64),
          torch.zeros(8194, dtype=torch.float64), R.HIST)
    with pytest.raises(ValueError, match="grad must be"):
        torch.ops.ort.irradiance_bin_vjp(x, y, p, xe, ye, torch.zeros(2, 2, dtype=torch.float64))
    lib = host._native.load_host()
    null = None
    assert lib.ort_host_irradiance_bin(null, null, null, 0, xe.data_ptr(), 1, ye.data_ptr(), 3,
                                       R.BILINEAR, 0.0, x.data_ptr()) == -1  # nx < 2
    assert lib.ort_host_irradiance_bin(null, null, null, 0, xe.data_ptr(), 3, ye.data_ptr(), 3,
                                       7, 0.0, x.data_ptr()) == -1  # unknown mode
    assert lib.ort_host_irradiance_bin(null, null, null, -1, xe.data_ptr(), 3, ye.data_ptr(), 3,
                                       R.HIST, 0.0, x.data_ptr()) == -1


def test_opcheck_both_ops():
    x, y, p, xe, ye = R.tensors(R.synthetic(50, 4, 3))
    torch.library.opcheck(torch.ops.ort.irradiance_bin, (x, y, p, xe, ye, R.HIST))
    xg, yg, pg = (t.clone().requires_grad_(True) for t in (x, y, p))
    torch.library.opcheck(torch.ops.ort.irradiance_bin, (xg, yg, pg, xe, ye, R.BILINEAR, 0.3))
    g = torch.ones(3, 4, dtype=torch.float64)
    torch.library.opcheck(torch.ops.ort.irradiance_bin_vjp, (x, y, p, xe, ye, g, 0.3))


def test_abi_constants_match_headers():
    text = open(os.path.join(REPO, "include", "optiland_rt.h")).read()
    assert int(re.search(r"ORT_BIN_HISTOGRAM = (\d+)", text).group(1)) == _abi.BIN_HISTOGRAM
    assert int(re.search(r"ORT_BIN_BILINEAR = (\d+)", text).group(1)) == _abi.BIN_BILINEAR
    assert int(re.search(r"#define ORT_IRRADIANCE_TILE_PIXELS (\d+)", text).group(1)) == \
        _abi.IRRADIANCE_TILE_PIXELS
    assert int(re.search(r"#define ORT_IRRADIANCE_MAX_PIXELS (\d+)", text).group(1)) == \
        _abi.IRRADIANCE_MAX_PIXELS
    assert _abi.irradiance_exponent(1, 1.0) == 61 and _abi.irradiance_exponent(5, 0.75) == 59
    assert _abi.irradiance_exponent(100, 0.0) == 0


# -- the class, with the fixture's traced rays in place of the device trace ----------------
def _stubbed(case, **kw):
    from optiland_pr_amd import IncoherentIrradiance
    from optiland_pr_amd.raytrace import RealRays

    c = R.fixture()[case]
    s = R.spec(c)
    lens = R.build_lens(case)
    traced = types.SimpleNamespace(**{k: torch.as_tensor(np.array(c[v]))
                                      for k, v in (("x", "gx"), ("y", "gy"), ("z", "gz"),
                                                   ("i", "power"))})
    if R.RECIPES[case][1] == "user":
        ux, uy, up = R.user_rays_arrays()
        zeros = np.zeros_like(ux)
        kw["user_initial_rays"] = RealRays(ux, uy, zeros - 5.0, zeros, zeros, zeros + 1.0, up,
                                           zeros + s["wavelength"], device="cpu")

        def trace_group(rays):
            assert len(rays) == ux.size and rays.x is not kw["user_initial_rays"].x
            rays.x, rays.y, rays.z, rays.i = traced.x, traced.y, traced.z, traced.i

        lens.surface_group.trace = trace_group
    else:
        lens.trace = lambda Hx, Hy, wl, num_rays, dist: traced
    if kw.pop("grad", False):
        traced.x.requires_grad_(True)
    res = (3, 3) if s["px_size"] else s["npix"]
    a = IncoherentIrradiance(lens, num_rays=s["num_rays"], res=res, px_size=s["px_size"],
                             fields=[s["field"]], wavelengths=[s["wavelength"]],
                             distribution=R.RECIPES[case][0], **kw)
    return a, c, s


@pytest.mark.parametrize("case", R.CASES)
def test_class_reproduces_reference_maps(case, capsys):
    a, c, s = _stubbed(case)
    irr, xe, ye = a.data[0][0]
    assert isinstance(xe, np.ndarray) and isinstance(ye, np.ndarray) and torch.is_tensor(irr)
    assert np.array_equal(xe, c["x_edges"]) and np.array_equal(ye, c["y_edges"])
    assert (a.npix_x, a.npix_y) == s["npix"] == tuple(irr.shape)  # X is the row index
    x, y, p = c["x"], c["y"], c["power"]
    kept = (R.pixel_index(xe, x) >= 0) & (R.pixel_index(ye, y) >= 0) & (p > 0)
    atol = R.bound(c["counts"], R.abs_sums(x, y, p, xe, ye), x.size, p[kept].max(),
                   float(c["pixel_area"]))
    R.assert_within(irr.numpy(), c["irr"], atol, case)
    assert float(a.peak_irradiance()[0][0]) == irr.numpy().max()
    printed = capsys.readouterr().out
    if s["px_size"]:
        assert "res parameter ignored - derived from px_size instead → (6,4) pixels" in printed
        assert "→ (5,4) pixels" in printed
    else:
        assert "IncoherentIrradiance" not in printed


def test_class_picks_the_bilinear_mode_for_inputs_that_require_grad():
    a, c, s = _stubbed(R.GRAD_CASE, grad=True)
    irr = a.data[0][0][0]
    assert tuple(irr.shape) == (s["npix"][1], s["npix"][0]) == c["irr"].shape  # [ny, nx]
    assert irr.requires_grad
    tx, ty, tp, txe, tye = R.tensors([c[k] for k in ("x", "y", "power", "x_edges", "y_edges")])
    _, cnt, mag = R.bilinear_ref(tx, ty, tp, txe, tye, 1.0)
    cmax = float((R.bilinear_parts(tx, ty, txe, tye)[2] * tp[:, None]).abs().max())
    R.assert_within(irr.detach().numpy(), c["irr"],
                    R.bound(cnt.numpy(), mag.numpy(), tx.numel(), cmax, float(c["pixel_area"])),
                    "class, bilinear")
    forced = _stubbed(R.GRAD_CASE, differentiable=False)[0].data[0][0][0]
    assert tuple(forced.shape) == s["npix"] and not forced.requires_grad
    assert _stubbed("res_8x6", differentiable=True)[0].data[0][0][0].shape == (6, 8)


def test_class_error_types():
    from optiland_pr_amd import IncoherentIrradiance
    from optiland_pr_amd.samples import CookeTriplet

    with pytest.raises(ValueError, match="no physical aperture"):
        IncoherentIrradiance(CookeTriplet(), res=(4, 4))
    with pytest.raises(TypeError, match="RealRays"):
        IncoherentIrradiance(R.build_lens("res_8x6"), res=(4, 4), user_initial_rays=object())


def test_public_export():
    import optiland_pr_amd
    from optiland_pr_amd.irradiance import IncoherentIrradiance

    assert optiland_pr_amd.IncoherentIrradiance is IncoherentIrradiance
    assert "IncoherentIrradiance" in optiland_pr_amd.__all__
