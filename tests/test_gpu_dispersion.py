"""GPU: every branch of the per-ray dispersion (csrc/ort_material.h) as the device evaluates
it -- material_nk_kernel and the F_WRAY trace kernels -- on the fixture materials of
tests/test_dispersion_cpu.py (tests/golden/dispersion_materials.json, dispersion.npz: the
reference's MaterialFile.n / .k and SurfaceGroup.trace, an mpmath value of n), numpy.interp
on synthetic tables, and the Abbe model's range ends.

Tolerances (the CPU file's). Branches without pow (_dispersion.pow_free): n bit-equal to
the reference, NaN / inf positions included. Branches with the device pow:
|n - n_exact| <= max(4 n_err_ref, 2 ulp) |n_exact| on the finite points, the reference's
NaN / inf positions; the bound is against the exact value, never the code under test. k:
bit-equal everywhere. Traces: pow-free materials bit-exact in x, y, z, L, M, N, opd; pow
materials and the Newton singlet 1e-9 mm / 1e-11; intensity rtol 1e-12.

Every input is a fixture sweep (at most 3311 points) or 256 rays.
"""

import ctypes as C

import numpy as np
import pytest

from tests import _dispersion as D

pytestmark = pytest.mark.gpu

K_BLOCK = 256  # csrc/ort_kernels.h kBlock: material_nk_kernel's workgroup (ort_k_closed.hip)


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("needs the MI355X")
    from optiland_pr_amd import _native

    _native.load()
    return torch


def _device_material(material, primary):
    """-> (DeviceLens of the singlet, index of `material` in it)."""
    from optiland_pr_amd.lowering import lower_surface_group
    from optiland_pr_amd.raytrace import DeviceLens

    lens = D.singlet(material, primary)
    table = lower_surface_group(lens.surface_group, [lens.primary_wavelength])
    mi = [i for i, m in enumerate(table.materials) if m is material]
    assert len(mi) == 1
    return DeviceLens(table), mi[0]


def _nk(material, primary, w):
    from optiland_pr_amd.raytrace import material_nk

    dl, mi = _device_material(material, primary)
    return tuple(v.cpu().numpy() for v in material_nk(dl, mi, w))


def _same(got, ref, msg):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=msg)
    ok = ~np.isnan(ref)
    np.testing.assert_array_equal(got[ok], ref[ok], err_msg=msg)
    np.testing.assert_array_equal(np.signbit(got[ok]), np.signbit(ref[ok]), err_msg=msg)


# ---- a. material_nk of every fixture material -------------------------------------------
@pytest.mark.parametrize("src", D.TRACEABLE)
def test_device_dispersion_every_branch(torch, src):
    from optiland_pr_amd.materials import Material

    g = D.golden()
    e = D.entries()[src]
    n, k = _nk(Material.from_entry(e), D.primary_wavelength(e), g[f"n/{src}/w"])
    ref = g[f"n/{src}/n"]
    if D.pow_free(e):
        _same(n, ref, f"{src} n")
    else:
        exact, err = g[f"n/{src}/n_exact"], float(g[f"n/{src}/n_err_ref"])
        np.testing.assert_array_equal(np.isnan(n), np.isnan(ref), err_msg=src)
        np.testing.assert_array_equal(np.isinf(n), np.isinf(ref), err_msg=src)
        ok = np.isfinite(exact)
        bound = max(4 * err, 2 * D.EPS) * np.abs(exact[ok])
        ratio = float(np.max(np.abs(n[ok] - exact[ok]) / bound))
        print(f"{src}: device pow, worst error / bound = {ratio:.3f} (n_err_ref {err:.2e}, "
              f"{int(np.sum(n[ok] != ref[ok]))} of {int(ok.sum())} points differ from NumPy)")
        assert ratio <= 1.0, src
    _same(k, g[f"n/{src}/k"], f"{src} k")


# ---- b. launch shape --------------------------------------------------------------------
@pytest.mark.parametrize("src", ["glass/ami/AMTIR-1", "main/AgGaS2/Kato-e"])
def test_material_nk_launch_shapes(torch, src):
    """One wavelength, one more than a workgroup, and either output alone (NULL for the
    other: ort_material_nk through the C ABI, which raytrace.material_nk cannot express)."""
    from optiland_pr_amd import _native
    from optiland_pr_amd.materials import Material
    from optiland_pr_amd.raytrace import _stream_handle, material_nk

    g = D.golden()
    e = D.entries()[src]
    dl, mi = _device_material(Material.from_entry(e), D.primary_wavelength(e))
    w_all = g[f"n/{src}/w"]
    pick = np.linspace(0, w_all.size - 1, K_BLOCK + 1).astype(int)
    w = np.ascontiguousarray(w_all[pick])
    full_n, full_k = (v.cpu().numpy() for v in material_nk(dl, mi, w))
    assert full_n.size == K_BLOCK + 1
    all_n, all_k = (v.cpu().numpy() for v in material_nk(dl, mi, w_all))
    _same(full_n, all_n[pick], "n, kBlock + 1")  # the second block's one thread included
    _same(full_k, all_k[pick], "k, kBlock + 1")
    _same(full_k, g[f"n/{src}/k"][pick], "k")
    for i in (0, K_BLOCK):
        one_n, one_k = (v.cpu().numpy() for v in material_nk(dl, mi, w[i:i + 1]))
        assert one_n.shape == (1,) and one_n[0] == full_n[i] and one_k[0] == full_k[i]
    lib = _native.load()
    wd = torch.as_tensor(w, device="cuda")
    for which in (0, 1):
        out = torch.full((w.size + 1,), -7.0, dtype=torch.float64, device="cuda")
        args = [None, None]
        args[which] = out.data_ptr()
        rc = lib.ort_material_nk(C.byref(dl.c), mi, wd.data_ptr(), w.size, args[0], args[1],
                                 _stream_handle())
        assert rc == 0
        got = out.cpu().numpy()
        _same(got[:-1], (full_n, full_k)[which], "single output")
        assert got[-1] == -7.0  # nothing past n
    assert lib.ort_material_nk(C.byref(dl.c), mi, wd.data_ptr(), 0, None, None,
                               _stream_handle()) == 0


# ---- c. np_interp edges -----------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.interp_tables()))
def test_device_np_interp_edges(torch, name):
    """np_interp = numpy.interp bit for bit (_dispersion.interp_tables / interp_queries:
    table lengths 1 .. 9, NaN and inf in fp, repeated wavelengths at the start, inside and at
    the end; every knot, both its neighbours, beyond both ends, NaN)."""
    xp, fp = D.interp_tables()[name]
    q = D.interp_queries(xp)
    with np.errstate(all="ignore"):
        ref = np.interp(q, xp, fp)
    n, k = _nk(D.tabulated(xp, fp), float(xp[0]), q)
    _same(n, ref, name)
    assert np.all(k == 0.0)


# ---- d. tables that are not strictly increasing -----------------------------------------
@pytest.mark.parametrize("src", ["glass/hikari/CaF/NICF-A", "main/Ag/Yang"])
def test_repeated_wavelengths_match_numpy(torch, src):
    """Non-decreasing tables with a repeated wavelength: numpy.interp bit for bit, at the
    repeated wavelength and its neighbours too (they are in the fixture sweep)."""
    from optiland_pr_amd.materials import Material

    e = D.entries()[src]
    w = D.golden()[f"n/{src}/w"]
    n, k = _nk(Material.from_entry(e), D.primary_wavelength(e), w)
    checked = 0
    for got, xk, fk in ((n, "n_wavelength", "n"), (k, "k_wavelength", "k")):
        if e[xk] is None or e["formula"].startswith("formula") and fk == "n":
            continue
        xp, fp = np.array(e[xk]), np.array(e[fk])
        dup = xp[1:][np.diff(xp) == 0]
        assert dup.size and np.all(np.diff(xp) >= 0)
        for v in dup:
            assert {np.nextafter(v, 0), v, np.nextafter(v, 9)} <= set(w.tolist())
        _same(got, np.interp(w, xp, fp), f"{src} {fk}")
        checked += 1
    assert checked >= 1


def test_decreasing_table_is_refused_per_ray(torch):
    """glass/lzos/CTK8 (one decreasing step): numpy.interp there depends on the query order
    (tests/test_dispersion_cpu.py), so per-ray calls raise and name the material; one
    wavelength per call -- host NumPy tables -- still traces."""
    from optiland_pr_amd.lowering import lower_surface_group
    from optiland_pr_amd.materials import Material
    from optiland_pr_amd.raytrace import DeviceLens, RealRays, material_nk, trace_rays

    e = D.entries()["glass/lzos/CTK8"]
    m = Material.from_entry(e)
    lens = D.singlet(m, 0.55)
    table = lower_surface_group(lens.surface_group, [0.55])
    dl = DeviceLens(table)
    mi = [i for i, v in enumerate(table.materials) if v is m][0]
    with pytest.raises(ValueError, match=r"Material\('CTK8'.*wavelengths decrease"):
        material_nk(dl, mi, np.array([0.5, 0.6]))
    air = [i for i, v in enumerate(table.materials) if not hasattr(v, "source")][0]
    n, _ = material_nk(dl, air, np.array([0.5, 0.6]))  # air, in the same lens: fine
    assert n.cpu().tolist() == [1.0, 1.0]

    def rays(w):
        z = torch.zeros(8, dtype=torch.float64, device="cuda")
        return RealRays(z + 0.5, z.clone(), z - 5, z.clone(), z.clone(), z + 1, z + 1, w)

    r = rays(torch.linspace(0.5, 0.6, 8, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="CTK8"):
        lens.surface_group.trace(r)
    with pytest.raises(ValueError, match="CTK8"):
        trace_rays(dl, r, r, per_ray_w=True)
    r = rays(0.55)
    lens.surface_group.trace(r)
    assert torch.isfinite(r.x).all() and float(r.x[0]) != 0.5


# ---- e. Abbe range ends -----------------------------------------------------------------
def test_abbe_range_boundaries(torch):
    from optiland_pr_amd.materials import AbbeMaterial
    from optiland_pr_amd.raytrace import RealRays
    from tests._cases import build_lens

    lo, hi = 0.380, 0.750
    m = AbbeMaterial(1.62041, 60.32)
    w = np.array([np.nextafter(lo, 0), lo, np.nextafter(lo, 1), np.nextafter(hi, 0), hi,
                  np.nextafter(hi, 1)])
    n, k = _nk(m, 0.55, w)
    inside = np.array([False, True, True, True, True, False])
    np.testing.assert_array_equal(n[inside], np.polyval(m._p, w[inside]))
    assert np.all(np.isnan(n[~inside])) and np.all(k == 0.0)

    lens = build_lens("cooke_abbe")
    for wv, ok in zip(w, inside, strict=True):
        wt = torch.full((64,), 0.55, dtype=torch.float64, device="cuda")
        wt[17] = float(wv)
        z = torch.zeros(64, dtype=torch.float64, device="cuda")
        r = RealRays(z, z.clone(), z.clone() - 5, z.clone(), z.clone(), z.clone() + 1,
                     z.clone() + 1, wt)
        if ok:
            lens.surface_group.trace(r)
            assert torch.isfinite(r.x).all()
        else:
            with pytest.raises(ValueError, match="Wavelength out of range for this model"):
                lens.surface_group.trace(r)


# ---- f. traces through the F_WRAY kernels -----------------------------------------------
def _trace(torch, src, prefix, asphere):
    from optiland_pr_amd.materials import Material
    from optiland_pr_amd.raytrace import RealRays

    g = D.golden()
    e = D.entries()[src]
    p = f"{prefix}/{src}"
    lens = D.singlet(Material.from_entry(e), D.primary_wavelength(e), asphere)
    rays = RealRays(*(torch.as_tensor(g[f"{p}/in_{a}"], device="cuda") for a in D.RAY_IN),
                    torch.as_tensor(g[f"{p}/w"], device="cuda"))
    assert len(rays) == 256 and np.unique(g[f"{p}/w"]).size == 256
    lens.surface_group.trace(rays)
    return {a: getattr(rays, a).cpu().numpy() for a in D.RAY_OUT}, p


def _check_trace(got, p, exact):
    g = D.golden()
    for a in ("x", "y", "z", "L", "M", "N", "opd"):
        if exact:
            np.testing.assert_array_equal(got[a], g[f"{p}/{a}"], err_msg=f"{p} {a}")
        else:
            tol = 1e-11 if a in ("L", "M", "N") else 1e-9
            np.testing.assert_allclose(got[a], g[f"{p}/{a}"], rtol=0, atol=tol, err_msg=f"{p} {a}")
    np.testing.assert_allclose(got["i"], g[f"{p}/i"], rtol=1e-12, atol=0, err_msg=f"{p} i")


@pytest.mark.parametrize("src", D.TRACEABLE)
def test_per_ray_trace_closed_form(torch, src):
    """trace_closed_kernel<F_WRAY>: 256 rays, 256 wavelengths, through the singlet."""
    got, p = _trace(torch, src, "trace", False)
    _check_trace(got, p, D.pow_free(D.entries()[src]))


@pytest.mark.parametrize("src", D.NEWTON)
def test_per_ray_trace_newton(torch, src):
    """trace_kernel<F_WRAY>: the second surface an even asphere."""
    got, p = _trace(torch, src, "trace_asph", True)
    _check_trace(got, p, False)


@pytest.mark.parametrize("src", D.POW_FREE)
def test_per_ray_path_equals_table_path(torch, src):
    """Rays that share one wavelength through the per-ray path = the per-wavelength table
    path (materials.py's formulas in host NumPy) bit for bit."""
    from optiland_pr_amd.lowering import lower_surface_group
    from optiland_pr_amd.materials import Material
    from optiland_pr_amd.raytrace import DeviceLens, RealRays, trace_rays

    g = D.golden()
    e = D.entries()[src]
    w0 = float(g[f"trace/{src}/w"][0])
    lens = D.singlet(Material.from_entry(e), w0)
    dl = DeviceLens(lower_surface_group(lens.surface_group, [w0]))
    base = [g[f"trace/{src}/in_{a}"] for a in D.RAY_IN]
    mk = lambda: RealRays(*(torch.as_tensor(v, device="cuda") for v in base), w0)  # noqa: E731
    r1, r2 = mk(), mk()
    trace_rays(dl, r1, r1)
    trace_rays(dl, r2, r2, per_ray_w=True)
    for f in ("x", "y", "z", "L", "M", "N", "opd"):
        assert torch.equal(getattr(r1, f), getattr(r2, f)), f
    assert torch.isfinite(r1.x).all()
