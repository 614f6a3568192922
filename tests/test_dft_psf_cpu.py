"""The FFT / MMDFT PSF transform and the FFT MTF without a GPU: the host build of the kernels'
terms (ort_host_dft_psf, csrc/ort_dft.h) behind the CPU key of torch.ops.ort.dft_psf against
the reference's FFTPSF, MMDFTPSF and FFTMTF (tests/golden/dft_psf.npz), against numpy's fft2
of the padded pupil, and at the kernels' tile edges against a NumPy restatement; the classes
from the wavefront data onward on host tensors; argument checks; the ABI constants.
The bounds are tests/_dft_psf.py's (derived there, relative tolerance 0).

The package traces on the device only, so "end to end" here starts from the fixture's
wavefront data (the rays' intensity and OPD the reference's Wavefront produced) and the
fixture's working F/#: pupil grid, pad size resolution, transform, normalisation, Strehl
ratio, MTF. From the lens itself: tests/test_gpu_dft_psf.py."""

import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import optiland_pr_amd
from optiland_pr_amd import _abi, _native, mtf, psf
from tests import _dft_psf as D
from tests.conftest import REPO


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy())


def _op(amp, opd, m, pad):
    return torch.ops.ort.dft_psf(_t(amp), _t(opd), m, pad)


@pytest.mark.parametrize("case", D.PSF_CASES)
def test_fixture_cases_cpu_key(case):
    """raw * 100 / count^2 against the reference's psf, within the bound."""
    c, amp, opd, n, m, pad, atol = D.case_arrays(case)
    raw = _op(amp, opd, m, pad)
    assert raw.shape == (m, m) and raw.dtype == torch.float64
    got = raw.numpy() * 100.0 / float(c["count"]) ** 2
    print(f"{case}: host max |d PSF| = {np.max(np.abs(got - c['psf'])):.3g} (atol {atol:.3g})")
    np.testing.assert_allclose(got, c["psf"], rtol=0, atol=atol)


def test_mtf_fixture_fields_as_one_batch():
    c, amp, opd, psf_ref, n, m, atol = D.mtf_arrays()
    raw = _op(amp, opd, m, float(m))
    assert raw.shape == psf_ref.shape
    counts = np.array([float(c[f"count{f}"]) for f in range(amp.shape[0])])
    got = raw.numpy() * 100.0 / counts[:, None, None] ** 2
    np.testing.assert_allclose(got, psf_ref, rtol=0, atol=atol)


@pytest.mark.parametrize("case", D.PSF_CASES + (D.MTF_CASE,))
def test_reference_noise_floor(case):
    """The reference alone (its PSF against a second computation, measured by the generator)
    sits a factor 100 inside the bound."""
    if case == D.MTF_CASE:
        c, _, _, _, _, _, atol = D.mtf_arrays()
    else:
        c, _, _, _, _, _, atol = D.case_arrays(case)
    assert float(c["ref_self_diff"]) < atol / 100


@pytest.mark.parametrize("case", [k for k in D.PSF_CASES if k != "mmdft_cooke_007"])
def test_integer_pad_against_fft2(case):
    c, amp, opd, n, m, pad, atol = D.case_arrays(case)
    assert pad == m
    scale = 100.0 / float(c["count"]) ** 2
    np.testing.assert_allclose(_op(amp, opd, m, pad).numpy() * scale,
                               D.padded_fft(amp, opd, m) * scale, rtol=0, atol=atol)


@pytest.mark.parametrize("kind", D.PAD_KINDS)
@pytest.mark.parametrize("m", D.IMAGE_SIZES)
@pytest.mark.parametrize("n", D.PUPIL_SIZES)
def test_tile_edges_cpu(n, m, kind):
    """Pupils and images around one and two tiles against the NumPy restatement, both sides
    scaled by 100 / (sum amp)^2."""
    amp, opd, pad, expected, scale, atol = D.synthetic(n, m, kind)
    got = _op(amp, opd, m, pad).numpy()
    assert np.all(np.isfinite(got)) and np.max(expected) / scale <= 1.0
    np.testing.assert_allclose(got / scale * 100.0, expected / scale * 100.0, rtol=0, atol=atol)


def test_batch_equals_single_calls_bit_for_bit():
    c, amp, opd, _, n, m, _ = D.mtf_arrays()
    batch = _op(amp, opd, m, float(m))
    for f in range(amp.shape[0]):
        assert torch.equal(batch[f], _op(amp[f], opd[f], m, float(m)))
    assert torch.equal(batch, _op(amp, opd, m, float(m)))
    amp2, opd2, pad, _, _, _ = D.synthetic(D.TK + 1, D.TM + 1, "fractional")
    pair = _op(np.stack([amp2, amp2]), np.stack([opd2, opd2]), D.TM + 1, pad)
    assert torch.equal(pair[0], pair[1]) and torch.equal(pair[0], _op(amp2, opd2, D.TM + 1, pad))


def test_zero_amplitude_and_non_finite_inputs():
    amp, opd, pad, _, _, _ = D.synthetic(D.TK + 1, 9, "fractional")
    zero = _op(np.zeros_like(amp), opd, 9, pad)
    assert zero.shape == (9, 9) and bool(torch.all(zero == 0.0))
    # amp == 0 with a finite opd contributes exactly 0: its opd does not matter
    other = np.where(amp == 0.0, 17.25, opd)
    assert np.count_nonzero(amp == 0.0) > 0
    assert torch.equal(_op(amp, opd, 9, pad), _op(amp, other, 9, pad))
    for bad_amp, bad_opd in ((np.nan, 0.5), (1.0, np.nan), (1.0, np.inf), (0.0, np.nan)):
        a, o = amp.copy(), opd.copy()
        a[3, 4], o[3, 4] = bad_amp, bad_opd
        assert bool(torch.all(torch.isnan(_op(a, o, 9, pad))))


def test_shapes_and_argument_errors():
    amp, opd, pad, _, _, _ = D.synthetic(D.TK - 1, 5, "integer")
    assert _op(amp, opd, 0, 3.0).shape == (0, 0)
    assert _op(amp[None], opd[None], 0, 3.0).shape == (1, 0, 0)
    assert _op(amp[None], opd[None], 5, pad).shape == (1, 5, 5)
    assert _op(np.zeros((0, *amp.shape)), np.zeros((0, *amp.shape)), 5, pad).shape == (0, 5, 5)
    with pytest.raises(ValueError, match="n == 0"):
        _op(np.zeros((0, 0)), np.zeros((0, 0)), 5, 5.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="pad_size"):
            _op(amp, opd, 5, bad)
    with pytest.raises(ValueError, match="float64"):
        torch.ops.ort.dft_psf(_t(amp).float(), _t(opd), 5, pad)
    with pytest.raises(ValueError, match=r"\(n, n\) or \(B, n, n\)"):
        torch.ops.ort.dft_psf(_t(amp)[:, :-1].contiguous(), _t(opd)[:, :-1].contiguous(), 5, pad)
    with pytest.raises(ValueError, match="contiguous"):
        torch.ops.ort.dft_psf(_t(amp).T, _t(opd).T, 5, pad)
    with pytest.raises(ValueError, match="image_size"):
        _op(amp, opd, _abi.DFT_MAX_SIZE + 1, pad)


def test_requires_grad_raises():
    amp, opd, pad, _, _, _ = D.synthetic(D.TK - 1, 5, "integer")
    for k in (0, 1):
        args = [_t(amp), _t(opd)]
        args[k].requires_grad_(True)
        with pytest.raises(NotImplementedError, match="not differentiable"):
            torch.ops.ort.dft_psf(*args, 5, pad)
    with torch.no_grad():
        assert torch.ops.ort.dft_psf(*args, 5, pad).shape == (5, 5)


def test_opcheck_dft_psf_cpu():
    amp, opd, pad, _, _, _ = D.synthetic(D.TK + 1, 9, "fractional")
    for args in ((_t(amp), _t(opd), 9, pad), (_t(amp)[None], _t(opd)[None], 9, pad)):
        res = torch.library.opcheck(torch.ops.ort.dft_psf.default, args)
        assert all(v == "SUCCESS" for v in res.values()), res


def _dp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_host_entry_argument_errors():
    lib = _native.load_host()
    err = -1  # ORT_ERR_ARG
    a = np.full((2, 4, 4), 0.5)
    out = np.full((2, 3, 3), -1.0)
    null = ctypes.c_void_p(0)

    def call(batch=2, n=4, m=3, pad=3.0, amp=_dp(a), opd=_dp(a), o=_dp(out)):
        return lib.ort_host_dft_psf(amp, opd, batch, n, m, pad, o)

    assert call(batch=-1) == err and call(n=0) == err and call(m=-1) == err
    assert call(n=_abi.DFT_MAX_SIZE + 1) == err and call(m=_abi.DFT_MAX_SIZE + 1) == err
    for bad in (0.0, -3.0, float("nan"), float("inf")):
        assert call(pad=bad) == err
    assert call(amp=null) == err and call(opd=null) == err and call(o=null) == err
    assert np.all(out == -1.0)
    assert call(batch=0, amp=null, opd=null, o=null) == 0
    assert call(m=0, o=null) == 0 and np.all(out == -1.0)
    assert call() == 0 and np.all(out >= 0.0)


def test_device_entry_argument_errors():
    """ort_dft_workspace_size and the checks ort_dft_psf makes before any launch (no GPU is
    touched: every call returns at its argument check)."""
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("HIP extension not built (run __graft_entry__.build())")
    lib = _native.load()
    err = -1
    assert lib.ort_dft_workspace_size(3, 4, 5) == 3 * 4 * 5 * 16
    assert lib.ort_dft_workspace_size(0, 4, 5) == 0 and lib.ort_dft_workspace_size(3, 4, 0) == 0
    assert lib.ort_dft_workspace_size(-1, 4, 5) == err
    assert lib.ort_dft_workspace_size(1, 0, 5) == err
    assert lib.ort_dft_workspace_size(1, 4, _abi.DFT_MAX_SIZE + 1) == err
    assert lib.ort_dft_workspace_size(2**40, 4, 5) == err
    a = np.zeros(64)
    p, null = _dp(a), ctypes.c_void_p(0)

    def call(batch=1, n=2, m=2, pad=2.0, amp=p, out=p, ws=p, ws_size=64):
        return lib.ort_dft_psf(amp, p, batch, n, m, pad, out, ws, ws_size, None)

    assert call(batch=-1) == err and call(n=0) == err and call(m=-1) == err
    assert call(pad=0.0) == err and call(pad=float("nan")) == err
    assert call(amp=null) == err and call(out=null) == err
    assert call(ws_size=63) == err and call(ws=null) == err
    assert call(batch=0, ws=null, ws_size=0) == 0 and call(m=0, ws=null, ws_size=0) == 0


def test_abi_constants_match_headers():
    rt = open(os.path.join(REPO, "include", "optiland_rt.h")).read()
    hh = open(os.path.join(REPO, "include", "optiland_host.h")).read()
    for name, value in (("ORT_DFT_TILE_M", _abi.DFT_TILE_M), ("ORT_DFT_TILE_K", _abi.DFT_TILE_K),
                        ("ORT_DFT_MAX_SIZE", _abi.DFT_MAX_SIZE)):
        assert int(re.search(rf"#define {name} (\d+)", rt).group(1)) == value
    assert int(re.search(r"#define ORT_ABI_VERSION (\d+)", rt).group(1)) == _abi.ABI_VERSION == 21
    assert (int(re.search(r"#define ORT_HOST_ABI_VERSION (\d+)", hh).group(1))
            == _native.HOST_ABI_VERSION == 3)
    assert _native.load_host().ort_host_abi_version() == 3
    assert "ort_dft_psf" in _native.EXPORTS and "ort_dft_workspace_size" in _native.EXPORTS
    assert "ort_host_dft_psf" in _native.HOST_EXPORTS
    assert re.search(r"int ort_dft_psf\(const double\* amp, const double\* opd_waves, int64_t "
                     r"batch, int64_t n, int64_t m,\s+double pad, double\* out, void\* workspace, "
                     r"int64_t workspace_size, void\* stream\);", rt)
    assert len(_native.DEVICE_PROTOTYPES["ort_dft_psf"][1]) == 10
    assert re.search(r"int ort_host_dft_psf\(const double\* amp, const double\* opd_waves, "
                     r"int64_t batch, int64_t n,\s+int64_t m, double pad, double\* out\);", hh)
    assert len(_native.HOST_PROTOTYPES["ort_host_dft_psf"][1]) == 7


def test_calculate_grid_size():
    table = D.fixture()["grid_size"]["table"]
    assert [int(r[0]) for r in table] == [32, 64, 100, 128, 1024]
    for rays, eff, grid in table:
        got = psf.calculate_grid_size(int(rays))
        assert (int(got[0]), int(got[1])) == (int(eff), int(grid))


def test_class_value_errors_carry_the_reference_texts():
    with pytest.raises(ValueError) as e:
        optiland_pr_amd.FFTPSF(None, (0, 0), 0.55, num_rays=31)
    assert str(e.value) == "num_rays must be at least 32 if grid_size is not specified."
    with pytest.raises(ValueError) as e:
        optiland_pr_amd.FFTPSF(None, (0, 0), 0.55, num_rays=40, grid_size=39)
    assert str(e.value) == ("Grid size (39) must be greater than or equal to the number of "
                            "rays (40).")
    with pytest.raises(ValueError) as e:
        optiland_pr_amd.MMDFTPSF(None, (0, 0), 0.55, num_rays=31)
    assert str(e.value) == ("num_rays must be at least 32 if image_size and pixel_pitch are "
                            "not specified.")
    with pytest.raises(ValueError) as e:
        optiland_pr_amd.FFTMTF(None, num_rays=40, grid_size=39)
    assert str(e.value) == ("Grid size (39) must be greater than or equal to the number of "
                            "rays (40).")


# -- the classes from the wavefront data onward, on host tensors ------------------------
def _rays_of(amp, opd):
    """The per-ray arrays a uniform-distribution Wavefront holds for these pupil grids (a
    common factor on the intensity: the classes divide by the mean)."""
    n = amp.shape[0]
    x = np.linspace(-1, 1, n)
    x, y = np.meshgrid(x, x)
    inside = (x * x + y * y) <= 1
    return types.SimpleNamespace(intensity=_t(amp[inside] * 0.75), opd=_t(opd[inside]))


@pytest.fixture
def host_wavefront(monkeypatch):
    """Wavefront without a trace: get_data returns the installed rays; the working F/# is the
    fixture's."""
    state = {"patch": monkeypatch}

    def init(self, optic, fields="all", wavelengths="all", num_rays=12, **kwargs):
        self.optic, self.fields, self.wavelengths = optic, fields, wavelengths
        self.num_rays = num_rays
        state["kwargs"] = kwargs

    monkeypatch.setattr(psf.Wavefront, "__init__", init)
    monkeypatch.setattr(psf.Wavefront, "get_data",
                        lambda self, field, wl: state["data"][tuple(field)])
    monkeypatch.setattr(psf, "get_working_FNO", lambda *a: state["fno"])
    monkeypatch.setattr(mtf, "get_working_FNO", lambda *a: state["fno"])
    return state


@pytest.mark.parametrize("case", D.PSF_CASES)
def test_classes_from_wavefront_data(host_wavefront, case):
    c, amp, opd, n, m, pad, atol = D.case_arrays(case)
    cls, _, field, wl, num_rays, kw = D.END_TO_END[case]
    host_wavefront["data"] = {tuple(field): _rays_of(amp, opd)}
    host_wavefront["fno"] = float(c["working_fno"])
    p = getattr(optiland_pr_amd, cls)(None, field, wl, num_rays=num_rays, **kw)
    assert host_wavefront["kwargs"]["distribution"] == "uniform" and p.num_rays == n
    assert p.psf.shape == (m, m) and p.psf.dtype == torch.float64
    np.testing.assert_allclose(p.psf.numpy(), c["psf"], rtol=0, atol=atol)
    np.testing.assert_allclose(p.strehl_ratio(), float(c["strehl"]), rtol=0, atol=atol / 100)
    pupil = p.pupils[0] if cls == "FFTPSF" else p.pupil
    assert pupil.shape == (n, n) and pupil.dtype == torch.complex128
    np.testing.assert_allclose(pupil.numpy(), amp * np.exp(-2j * np.pi * opd), rtol=0,
                               atol=1e-13)
    if cls == "FFTPSF":
        assert p.grid_size == m
    else:
        assert p.image_size == m
        np.testing.assert_allclose(p.pixel_pitch, float(c["pixel_pitch"]), rtol=1e-12, atol=0)
        np.testing.assert_allclose(p.pad_size, pad, rtol=1e-12, atol=0)


def test_mmdft_image_size_above_pad_size_raises(host_wavefront):
    c, amp, opd, n, m, pad, _ = D.case_arrays("mmdft_cooke_007")
    host_wavefront["data"] = {(0, 0.7): _rays_of(amp, opd)}
    host_wavefront["fno"] = float(c["working_fno"])
    with pytest.raises(ValueError) as e:
        optiland_pr_amd.MMDFTPSF(None, (0, 0.7), 0.48, num_rays=20, image_size=40,
                                 pixel_pitch=1.3)
    assert str(e.value) == ("Supplied image_size of 40 not less than or equal to calculated pad "
                            "size of 36. Consider increasing num_rays.")
    # image_size from the pixel pitch alone: one pixel inside the pad size
    p = optiland_pr_amd.MMDFTPSF(None, (0, 0.7), 0.48, num_rays=20, pixel_pitch=1.3)
    assert p.image_size == 36 and p.psf.shape == (36, 36)


def test_fftmtf_from_wavefront_data(host_wavefront):
    c, amp, opd, psf_ref, n, m, atol = D.mtf_arrays()
    fields = [tuple(f) for f in c["fields"]]
    host_wavefront["data"] = {f: _rays_of(amp[k], opd[k]) for k, f in enumerate(fields)}
    host_wavefront["fno"] = float(c["working_fno"])
    optic = types.SimpleNamespace(
        fields=types.SimpleNamespace(get_field_coords=lambda: [tuple(f) for f in c["fields"]]),
        primary_wavelength=float(c["wavelength"]))
    calls = []

    def counting(amp_t, *args):
        calls.append(tuple(amp_t.shape))
        return psf.normalized_dft_psf(amp_t, *args)

    host_wavefront["patch"].setattr(mtf, "normalized_dft_psf", counting)
    mt = optiland_pr_amd.FFTMTF(optic, num_rays=D.MTF_NUM_RAYS)
    assert calls == [(len(fields), n, n)]  # every field in one batched transform
    assert (mt.num_rays, mt.grid_size) == (n, m) and len(mt.psf) == len(mt.mtf) == len(fields)
    np.testing.assert_allclose(mt.FNO, float(c["working_fno"]), rtol=0, atol=0)
    np.testing.assert_allclose(mt.max_freq, float(c["max_freq"]), rtol=1e-12, atol=0)
    assert mt.freq.shape == (m // 2,)
    np.testing.assert_allclose(mt.freq.numpy(), c["freq"], rtol=1e-12, atol=0)
    for k in range(len(fields)):
        np.testing.assert_allclose(mt.psf[k].numpy(), psf_ref[k], rtol=0, atol=atol)
        tol = D.mtf_bound(atol, psf_ref[k])
        for got, name in zip(mt.mtf[k], ("tangential", "sagittal"), strict=True):
            want = c[f"{name}{k}"]
            assert got.shape == (m - m // 2,) == want.shape
            print(f"field {k} {name}: max |d MTF| = "
                  f"{np.max(np.abs(got.numpy() - want)):.3g} (atol {tol:.3g})")
            np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=tol)


def test_public_exports():
    assert optiland_pr_amd.FFTPSF is psf.FFTPSF and optiland_pr_amd.MMDFTPSF is psf.MMDFTPSF
    assert optiland_pr_amd.FFTMTF is mtf.FFTMTF
    assert {"FFTPSF", "MMDFTPSF", "FFTMTF"} <= set(optiland_pr_amd.__all__)
