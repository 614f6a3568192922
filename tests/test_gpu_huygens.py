"""The Huygens-Fresnel PSF on the MI355X: the fused summation kernel (ort_huygens_psf, the
CUDA key of torch.ops.ort.huygens_psf) against the reference's HuygensPSF
(tests/golden/huygens.npz) and against the host build at the chunk and tile edges, its
determinism, and HuygensPSF end to end (trace, wavefront, image grid, sum, normalisation).
The bound is tests/_huygens.py's (derived there, relative tolerance 0).

Measured on the MI355X (max |d PSF| against the reference, PSF units, ideal peak 100):
see DESIGN.md "Huygens-Fresnel PSF"."""

import numpy as np
import pytest
import torch

from tests import _huygens as H

pytestmark = pytest.mark.gpu

END_TO_END = {  # tests/golden/gen_huygens_golden.py CASES, with this package's lenses
    "cooke_00": ("CookeTriplet", (0, 0), 0.55, 16, 15, {}),
    "cooke_01": ("CookeTriplet", (0, 1), 0.55, 16, 16, {}),
    "dg_007": ("DoubleGauss", (0, 0.7), 0.5876, 20, 16, {}),
    "cooke_pitch": ("CookeTriplet", (0, 0.7), 0.48, 16, 9,
                    {"pixel_pitch": 0.001, "remove_tilt": True}),
    "cooke_oversample": ("CookeTriplet", (0, 0), 0.55, 16, 8, {"oversample": 2.0}),
}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs the MI355X")
    return torch.device("cuda")


def _t(arrays, dev):
    return [torch.as_tensor(np.array(a), device=dev) for a in arrays]


@pytest.mark.parametrize("case", H.CASES)
def test_summation_against_reference(gpu, case):
    """The fixture's own image grid and pupil through the CUDA key: within the bound; the
    same call twice and the image as one (N,) tensor give identical bits."""
    c, image, pupil, atol = H.case_arrays(case)
    wl, rp = float(c["wavelength_mm"]), float(c["radius"])
    ti, tp = _t(image, gpu), _t(pupil, gpu)
    raw = torch.ops.ort.huygens_psf(*ti, *tp, wl, rp)
    assert raw.shape == c["psf"].shape and raw.dtype == torch.float64 and raw.is_cuda
    got = raw.cpu().numpy() / float(c["norm"]) * 100.0
    print(f"{case}: device max |d PSF| = {np.max(np.abs(got - c['psf'])):.3g} "
          f"(atol {atol:.3g})")
    np.testing.assert_allclose(got, c["psf"], rtol=0, atol=atol)
    assert torch.equal(torch.ops.ort.huygens_psf(*ti, *tp, wl, rp), raw)
    flat = torch.ops.ort.huygens_psf(*(t.reshape(-1) for t in ti), *tp, wl, rp)
    assert flat.shape == (raw.numel(),) and torch.equal(flat, raw.reshape(-1))


@pytest.mark.parametrize("n_pupil", H.PUPIL_SIZES)
@pytest.mark.parametrize("n_image", H.IMAGE_SIZES)
def test_chunk_and_tile_edges(gpu, n_image, n_pupil):
    """Pupils around one and two chunks, image sizes around one wave: the device against the
    host key (both sides scaled by the ideal-norm bound to a peak of 100) and against the
    NumPy restatement, within the bound."""
    image, pupil, expected, scale, atol = H.synthetic(n_image, n_pupil)
    dev = torch.ops.ort.huygens_psf(*_t(image, gpu), *_t(pupil, gpu), H.WAVELENGTH_MM, H.RP)
    cpu = torch.ops.ort.huygens_psf(*_t(image, "cpu"), *_t(pupil, "cpu"), H.WAVELENGTH_MM, H.RP)
    got = dev.cpu().numpy() / scale * 100.0
    np.testing.assert_allclose(got, cpu.numpy() / scale * 100.0, rtol=0, atol=atol)
    np.testing.assert_allclose(got, expected / scale * 100.0, rtol=0, atol=atol)


def test_image_tiling_does_not_change_bits(gpu):
    """300 image points (two tiles, the second partial) over a three-chunk pupil: as one
    row, as a 20 x 15 grid, and as its first 65 points alone -- the same bits per point."""
    image, pupil, _, _, _ = H.synthetic(300, 2 * H.CHUNK + 3)
    ti, tp = _t(image, gpu), _t(pupil, gpu)
    flat = torch.ops.ort.huygens_psf(*ti, *tp, H.WAVELENGTH_MM, H.RP)
    grid = torch.ops.ort.huygens_psf(*(t.reshape(20, 15) for t in ti), *tp, H.WAVELENGTH_MM,
                                     H.RP)
    head = torch.ops.ort.huygens_psf(*(t[:65].clone() for t in ti), *tp, H.WAVELENGTH_MM, H.RP)
    assert torch.equal(grid.reshape(-1), flat)
    assert torch.equal(head, flat[:65])


def test_empty_pupil_and_empty_image(gpu):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=gpu)  # noqa: E731
    out = torch.ops.ort.huygens_psf(z(3, 2), z(3, 2), z(3, 2), z(0), z(0), z(0), z(0), z(0),
                                    H.WAVELENGTH_MM, H.RP)
    assert out.shape == (3, 2) and bool(torch.all(out == 0.0))
    out = torch.ops.ort.huygens_psf(z(0), z(0), z(0), z(5), z(5), z(5), z(5), z(5),
                                    H.WAVELENGTH_MM, H.RP)
    assert out.shape == (0,)


def test_non_default_stream(gpu):
    c, image, pupil, _ = H.case_arrays("dg_007")
    wl, rp = float(c["wavelength_mm"]), float(c["radius"])
    ti, tp = _t(image, gpu), _t(pupil, gpu)
    ref = torch.ops.ort.huygens_psf(*ti, *tp, wl, rp)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = torch.ops.ort.huygens_psf(*ti, *tp, wl, rp)
    s.synchronize()
    assert torch.equal(got, ref)


def test_requires_grad_raises(gpu):
    image, pupil, _, _, _ = H.synthetic(1, H.CHUNK - 1)
    args = _t(image, gpu) + _t(pupil, gpu)
    args[7].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        torch.ops.ort.huygens_psf(*args, H.WAVELENGTH_MM, H.RP)


def test_opcheck_huygens_psf_cuda(gpu):
    c, image, pupil, _ = H.case_arrays("cooke_00")
    args = (*_t(image, gpu), *_t(pupil, gpu), float(c["wavelength_mm"]), float(c["radius"]))
    res = torch.library.opcheck(torch.ops.ort.huygens_psf.default, args)
    assert all(v == "SUCCESS" for v in res.values()), res


@pytest.mark.parametrize("case", H.CASES)
def test_huygens_psf_end_to_end(gpu, case):
    """HuygensPSF(...) from the lens: the PSF within the bound; the grid's pitch and centre
    to rtol 1e-12 (atol 1e-15 for the centres); the working F/# to rtol 1e-12; the Strehl
    ratio within atol / 100; shape, dtype and device."""
    from optiland_pr_amd import HuygensPSF, samples

    c, _, _, atol = H.case_arrays(case)
    lens, field, wl, num_rays, image_size, kw = END_TO_END[case]
    p = HuygensPSF(getattr(samples, lens)(), field, wl, num_rays=num_rays,
                   image_size=image_size, **kw)
    assert p.psf.shape == (image_size, image_size) and p.image_size == image_size
    assert p.psf.dtype == torch.float64 and p.psf.is_cuda
    got = p.psf.cpu().numpy()
    print(f"{case}: end-to-end max |d PSF| = {np.max(np.abs(got - c['psf'])):.3g} "
          f"(atol {atol:.3g}), pitch {float(p.pixel_pitch)!r} vs {float(c['pixel_pitch'])!r}")
    np.testing.assert_allclose(float(p.pixel_pitch), float(c["pixel_pitch"]), rtol=1e-12, atol=0)
    np.testing.assert_allclose(float(p.cx), float(c["cx"]), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(float(p.cy), float(c["cy"]), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(float(p._get_working_FNO()), float(c["working_fno"]),
                               rtol=1e-12, atol=0)
    np.testing.assert_allclose(got, c["psf"], rtol=0, atol=atol)
    np.testing.assert_allclose(p.strehl_ratio(), float(c["strehl"]), rtol=0, atol=atol / 100)
