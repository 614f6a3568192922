"""The FFT / MMDFT PSF and the FFT MTF on the MI355X: the fused DFT kernels (ort_dft_psf, the
CUDA key of torch.ops.ort.dft_psf) against the reference's FFTPSF, MMDFTPSF and FFTMTF
(tests/golden/dft_psf.npz), against the host build and a NumPy restatement at the kernels'
tile edges, their determinism, and the three classes end to end from the sample lenses
(trace, wavefront, pupil grid, transform, normalisation, MTF).
The bounds are tests/_dft_psf.py's (derived there, relative tolerance 0).

Measured on the MI355X (max |d PSF| against the reference, PSF units, ideal peak 100):
see DESIGN.md "FFT / MMDFT PSF and MTF"."""

import numpy as np
import pytest
import torch

from tests import _dft_psf as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs the MI355X")
    return torch.device("cuda")


def _t(a, dev):
    return torch.as_tensor(np.array(a), device=dev)


def _op(amp, opd, m, pad, dev):
    return torch.ops.ort.dft_psf(_t(amp, dev), _t(opd, dev), m, pad)


@pytest.mark.parametrize("case", D.PSF_CASES)
def test_transform_against_reference(gpu, case):
    """The fixture's own pupil grids through the CUDA key: within the bound; the same call
    twice gives identical bits."""
    c, amp, opd, n, m, pad, atol = D.case_arrays(case)
    raw = _op(amp, opd, m, pad, gpu)
    assert raw.shape == (m, m) and raw.dtype == torch.float64 and raw.is_cuda
    got = raw.cpu().numpy() * 100.0 / float(c["count"]) ** 2
    print(f"{case}: device max |d PSF| = {np.max(np.abs(got - c['psf'])):.3g} "
          f"(atol {atol:.3g})")
    np.testing.assert_allclose(got, c["psf"], rtol=0, atol=atol)
    assert torch.equal(_op(amp, opd, m, pad, gpu), raw)


def test_batch_of_three_fields(gpu):
    """The MTF fixture's three pupils as one (3, n, n) call: within the bound of the
    reference's PSFs, and equal to three single calls bit for bit."""
    c, amp, opd, psf_ref, n, m, atol = D.mtf_arrays()
    assert amp.shape[0] == 3
    batch = _op(amp, opd, m, float(m), gpu)
    assert batch.shape == (3, m, m)
    counts = np.array([float(c[f"count{f}"]) for f in range(3)])
    got = batch.cpu().numpy() * 100.0 / counts[:, None, None] ** 2
    print(f"mtf_cooke: device max |d PSF| = {np.max(np.abs(got - psf_ref)):.3g} "
          f"(atol {atol:.3g})")
    np.testing.assert_allclose(got, psf_ref, rtol=0, atol=atol)
    for f in range(3):
        assert torch.equal(batch[f], _op(amp[f], opd[f], m, float(m), gpu))
    # and at sizes that end inside a tile, with a non-integer pad
    n2, m2 = 2 * D.TK + 3, D.TM + 1
    probs = [D.synthetic(n2, m2, "fractional"), D.synthetic(n2, m2, "integer")]
    pad = probs[0][2]
    amps = np.stack([probs[0][0], probs[1][0], probs[0][0]])
    opds = np.stack([probs[0][1], probs[1][1], probs[0][1]])
    batch = _op(amps, opds, m2, pad, gpu)
    for f in range(3):
        assert torch.equal(batch[f], _op(amps[f], opds[f], m2, pad, gpu))
    assert torch.equal(batch[0], batch[2])


@pytest.mark.parametrize("kind", D.PAD_KINDS)
@pytest.mark.parametrize("m", D.IMAGE_SIZES)
@pytest.mark.parametrize("n", D.PUPIL_SIZES)
def test_tile_edges(gpu, n, m, kind):
    """Pupils around one and two sum chunks, images around one and two column steps: the
    device against the host key and against the NumPy restatement (all scaled by
    100 / (sum amp)^2), within the bound."""
    amp, opd, pad, expected, scale, atol = D.synthetic(n, m, kind)
    dev = _op(amp, opd, m, pad, gpu).cpu().numpy() / scale * 100.0
    cpu = _op(amp, opd, m, pad, "cpu").numpy() / scale * 100.0
    np.testing.assert_allclose(dev, cpu, rtol=0, atol=atol)
    np.testing.assert_allclose(dev, expected / scale * 100.0, rtol=0, atol=atol)


def test_non_default_stream(gpu):
    amp, opd, pad, _, _, _ = D.synthetic(D.TK + 1, D.TM + 1, "fractional")
    ta, to = _t(amp, gpu), _t(opd, gpu)
    ref = torch.ops.ort.dft_psf(ta, to, D.TM + 1, pad)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = torch.ops.ort.dft_psf(ta, to, D.TM + 1, pad)
    s.synchronize()
    assert torch.equal(got, ref)


def test_zero_amplitude_and_empty_image(gpu):
    amp, opd, pad, _, _, _ = D.synthetic(D.TK + 1, D.TM - 1, "integer")
    out = _op(np.zeros_like(amp), opd, D.TM - 1, pad, gpu)
    assert out.shape == (D.TM - 1, D.TM - 1) and bool(torch.all(out == 0.0))
    assert _op(amp, opd, 0, pad, gpu).shape == (0, 0)
    assert _op(amp[None], opd[None], 0, pad, gpu).shape == (1, 0, 0)
    with pytest.raises(ValueError, match="n == 0"):
        _op(np.zeros((0, 0)), np.zeros((0, 0)), 4, 4.0, gpu)
    with pytest.raises(ValueError, match="pad_size"):
        _op(amp, opd, 4, 0.0, gpu)


def test_requires_grad_raises(gpu):
    amp, opd, pad, _, _, _ = D.synthetic(D.TK - 1, 1, "integer")
    ta, to = _t(amp, gpu), _t(opd, gpu)
    to.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        torch.ops.ort.dft_psf(ta, to, 1, pad)


def test_opcheck_dft_psf_cuda(gpu):
    amp, opd, pad, _, _, _ = D.synthetic(D.TK + 1, D.TM - 1, "fractional")
    for args in ((_t(amp, gpu), _t(opd, gpu), D.TM - 1, pad),
                 (_t(amp[None], gpu), _t(opd[None], gpu), D.TM - 1, pad)):
        res = torch.library.opcheck(torch.ops.ort.dft_psf.default, args)
        assert all(v == "SUCCESS" for v in res.values()), res


@pytest.mark.parametrize("case", D.PSF_CASES)
def test_psf_classes_end_to_end(gpu, case):
    """FFTPSF / MMDFTPSF from the lens: the PSF within the op's bound plus the OPD parity
    term; pixel_pitch and the working F/# to rtol 1e-12; the Strehl ratio within the bound
    / 100; shape, dtype and device."""
    import optiland_pr_amd
    from optiland_pr_amd import samples

    c, amp, opd, n, m, pad, atol = D.case_arrays(case)
    atol = atol + D.E2E_EXTRA
    cls, lens, field, wl, num_rays, kw = D.END_TO_END[case]
    p = getattr(optiland_pr_amd, cls)(getattr(samples, lens)(), field, wl, num_rays=num_rays,
                                      **kw)
    assert p.psf.shape == (m, m) and p.psf.dtype == torch.float64 and p.psf.is_cuda
    assert p.num_rays == n
    got = p.psf.cpu().numpy()
    print(f"{case}: end-to-end max |d PSF| = {np.max(np.abs(got - c['psf'])):.3g} "
          f"(atol {atol:.3g})")
    fno = float(p._get_working_FNO())
    np.testing.assert_allclose(fno, float(c["working_fno"]), rtol=1e-12, atol=0)
    if cls == "FFTPSF":
        assert p.grid_size == m
        pitch = wl * fno / (m / (n - 1))
        pupil = p.pupils[0]
    else:
        assert p.image_size == m
        pitch = float(p.pixel_pitch)
        pupil = p.pupil
    np.testing.assert_allclose(pitch, float(c["pixel_pitch"]), rtol=1e-12, atol=0)
    assert pupil.shape == (n, n) and pupil.dtype == torch.complex128 and pupil.is_cuda
    np.testing.assert_allclose(got, c["psf"], rtol=0, atol=atol)
    np.testing.assert_allclose(p.strehl_ratio(), float(c["strehl"]), rtol=0, atol=atol / 100)


def test_fftmtf_end_to_end(gpu):
    """FFTMTF(CookeTriplet(), num_rays=32): every field's PSF within the end-to-end bound,
    freq and max_freq to rtol 1e-12, both curves within the bound derived from the PSF's."""
    from optiland_pr_amd import FFTMTF, samples

    c, amp, opd, psf_ref, n, m, atol = D.mtf_arrays()
    atol = atol + D.E2E_EXTRA
    mt = FFTMTF(samples.CookeTriplet(), num_rays=D.MTF_NUM_RAYS)
    nf = psf_ref.shape[0]
    assert (mt.num_rays, mt.grid_size) == (n, m) and len(mt.psf) == len(mt.mtf) == nf
    np.testing.assert_allclose(float(mt.FNO), float(c["working_fno"]), rtol=1e-12, atol=0)
    np.testing.assert_allclose(float(mt.max_freq), float(c["max_freq"]), rtol=1e-12, atol=0)
    assert mt.freq.shape == (m // 2,) and mt.freq.is_cuda and mt.freq.dtype == torch.float64
    np.testing.assert_allclose(mt.freq.cpu().numpy(), c["freq"], rtol=1e-12, atol=0)
    for k in range(nf):
        assert mt.psf[k].shape == (m, m) and mt.psf[k].is_cuda
        got = mt.psf[k].cpu().numpy()
        print(f"field {k}: end-to-end max |d PSF| = {np.max(np.abs(got - psf_ref[k])):.3g} "
              f"(atol {atol:.3g})")
        np.testing.assert_allclose(got, psf_ref[k], rtol=0, atol=atol)
        tol = D.mtf_bound(atol, psf_ref[k])
        for curve, name in zip(mt.mtf[k], ("tangential", "sagittal"), strict=True):
            want = c[f"{name}{k}"]
            assert curve.shape == (m - m // 2,) and curve.is_cuda
            print(f"field {k} {name}: max |d MTF| = "
                  f"{np.max(np.abs(curve.cpu().numpy() - want)):.3g} (atol {tol:.3g})")
            np.testing.assert_allclose(curve.cpu().numpy(), want, rtol=0, atol=tol)
