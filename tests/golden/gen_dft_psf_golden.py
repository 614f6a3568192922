"""FFT / MMDFT PSF and FFT MTF golden vectors: the REFERENCE's FFTPSF (optiland/psf/fft.py),
MMDFTPSF (optiland/psf/mmdft.py) and FFTMTF (optiland/mtf/fft.py) with the NumPy backend on
small pupils and images of the sample lenses.

Test infrastructure only, run in the build container (never on the GPU box):

    PYTHONPATH=tests/golden/shims:/root/reference PYTHONDONTWRITEBYTECODE=1 \
        python tests/golden/gen_dft_psf_golden.py

Writes tests/golden/dft_psf.npz, arrays "<case>/<name>". Per PSF case: the real pupil grids
the reference transformed (amp = |pupil|, opd in waves, both [n, n]; outside the aperture
both are 0), n, m, pad_size, the normalisation count, the reference's psf, strehl,
pixel_pitch (MMDFT: um; FFT: the lambda FNO / Q of its _get_psf_units) and working_fno, and
ref_self_diff: the largest difference between the reference's psf and the same transform
recomputed here a second way -- the explicit double sum over the pupil with every phase
reduced to a fraction of a cycle before the exponential (the FFT cases and the non-integer
MMDFT case), or numpy.fft.fft2 of the zero-padded pupil (the integer-pad MMDFT case) -- the
reference's own floating-point noise floor, asserted to sit a factor 100 inside the tests'
bound (tests/_dft_psf.py, restated in bound() below). The MTF case stores per field the
pupil grids and the psf, and freq, max_freq, working_fno and both curves per field. Every
case's pupil is asserted to have all rays valid. calculate_grid_size is recorded for 32, 64,
100, 128 and 1024 rays.
"""

from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

import optiland.backend as be  # noqa: E402
from optiland.mtf import FFTMTF  # noqa: E402
from optiland.psf import FFTPSF, MMDFTPSF  # noqa: E402
from optiland.psf.fft import calculate_grid_size  # noqa: E402
from optiland.samples.objectives import CookeTriplet, DoubleGauss  # noqa: E402

be.set_backend("numpy")

# name -> (class, lens builder, field, wavelength um, num_rays, keywords)
PSF_CASES = {
    "fft_cooke_00": (FFTPSF, CookeTriplet, (0, 0), 0.55, 16, {"grid_size": 32}),
    "fft_cooke_01": (FFTPSF, CookeTriplet, (0, 1), 0.55, 32, {}),
    "fft_dg_007": (FFTPSF, DoubleGauss, (0, 0.7), 0.5876, 21, {"grid_size": 33}),
    "mmdft_cooke_007": (MMDFTPSF, CookeTriplet, (0, 0.7), 0.48, 20,
                        {"image_size": 24, "pixel_pitch": 1.3, "remove_tilt": True}),
    "mmdft_dg_00": (MMDFTPSF, DoubleGauss, (0, 0), 0.5876, 32, {}),
}
MTF_NUM_RAYS = 32
GRID_SIZE_RAYS = (32, 64, 100, 128, 1024)


def bound(n, m, pad, opd):
    """tests/_dft_psf.py bound(), restated (PSF units, ideal peak 100)."""
    phi_max = 2.0 * np.pi * ((n / 2.0) * (m / 2.0) / pad + float(np.max(np.abs(opd))))
    return 200.0 * (8.0 * phi_max + 4.0 * n + 80.0) * 2.0 ** -53


def double_sum(amp, opd, m, pad):
    """|sum_jk amp exp(-2 pi i opd) exp(-2 pi i ((v - m//2)(j - n//2) + (u - m//2)(k - n//2)) /
    pad)|^2 with each phase reduced to a fraction of a cycle first, summed by numpy's matmul."""
    n = amp.shape[0]
    g = amp * np.exp(-2j * np.pi * (opd - np.rint(opd)))
    t = np.outer(np.arange(m) - m // 2, np.arange(n) - n // 2) / pad
    w = np.exp(-2j * np.pi * (t - np.rint(t)))  # [m, n]
    field = w @ g @ w.T
    return field.real ** 2 + field.imag ** 2


def padded_fft(amp, opd, m):
    """psf/fft.py:199-234 on the same pupil: |fftshift(fft2(zero-padded pupil))|^2."""
    n = amp.shape[0]
    g = amp * np.exp(-2j * np.pi * opd)
    before = (m - n) // 2
    after = before + (m - n) % 2
    padded = np.pad(g, ((before, after), (before, after)))
    field = np.fft.fftshift(np.fft.fft2(padded))
    return field.real ** 2 + field.imag ** 2


def pupil_grids(p, n):
    """The amplitude and OPD the reference's pupil was built from (psf/fft.py:140-164)."""
    d = p.get_data(p.fields[0], p.wavelengths[0])
    inten = np.asarray(d.intensity, dtype=np.float64)
    assert np.all(inten > 0), "vignetted pupil points"
    x = np.linspace(-1, 1, n)
    x, y = np.meshgrid(x, x)
    inside = (x.ravel() ** 2 + y.ravel() ** 2) <= 1
    amp = np.zeros(n * n)
    opd = np.zeros(n * n)
    amp[inside] = inten / np.mean(inten[inten > 0])
    opd[inside] = np.asarray(d.opd, dtype=np.float64)
    return amp.reshape(n, n), opd.reshape(n, n)


def psf_case(key, cls, builder, field, wl, num_rays, kw):
    p = cls(builder(), field, wl, num_rays=num_rays, **kw)
    n = int(p.num_rays)
    amp, opd = pupil_grids(p, n)
    pupil = np.asarray(p.pupils[0] if cls is FFTPSF else p.pupil)
    # the grids restate the reference's pupil exactly
    assert np.array_equal(amp * np.exp(-1j * 2 * np.pi * opd), pupil), key
    fno = float(p._get_working_FNO())
    if cls is FFTPSF:
        m = int(p.grid_size)
        pad = float(m)
        pitch = wl * fno / (m / (n - 1))
    else:
        m = int(p.image_size)
        pad = float(wl * fno * (n - 1) / p.pixel_pitch)
        pitch = float(p.pixel_pitch)
    count = int(np.sum(np.abs(pupil) > 0))
    psf = np.asarray(p.psf, dtype=np.float64)
    assert psf.shape == (m, m), (key, psf.shape)
    integer_pad = pad == np.rint(pad)
    if cls is MMDFTPSF and integer_pad:
        assert m == pad, key
        again = padded_fft(amp, opd, m)
    else:
        again = double_sum(amp, opd, m, pad)
    self_diff = float(np.max(np.abs(again / count ** 2 * 100.0 - psf)))
    atol = bound(n, m, pad, opd)
    assert self_diff < atol / 100.0, (key, self_diff, atol)
    print(f"{key}: n {n}, m {m}, pad {pad!r}, count {count}, strehl "
          f"{float(p.strehl_ratio()):.6f}, self diff {self_diff:.3g}, atol {atol:.3g}")
    return dict(amp=amp, opd=opd, n=n, m=m, pad_size=pad, count=count, psf=psf,
                strehl=float(p.strehl_ratio()), pixel_pitch=pitch, working_fno=fno,
                ref_self_diff=self_diff)


def mtf_case():
    lens = CookeTriplet()
    mt = FFTMTF(lens, num_rays=MTF_NUM_RAYS)
    n, m = int(mt.num_rays), int(mt.grid_size)
    out = dict(n=n, m=m, pad_size=float(m), freq=np.asarray(mt.freq, dtype=np.float64),
               max_freq=float(mt.max_freq), working_fno=float(mt.FNO),
               wavelength=float(mt.resolved_wavelength),
               n_fields=len(mt.resolved_fields),
               fields=np.asarray(mt.resolved_fields, dtype=np.float64))
    worst = 0.0
    for f, field in enumerate(mt.resolved_fields):
        p = FFTPSF(lens, field, mt.resolved_wavelength, n, m)
        amp, opd = pupil_grids(p, n)
        psf = np.asarray(mt.psf[f], dtype=np.float64)
        assert np.array_equal(psf, np.asarray(p.psf)), f
        count = int(np.sum(amp > 0))
        self_diff = float(np.max(np.abs(double_sum(amp, opd, m, float(m)) / count ** 2 * 100.0
                                        - psf)))
        atol = bound(n, m, float(m), opd)
        assert self_diff < atol / 100.0, (f, self_diff, atol)
        worst = max(worst, self_diff)
        out.update({f"amp{f}": amp, f"opd{f}": opd, f"count{f}": count, f"psf{f}": psf,
                    f"tangential{f}": np.asarray(mt.mtf[f][0], dtype=np.float64),
                    f"sagittal{f}": np.asarray(mt.mtf[f][1], dtype=np.float64)})
    out["ref_self_diff"] = worst
    print(f"mtf_cooke: n {n}, m {m}, {len(mt.resolved_fields)} fields, cutoff "
          f"{out['max_freq']:.4f} cycles/mm, self diff {worst:.3g}")
    return out


def main():
    arrays = {}
    for key, (cls, builder, field, wl, num_rays, kw) in PSF_CASES.items():
        for name, v in psf_case(key, cls, builder, field, wl, num_rays, kw).items():
            arrays[f"{key}/{name}"] = np.asarray(v, dtype=np.float64)
    for name, v in mtf_case().items():
        arrays[f"mtf_cooke/{name}"] = np.asarray(v, dtype=np.float64)
    sizes = np.array([[r, *calculate_grid_size(r)] for r in GRID_SIZE_RAYS], dtype=np.float64)
    arrays["grid_size/table"] = sizes  # rows: num_rays, effective pupil sampling, grid size
    np.savez_compressed(os.path.join(HERE, "dft_psf.npz"), **arrays)


if __name__ == "__main__":
    main()
