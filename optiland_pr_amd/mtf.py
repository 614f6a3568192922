"""FFTMTF (mtf/base.py:25-72, mtf/fft.py:53-163): the modulation transfer function of every
field from its FFT PSF.

The pupils of all fields come from one Wavefront (uniform pupil grid, traced and reduced on
the device) and go through ONE batched torch.ops.ort.dft_psf call (ort_dft_psf,
csrc/ort_k_dft.hip). The reference reads two slices of |fftshift(fft2(psf))|: the column of
zero horizontal frequency and the row of zero vertical frequency. Each is the 1-D DFT of the
PSF's row sums resp. column sums, so that is what is computed -- torch.fft.fft of the
projection on the device, shifted, absolute value, divided by its own maximum; no 2-D FFT.
Visualisation (view) is out of scope, as everywhere in this package.

SampledMTF (mtf/sampled.py:17-207): the MTF at a list of arbitrary frequencies without a PSF,
from the pupil's overlap with its sheared copy -- one fused kernel for the whole list
(torch.ops.ort.sampled_otf).
"""

from __future__ import annotations

import numpy as np
import torch

from .analysis import Wavefront, get_working_FNO, resolve_fields
from .psf import calculate_grid_size, normalized_dft_psf, pupil_grids, resolve_wavelength


def mtf_curves(psf):
    """mtf/fft.py:146-151 for psf [..., G, G] -> (tangential, sagittal), each
    [..., G - G // 2]: |fftshift(fft2(psf))|[G // 2:, G // 2] and [G // 2, G // 2:], each over
    its maximum, from the 1-D DFTs of the projections."""
    half = psf.shape[-1] // 2

    def curve(projection):
        spectrum = torch.fft.fftshift(torch.fft.fft(projection, dim=-1), dim=-1).abs()
        c = spectrum[..., half:]
        return c / c.max(dim=-1, keepdim=True).values

    return curve(psf.sum(dim=-1)), curve(psf.sum(dim=-2))


class FFTMTF:
    """mtf/fft.py:17-163 on the device. Attributes as the reference's: psf (a list of float64
    device tensors [grid_size, grid_size], one per field), mtf (a list of [tangential,
    sagittal] device tensors of grid_size - grid_size // 2 values), freq (device tensor,
    cycles / mm), max_freq, FNO, num_rays, grid_size, resolved_fields, resolved_wavelength."""

    def __init__(self, optic, fields="all", wavelength="primary", num_rays=128, grid_size=None,
                 max_freq="cutoff", strategy="chief_ray", remove_tilt=False, **kwargs):
        if grid_size is None:
            self.num_rays, self.grid_size = calculate_grid_size(num_rays)
        else:
            self.num_rays, self.grid_size = num_rays, grid_size
        self.num_rays, self.grid_size = int(self.num_rays), int(self.grid_size)
        if self.grid_size < self.num_rays:  # psf/fft.py:104-108, through the reference's FFTPSF
            raise ValueError(f"Grid size ({self.grid_size}) must be greater than or equal to "
                             f"the number of rays ({self.num_rays}).")
        self.optic = optic
        self.fields = fields
        self.wavelength = wavelength
        self.strategy = strategy
        self.remove_tilt = remove_tilt
        self.strategy_kwargs = kwargs
        self.resolved_fields = resolve_fields(optic, fields)
        self.resolved_wavelength = resolve_wavelength(optic, wavelength)

        self._calculate_psf()
        self.mtf = self._generate_mtf_data()

        self.FNO = get_working_FNO(optic, (0, 0), self.resolved_wavelength)  # always on axis
        if max_freq == "cutoff":
            self.max_freq = 1 / (self.resolved_wavelength * 1e-3 * self.FNO)
        else:
            self.max_freq = max_freq
        self.freq = torch.arange(self.grid_size // 2, dtype=torch.float64,
                                 device=self.psf[0].device) * self._get_mtf_units()

    def _calculate_psf(self):
        """mtf/fft.py:82-99: every field's FFT PSF, all pupils in one dft_psf call."""
        wl = self.resolved_wavelength
        fields = [tuple(f) for f in self.resolved_fields]
        wf = Wavefront(self.optic, fields=fields, wavelengths=[wl], num_rays=self.num_rays,
                       distribution="uniform", strategy=self.strategy,
                       remove_tilt=self.remove_tilt, **self.strategy_kwargs)
        grids = [pupil_grids(d.intensity, d.opd, self.num_rays)
                 for d in (wf.get_data(f, wl) for f in fields)]
        amp = torch.stack([g[0] for g in grids])
        opd = torch.stack([g[1] for g in grids])
        psf = normalized_dft_psf(amp, opd, self.grid_size, float(self.grid_size))
        self.psf = list(psf.unbind(0))

    def _generate_mtf_data(self):
        tangential, sagittal = mtf_curves(torch.stack(self.psf))
        return [[t, s] for t, s in zip(tangential.unbind(0), sagittal.unbind(0), strict=True)]

    def _get_mtf_units(self):
        """mtf/fft.py:154-163."""
        return 1 / ((self.num_rays - 1) * self.resolved_wavelength * 1e-3 * self.FNO)


def pupil_shears(frequencies, wavelength_um, xpd, xpl):
    """mtf/sampled.py:158-178 on the host, in the reference's operation order: the shear of
    the pupil, in normalised pupil units, for each (fx, fy) in cycles / mm:
    xpl * (wl_mm * f) / (xpd / 2). -> (shift_x, shift_y), float64 arrays [F]."""
    wl_mm = wavelength_um * 1e-3
    f = np.asarray([(float(fx), float(fy)) for fx, fy in frequencies],
                   dtype=np.float64).reshape(-1, 2)
    half = xpd / 2
    return xpl * (wl_mm * f[:, 0]) / half, xpl * (wl_mm * f[:, 1]) / half


def otf_modulus(otf, otf_at_zero):
    """mtf/sampled.py:198-203: |otf| / otf_at_zero of [..., 2] (re, im), 0 where otf_at_zero
    is 0; otf_at_zero broadcasts against otf[..., 0]."""
    mod = torch.hypot(otf[..., 0], otf[..., 1])
    zero = otf_at_zero == 0
    return torch.where(zero, torch.zeros_like(mod), mod / torch.where(zero, 1.0, otf_at_zero))


class SampledMTF:
    """mtf/sampled.py:17-207 on the device: the MTF at arbitrary (fx, fy) as the overlap sum
    of the pupil with a copy of itself sheared through the Zernike fit of its OPD.

    Attributes as the reference's: optic, field, wavelength, num_rays, distribution,
    zernike_terms, zernike_type, x_norm, y_norm, opd_waves, intensity (float64 device tensors),
    xpd, xpl, zernike_fit and otf_at_zero (a 0-dim device tensor). The reference's complex
    pupil P1 is omitted: the kernel folds exp(i 2 pi opd) and exp(-i 2 pi W) into one
    exponential and never stores either factor.

    The wavefront is traced and reduced on the device; the constructor reads the OPD back
    once for the host least-squares fit. calculate_mtf sends every frequency of the list
    through ONE torch.ops.ort.sampled_otf call (ort_sampled_otf, csrc/ort_k_sampled_otf.hip)
    and reads the result back once."""

    def __init__(self, optic, field, wavelength, num_rays=128, distribution="uniform",
                 zernike_terms=37, zernike_type="fringe"):
        from .zernike import ZernikeFit

        self.optic = optic
        self.field = field
        self.wavelength = resolve_wavelength(optic, wavelength)
        self.num_rays = num_rays
        self.distribution = distribution
        self.zernike_terms = zernike_terms
        self.zernike_type = zernike_type

        wf = Wavefront(optic, fields=[self.field], wavelengths=[self.wavelength],
                       num_rays=self.num_rays, distribution=self.distribution)
        data = wf.get_data(self.field, self.wavelength)
        dev = data.opd.device
        self.x_norm = torch.as_tensor(np.asarray(wf.distribution.x, dtype=np.float64), device=dev)
        self.y_norm = torch.as_tensor(np.asarray(wf.distribution.y, dtype=np.float64), device=dev)
        self.opd_waves = data.opd
        self.intensity = data.intensity

        self.xpd = self.optic.paraxial.XPD()
        self.xpl = -self.optic.paraxial.XPL()

        self.zernike_fit = ZernikeFit(self.x_norm, self.y_norm, self.opd_waves,
                                      self.zernike_type, self.zernike_terms)
        self.otf_at_zero = torch.sum(self.intensity)

    def calculate_mtf(self, frequencies, as_tensor=False):
        """mtf/sampled.py:108-207: the MTF at each (fx, fy) in cycles / mm, a list of Python
        floats (as_tensor=True: the float64 device tensor [F], no read-back)."""
        freqs = [(float(fx), float(fy)) for fx, fy in frequencies]
        dev = self.opd_waves.device
        if self.xpd == 0.0:  # sampled.py:163-168
            out = [1.0 if fx == 0.0 and fy == 0.0 else 0.0 for fx, fy in freqs]
            return torch.tensor(out, dtype=torch.float64, device=dev) if as_tensor else out
        sx, sy = pupil_shears(freqs, self.wavelength, self.xpd, self.xpl)
        otf = torch.ops.ort.sampled_otf(
            self.x_norm, self.y_norm, self.intensity, self.opd_waves, self.zernike_fit.coeffs,
            self.zernike_type, torch.as_tensor(sx, device=dev), torch.as_tensor(sy, device=dev))
        mtf = otf_modulus(otf, self.otf_at_zero)
        return mtf if as_tensor else mtf.cpu().tolist()
