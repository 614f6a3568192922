"""HuygensPSF (psf/base.py:51-97, 418-458; psf/huygens_fresnel.py:25-315): the point spread
function of one field point and wavelength by the Huygens-Fresnel sum over the exit pupil,
normalised so that the peak of the same pupil with zero phase error is 100 (the centre
pixel / 100 is the Strehl ratio).

The pupil data is the project's Wavefront (uniform pupil grid, traced and reduced on the
device); the sum itself -- the reference's Numba double loop over image points x pupil
points, huygens_fresnel_strategies.py:97 -- is one fused fp64 HIP kernel behind
torch.ops.ort.huygens_psf (ort_huygens_psf, csrc/ort_k_huygens.hip). The image grid is
formed on the host from the few numbers the reference also reads there (the centre of a
126-ray hexapolar trace, the working F/#), uploaded once, and sagged / globalised on the
device; the PSF and its normalisation stay device tensors. Visualisation (view) is out of
scope, as everywhere in this package.

FFTPSF (psf/fft.py:20-258) and MMDFTPSF (psf/mmdft.py:19-290): the same Wavefront data
scattered into the (num_rays, num_rays) pupil grid as a real amplitude and an OPD in waves,
and the pupil-to-image transform -- the reference's fftshift(fft2(padded pupil)) resp. its
matrix triple product L g R -- as one fused fp64 DFT, torch.ops.ort.dft_psf (ort_dft_psf,
csrc/ort_k_dft.hip), which forms the complex pupil and the twiddles on chip.
"""

from __future__ import annotations

import numpy as np
import torch

from .analysis import Wavefront, get_working_FNO, globalize_points, localize_points


def resolve_wavelength(optic, wavelength):
    """utils.py:113-135."""
    if isinstance(wavelength, str):
        if wavelength == "primary":
            return optic.primary_wavelength
        raise ValueError("Invalid wavelength string. For a single wavelength, it must be "
                         "'primary'.")
    if isinstance(wavelength, int | float):
        return float(wavelength)
    raise TypeError("Wavelength must be a string ('primary') or a number.")


class HuygensPSF(Wavefront):
    """psf/huygens_fresnel.py:25-315 on the device. Attributes as the reference's: psf
    (float64 device tensor [image_size, image_size]), pixel_pitch (mm), cx, cy (the centre
    of the image grid in the image surface's frame), image_size."""

    def __init__(self, optic, field, wavelength, num_rays=128, image_size=128,
                 strategy="chief_ray", remove_tilt=False, oversample=None, pixel_pitch=None,
                 **kwargs):
        super().__init__(optic, fields=[tuple(field)],
                         wavelengths=[resolve_wavelength(optic, wavelength)],
                         num_rays=num_rays, distribution="uniform", strategy=strategy,
                         remove_tilt=remove_tilt, **kwargs)
        self.cx = None
        self.cy = None
        self.pixel_pitch = pixel_pitch
        self.image_size = image_size
        self.oversample = oversample
        self.psf = self._compute_psf()

    # -- the image grid (huygens_fresnel.py:111-229) -----------------------------------
    def _determine_image_center(self):
        """:111-136: the image-frame intercepts of a 6-ring hexapolar trace with i > 0, as
        host arrays (the reference takes their mean and extent on the host too)."""
        Hx, Hy = self.fields[0]
        rays = self.optic.trace(Hx, Hy, self.wavelengths[0], num_rays=6,
                                distribution="hexapolar")
        valid = rays.i > 0
        if not bool(torch.any(valid)):
            return np.array([0.0]), np.array([0.0])
        rx, ry, _ = localize_points(rays.x[valid], rays.y[valid], rays.z[valid],
                                    self.optic.image_surface)
        return rx.cpu().numpy(), ry.cpu().numpy()

    def _get_image_extent(self):
        """:138-169."""
        rx, ry = self._determine_image_center()
        self.cx = np.mean(rx)
        self.cy = np.mean(ry)
        if self.pixel_pitch is not None:
            extent = 0.5 * self.image_size * self.pixel_pitch
        else:
            if self.oversample is not None:
                extent = self._extent_from_cutoff()
            else:
                extent = self._extent_from_geometry(rx, ry)
            self.pixel_pitch = 2 * extent / self.image_size
        return -extent + self.cx, extent + self.cx, -extent + self.cy, extent + self.cy

    def _extent_from_cutoff(self):
        """:171-183."""
        f_cutoff = 1.0 / (self._get_working_FNO() * self.wavelengths[0] * 1e-3)
        f_nyquist = self.oversample * f_cutoff
        self.pixel_pitch = 1.0 / (2 * f_nyquist)
        return 0.5 * self.image_size * self.pixel_pitch

    def _extent_from_geometry(self, rx, ry):
        """:185-202: the larger of the geometric footprint and 5 Airy radii."""
        num_Airy_disks = 5.0
        extent_geometric = np.max(np.hypot(rx - self.cx, ry - self.cy))
        extent_ideal = (num_Airy_disks * self._get_working_FNO() * 1.22
                        * (self.wavelengths[0] * 1e-3))
        return max(extent_geometric, extent_ideal)

    def _get_image_coordinates(self):
        """:204-229: the grid in the image surface's frame (linspace + meshgrid in the
        reference's index order: x varies along the second axis), its sag, and the points
        in the global frame -- device tensors [image_size, image_size]."""
        xmin, xmax, ymin, ymax = self._get_image_extent()
        image_x = np.linspace(xmin, xmax, self.image_size)
        image_y = np.linspace(ymin, ymax, self.image_size)
        image_x, image_y = np.meshgrid(image_x, image_y)
        surface = self.optic.image_surface
        dev = self._device()
        x = torch.as_tensor(np.ascontiguousarray(image_x).reshape(-1), device=dev)
        y = torch.as_tensor(np.ascontiguousarray(image_y).reshape(-1), device=dev)
        z = surface.geometry.sag(x, y).to(dev)
        shape = (self.image_size, self.image_size)
        return tuple(t.reshape(shape) for t in globalize_points(x, y, z, surface))

    def _device(self):
        return self.get_data(self.fields[0], self.wavelengths[0]).opd.device

    # -- normalisation and the sum (huygens_fresnel.py:231-315) ------------------------
    def _get_normalization(self):
        """:231-278: the on-axis pupil with zero OPD evaluated at the single point
        (0, 0, z_image), a 0-dim device tensor."""
        wl = self.wavelengths[0]
        if self.fields[0] == (0, 0):
            data = self.get_data((0, 0), wl)
        else:
            wf = Wavefront(self.optic, distribution="uniform", num_rays=self.num_rays,
                           fields=[(0, 0)], wavelengths=[wl])
            data = wf.get_data((0, 0), wl)
        dev = data.opd.device
        zero = torch.zeros((1, 1), dtype=torch.float64, device=dev)
        ideal_z = float(np.ravel(self.optic.surface_group.positions[-1])[0])
        psf_max = torch.ops.ort.huygens_psf(
            zero, zero, torch.full_like(zero, ideal_z), data.pupil_x, data.pupil_y,
            data.pupil_z, data.intensity, torch.zeros_like(data.opd), wl * 1e-3,
            float(data.radius))
        return psf_max[0, 0]

    def _compute_psf(self):
        """:280-315."""
        wavelength_mm = self.wavelengths[0] * 1e-3
        data = self.get_data(self.fields[0], self.wavelengths[0])
        pupil_opd = data.opd * wavelength_mm  # waves to mm
        image_x, image_y, image_z = self._get_image_coordinates()
        psf = torch.ops.ort.huygens_psf(image_x, image_y, image_z, data.pupil_x, data.pupil_y,
                                        data.pupil_z, data.intensity, pupil_opd,
                                        wavelength_mm, float(data.radius))
        return psf / self._get_normalization() * 100.0

    # -- psf/base.py:418-458 ----------------------------------------------------------
    def strehl_ratio(self):
        if self.psf is None:
            raise RuntimeError("PSF has not been computed.")
        strehl = self.psf[self.psf.shape[0] // 2, self.psf.shape[1] // 2] / 100
        return float(strehl.item())

    def _get_working_FNO(self):
        return get_working_FNO(self.optic, self.fields[0], self.wavelengths[0])


# --------------------------------------------------------------------------------------
# FFTPSF / MMDFTPSF (psf/fft.py, psf/mmdft.py)
# --------------------------------------------------------------------------------------
def calculate_grid_size(num_rays):
    """psf/fft.py:20-39: (effective pupil sampling, grid size) of OpticStudio's FFT PSF."""
    effective_pupil_sampling = np.floor(32 * 2 ** ((np.log2(num_rays) - 5) / 2)).astype(int)
    return effective_pupil_sampling, num_rays * 2


def pupil_grids(intensity, opd_waves, num_rays):
    """psf/fft.py:140-164 without the exponential: the per-ray intensity and OPD (waves) of a
    uniform-distribution Wavefront scattered into the linspace(-1, 1, num_rays) meshgrid where
    R^2 <= 1 (the reference's order, which is the distribution's), zero elsewhere ->
    (amp, opd), float64 (num_rays, num_rays) tensors on the inputs' device.
    amp = intensity / mean(intensity[intensity > 0]), all zeros when no ray is valid."""
    n = int(num_rays)
    x = np.linspace(-1, 1, n)
    x, y = np.meshgrid(x, x)
    inside = torch.as_tensor(np.flatnonzero((x.ravel() ** 2 + y.ravel() ** 2) <= 1),
                             device=intensity.device)
    if inside.numel() != intensity.numel() or opd_waves.numel() != intensity.numel():
        raise ValueError(f"pupil_grids: {intensity.numel()} rays for the {inside.numel()} "
                         f"points of a uniform pupil grid of {n} x {n}")
    valid = intensity > 0
    count = valid.sum()
    mean = torch.where(valid, intensity, torch.zeros_like(intensity)).sum() / count.clamp(min=1)
    amplitude = torch.where(count > 0, intensity / mean, torch.zeros_like(intensity))
    amp = torch.zeros(n * n, dtype=torch.float64, device=intensity.device)
    opd = torch.zeros_like(amp)
    amp[inside] = amplitude
    opd[inside] = opd_waves
    return amp.reshape(n, n), opd.reshape(n, n)


def normalized_dft_psf(amp, opd, image_size, pad_size):
    """psf/fft.py:194-203, 236-258 / psf/mmdft.py:180-208: dft_psf of one (n, n) pupil or a
    batch (B, n, n), scaled so that the same aperture with unit amplitude and zero phase peaks
    at 100: 100 / count_nonzero(amp)^2 per pupil (a device scalar; an empty aperture gives
    NaN as the reference's 0 / 0 does)."""
    raw = torch.ops.ort.dft_psf(amp.contiguous(), opd.contiguous(), int(image_size),
                                float(pad_size))
    count = (amp != 0).sum(dim=(-2, -1), keepdim=True).to(torch.float64)
    return raw / (count * count) * 100.0


class _PupilPSF(Wavefront):
    """What FFTPSF and MMDFTPSF share (psf/base.py:51-97): one field, one wavelength, the
    uniform pupil grid, and the pupil as real (amp, opd) device tensors."""

    def __init__(self, optic, field, wavelength, num_rays, strategy, remove_tilt, **kwargs):
        super().__init__(optic, fields=[tuple(field)],
                         wavelengths=[resolve_wavelength(optic, wavelength)],
                         num_rays=int(num_rays), distribution="uniform", strategy=strategy,
                         remove_tilt=remove_tilt, **kwargs)
        data = self.get_data(self.fields[0], self.wavelengths[0])
        self._amp, self._opd = pupil_grids(data.intensity, data.opd, self.num_rays)
        self._pupil = None

    def _complex_pupil(self):
        """psf/fft.py:161-164: amp exp(-2 pi i opd), complex128 -- for the attribute only (the
        transform never reads it)."""
        if self._pupil is None:
            self._pupil = torch.polar(self._amp, -2.0 * np.pi * self._opd)
        return self._pupil

    def _get_working_FNO(self):
        return get_working_FNO(self.optic, self.fields[0], self.wavelengths[0])


class FFTPSF(_PupilPSF):
    """psf/fft.py:42-258 on the device. Attributes as the reference's: psf (float64 device
    tensor [grid_size, grid_size]), pupils (a list of one complex128 [num_rays, num_rays]
    tensor, built on first access), grid_size, num_rays."""

    def __init__(self, optic, field, wavelength, num_rays=128, grid_size=None,
                 strategy="chief_ray", remove_tilt=False, **kwargs):
        if grid_size is None:
            if num_rays < 32:
                raise ValueError("num_rays must be at least 32 if grid_size is not specified.")
            num_rays, grid_size = calculate_grid_size(num_rays)
        elif grid_size < num_rays:
            raise ValueError(f"Grid size ({grid_size}) must be greater than or equal to the "
                             f"number of rays ({num_rays}).")
        super().__init__(optic, field, wavelength, num_rays, strategy, remove_tilt, **kwargs)
        self.grid_size = int(grid_size)
        self.psf = normalized_dft_psf(self._amp, self._opd, self.grid_size,
                                      float(self.grid_size))

    @property
    def pupils(self):
        return [self._complex_pupil()]

    def strehl_ratio(self):
        """psf/base.py:418-458: the centre pixel / 100."""
        if self.psf is None:
            raise RuntimeError("PSF has not been computed.")
        strehl = self.psf[self.psf.shape[0] // 2, self.psf.shape[1] // 2] / 100
        return float(strehl.item())


class MMDFTPSF(_PupilPSF):
    """psf/mmdft.py:19-290 on the device. Attributes as the reference's: psf (float64 device
    tensor [image_size, image_size]), pupil (complex128 [num_rays, num_rays], built on first
    access), image_size, pixel_pitch (um), num_rays. Where the reference multiplies by its
    raw `wavelength` argument this uses the resolved wavelength, so "primary" works."""

    def __init__(self, optic, field, wavelength, num_rays=128, image_size=None,
                 pixel_pitch=None, strategy="chief_ray", remove_tilt=False, **kwargs):
        grid_size = None
        if image_size is None and pixel_pitch is None:
            if num_rays < 32:
                raise ValueError("num_rays must be at least 32 if image_size and pixel_pitch "
                                 "are not specified.")
            num_rays, grid_size = calculate_grid_size(num_rays)
        super().__init__(optic, field, wavelength, num_rays, strategy, remove_tilt, **kwargs)
        # :90-117: the three-way resolution of image_size and pixel_pitch
        span = self.wavelengths[0] * self._get_working_FNO() * (self.num_rays - 1)
        if pixel_pitch is None:
            if image_size is None:
                image_size = grid_size
            pixel_pitch = span / image_size
        if image_size is None:
            image_size = int(span / pixel_pitch)
        self.image_size = image_size
        self.pixel_pitch = pixel_pitch
        # :246-261
        pad_size = span / self.pixel_pitch
        if self.image_size > pad_size:
            max_size = int(pad_size)
            raise ValueError(f"Supplied image_size of {self.image_size} not less than or equal "
                             f"to calculated pad size of {max_size}. Consider increasing "
                             "num_rays.")
        self.pad_size = float(pad_size)
        self.psf = normalized_dft_psf(self._amp, self._opd, int(self.image_size), self.pad_size)

    @property
    def pupil(self):
        return self._complex_pupil()

    def strehl_ratio(self):
        """psf/mmdft.py:210-228: max(psf) / 100 (the PSF may not be centred)."""
        if self.psf is None:
            raise RuntimeError("PSF has not been computed.")
        return float((torch.max(self.psf) / 100).item())
