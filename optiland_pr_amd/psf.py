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
