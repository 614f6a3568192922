"""IncoherentIrradiance (analysis/irradiance.py:35-330): the power of the traced rays binned
on a detector surface that carries a physical aperture, in W/mm^2, per (field, wavelength).

The trace is the project's (Optic.trace, or SurfaceGroup.trace for user_initial_rays); the
image points are taken into the detector surface's frame with localize_points; the sum -- the
reference's numpy.histogram2d, or get_bilinear_weights + four index_put(accumulate=True) in
its differentiable form -- is one fixed-point HIP binning op, torch.ops.ort.irradiance_bin
(ort_irradiance_bin, csrc/ort_k_irradiance.hip): bit-identical under any order of the rays.
The maps stay device tensors; the edges are host NumPy arrays, as in the reference.
Visualisation (view) is out of scope, as everywhere in this package.

Orientation, as in the reference: the histogram map is [npix_x, npix_y] (X is the row
index), the bilinear (differentiable) map is [npix_y, npix_x].
"""

from __future__ import annotations

import numpy as np
import torch

from . import _abi
from .analysis import localize_points, resolve_wavelengths
from .raytrace import RealRays


class IncoherentIrradiance:
    """analysis/irradiance.py:35-330 on the device. data[f][w] = (irr, x_edges, y_edges).

    differentiable: None (default) bins with the bilinear mode when the traced x, y or
    intensity require grad (the reference's be.grad_mode switch) and with the histogram
    otherwise; True / False force the choice."""

    def __init__(self, optic, num_rays=5, res=(128, 128), px_size=None, detector_surface=-1, *,
                 fields="all", wavelengths="all", distribution="random",
                 user_initial_rays=None, differentiable=None):
        if fields == "all":
            self.fields = optic.fields.get_field_coords()
        else:
            self.fields = tuple(fields)
        self.num_rays = num_rays
        self.npix_x, self.npix_y = res
        self.px_size = None if px_size is None else (float(px_size[0]), float(px_size[1]))
        self.detector_surface = int(detector_surface)
        self.user_initial_rays = user_initial_rays
        if user_initial_rays is not None and not isinstance(user_initial_rays, RealRays):
            raise TypeError("user_initial_rays must be a RealRays object.")
        self.distribution = distribution
        self.differentiable = differentiable

        surf = optic.surface_group.surfaces[self.detector_surface]
        if surf.aperture is None:
            raise ValueError(
                "Detector surface has no physical aperture - set one "
                "(e.g. RectangularAperture) so that the detector size is defined.")

        if self.px_size is not None:
            x_min, x_max, y_min, y_max = surf.aperture.extent
            new_npix_x = int(round((x_max - x_min) / self.px_size[0]))
            new_npix_y = int(round((y_max - y_min) / self.px_size[1]))
            print("[IncoherentIrradiance] Warning: res parameter ignored - derived "
                  f"from px_size instead → ({new_npix_x},{new_npix_y}) pixels")
            self.npix_x, self.npix_y = new_npix_x, new_npix_y

        self.optic = optic
        self.wavelengths = resolve_wavelengths(optic, wavelengths)
        self.data = self._generate_data()

    def peak_irradiance(self):
        """Maximum pixel value for each (field, wavelength) pair (0-dim device tensors)."""
        return [[torch.max(irr) for irr, *_ in fblock] for fblock in self.data]

    def _generate_data(self):
        return [[self._generate_field_data(field, wl) for wl in self.wavelengths]
                for field in self.fields]

    def _trace(self, field, wavelength):
        """:257-266: the traced rays of one (field, wavelength); user rays are copied, so every
        pair traces the same initial rays."""
        if self.user_initial_rays is None:
            Hx, Hy = field
            return self.optic.trace(Hx, Hy, wavelength, self.num_rays, self.distribution)
        u = self.user_initial_rays
        rays = RealRays(u.x.clone(), u.y.clone(), u.z.clone(), u.L.clone(), u.M.clone(),
                        u.N.clone(), u.i.clone(), u.w.clone(), device=u.x.device)
        self.optic.surface_group.trace(rays)
        return rays

    def _edges(self, surf):
        """:281-298: the pixel edges and area (linspace over the aperture's extent, or arange
        with the pixel pitch, which may correct the resolution once more)."""
        x_min, x_max, y_min, y_max = surf.aperture.extent
        if self.px_size is None:
            x_edges = np.linspace(x_min, x_max, self.npix_x + 1, dtype=float)
            y_edges = np.linspace(y_min, y_max, self.npix_y + 1, dtype=float)
            return x_edges, y_edges, (x_edges[1] - x_edges[0]) * (y_edges[1] - y_edges[0])
        dx, dy = self.px_size
        x_edges = np.arange(x_min, x_max + 0.5 * dx, dx, dtype=float)
        y_edges = np.arange(y_min, y_max + 0.5 * dy, dy, dtype=float)
        exp_nx, exp_ny = len(x_edges) - 1, len(y_edges) - 1
        if (exp_nx, exp_ny) != (self.npix_x, self.npix_y):
            print("[IncoherentIrradiance] Warning: res parameter ignored - "
                  f"derived from px_size instead → ({exp_nx},{exp_ny}) pixels")
            self.npix_x, self.npix_y = exp_nx, exp_ny
        return x_edges, y_edges, dx * dy

    def _generate_field_data(self, field, wavelength):
        """:250-330: trace, localise, bin."""
        rays = self._trace(field, wavelength)
        surf = self.optic.surface_group.surfaces[self.detector_surface]
        x, y, _ = localize_points(rays.x, rays.y, rays.z, surf)
        power = rays.i
        x_edges, y_edges, pixel_area = self._edges(surf)
        bilinear = self.differentiable
        if bilinear is None:
            bilinear = any(t.requires_grad for t in (x, y, power))
        if bilinear and x.numel() == 0:  # (:305-307, with the reference's shape)
            return (torch.zeros((self.npix_x, self.npix_y), dtype=torch.float64,
                                device=x.device), x_edges, y_edges)
        mode = _abi.BIN_BILINEAR if bilinear else _abi.BIN_HISTOGRAM
        if not bilinear:
            x, y, power = x.detach(), y.detach(), power.detach()
        ex = torch.as_tensor(x_edges, dtype=torch.float64, device=x.device)
        ey = torch.as_tensor(y_edges, dtype=torch.float64, device=x.device)
        irr = torch.ops.ort.irradiance_bin(x.contiguous(), y.contiguous(), power.contiguous(),
                                           ex, ey, mode, float(pixel_area))
        return irr, x_edges, y_edges
