"""ThroughFocusMTF (analysis/through_focus.py:15-147, analysis/through_focus_mtf.py:27-123):
the tangential and sagittal MTF at one spatial frequency for every field, at image-plane
positions around the nominal focus.

The reference builds one SampledMTF per field and step and calls it twice. Here a step is one
Wavefront over all fields (traced and reduced on the device), one Zernike fit per field on
the host, and ONE torch.ops.ort.sampled_otf call with B = n_fields and F = 2 -- the shears
(f, 0) and (0, f) -- followed by one read-back. Visualisation (view) is out of scope, as
everywhere in this package.
"""

from __future__ import annotations

import numpy as np
import torch

from .analysis import Wavefront
from .mtf import otf_modulus, pupil_shears
from .zernike import ZernikeFit


class ThroughFocusAnalysis:
    """analysis/through_focus.py:15-147: the loop over image-plane positions. A subclass
    supplies _perform_analysis_at_focus. The nominal focus is restored afterwards, also when
    a step raises."""

    MAX_STEPS = 7
    MIN_STEPS = 1

    def __init__(self, optic, delta_focus=0.1, num_steps=5, fields="all", wavelengths="all"):
        self.optic = optic
        self.delta_focus = delta_focus
        self._validate_num_steps(num_steps)
        self.num_steps = num_steps
        self.fields = self._resolve_fields(fields)
        self.wavelengths = self._resolve_wavelengths(wavelengths)
        self.positions = self._generate_focus_positions()
        self.nominal_focus = float(self.optic.image_surface.geometry.cs.z)
        self.results = []
        self._calculate_through_focus()

    def _validate_num_steps(self, num_steps):
        if not isinstance(num_steps, int) or num_steps < self.MIN_STEPS:
            raise ValueError("'num_steps' must be a positive integer.")
        if num_steps % 2 == 0:
            raise ValueError("'num_steps' must be an odd integer.")
        if num_steps > self.MAX_STEPS:
            raise ValueError(
                "'num_steps' must be less than or equal to 7 for performance reasons.")

    def _resolve_fields(self, fields):
        return self.optic.fields.get_field_coords() if fields == "all" else fields

    def _resolve_wavelengths(self, wavelengths):
        return (self.optic.wavelengths.get_wavelengths() if wavelengths == "all"
                else wavelengths)

    def _generate_focus_positions(self):
        nominal_focus = self.optic.image_surface.geometry.cs.z
        return [nominal_focus + (i - self.num_steps // 2) * self.delta_focus
                for i in range(self.num_steps)]

    def _defocus_image_plane(self, z_position):
        self.optic.image_surface.geometry.cs.z = z_position

    def _reset_focus(self):
        self._defocus_image_plane(self.nominal_focus)

    def _perform_analysis_at_focus(self):
        raise NotImplementedError

    def _calculate_through_focus(self):
        try:
            for position in self.positions:
                self._defocus_image_plane(position)
                self.results.append(self._perform_analysis_at_focus())
        finally:
            self._reset_focus()


class ThroughFocusMTF(ThroughFocusAnalysis):
    """analysis/through_focus_mtf.py:27-123. results[step][field] = {"tangential": ...,
    "sagittal": ...} (Python floats) at (spatial_frequency, 0) and (0, spatial_frequency);
    positions, nominal_focus, fields, wavelength, num_rays as the reference's."""

    MAX_STEPS = 15
    MIN_STEPS = 1
    ZERNIKE_TERMS = 37
    ZERNIKE_TYPE = "fringe"

    def __init__(self, optic, spatial_frequency, delta_focus=0.1, num_steps=5, fields="all",
                 wavelength="primary", num_rays=128):
        self.spatial_frequency = spatial_frequency
        self.num_rays = num_rays
        self.wavelength = optic.primary_wavelength if wavelength == "primary" else wavelength
        super().__init__(optic, delta_focus=delta_focus, num_steps=num_steps, fields=fields,
                         wavelengths=[self.wavelength])

    def _perform_analysis_at_focus(self):
        fields = [tuple(f) for f in self.fields]
        wl = float(self.wavelength)
        wf = Wavefront(self.optic, fields=fields, wavelengths=[wl], num_rays=self.num_rays,
                       distribution="uniform")
        data = [wf.get_data(f, wl) for f in fields]
        dev = data[0].opd.device
        x = torch.as_tensor(np.asarray(wf.distribution.x, dtype=np.float64), device=dev)
        y = torch.as_tensor(np.asarray(wf.distribution.y, dtype=np.float64), device=dev)
        intensity = torch.stack([d.intensity for d in data])
        opd = torch.stack([d.opd for d in data])
        coeffs = torch.stack([ZernikeFit(x, y, d.opd, self.ZERNIKE_TYPE,
                                         self.ZERNIKE_TERMS).coeffs for d in data])
        xpd = self.optic.paraxial.XPD()
        xpl = -self.optic.paraxial.XPL()
        f = float(self.spatial_frequency)
        freqs = [(f, 0.0), (0.0, f)]
        if xpd == 0.0:  # mtf/sampled.py:163-168
            row = [1.0 if fx == 0.0 and fy == 0.0 else 0.0 for fx, fy in freqs]
            return [{"tangential": row[0], "sagittal": row[1]} for _ in fields]
        sx, sy = pupil_shears(freqs, wl, xpd, xpl)
        otf = torch.ops.ort.sampled_otf(x, y, intensity, opd, coeffs, self.ZERNIKE_TYPE,
                                        torch.as_tensor(sx, device=dev),
                                        torch.as_tensor(sy, device=dev))
        mtf = otf_modulus(otf, intensity.sum(dim=1, keepdim=True)).cpu().tolist()
        return [{"tangential": t, "sagittal": s} for t, s in mtf]
