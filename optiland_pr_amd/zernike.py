"""Zernike bases and the least-squares fit (zernike/base.py:26-258, zernike/standard.py,
fringe.py, noll.py, zernike/fit.py:33-118).

ZernikeStandard, ZernikeFringe and ZernikeNoll evaluate sum_j c_j N_j R_nj^|mj|(r) {cos | sin}
(|mj| phi) with the reference's own operations -- the factorial-weighted power sum and
cos / sin of m * phi, term by term -- on NumPy arrays or torch tensors. The index order, the
radial weights and the normalisation constants are the ones the Zernike surfaces use
(geometries.zernike_indices, radial_coefficients, _norm_constant): one copy of each table.

ZernikeFit solves for the coefficients as the reference does: the design matrix of unit-
coefficient terms stacked on axis 1, numpy.linalg.lstsq(rcond=None) in float64 on the host
(the precedent is analysis.BestFitSphereStrategy). Device tensors are read back once; the
coefficients return as a float64 tensor on the inputs' device. Visualisation (view,
view_residual) is out of scope, as everywhere in this package.
"""

from __future__ import annotations

import numpy as np
import torch

from .geometries import _norm_constant, radial_coefficients, zernike_indices


def _is_tensor(v):
    return torch.is_tensor(v)


class BaseZernike:
    """zernike/base.py:26-258. coeffs: a sequence, array or tensor of coefficients (None:
    num_terms zeros, a float64 CPU tensor)."""

    kind = None

    def __init__(self, coeffs=None, num_terms=36):
        self.coeffs = torch.zeros(num_terms, dtype=torch.float64) if coeffs is None else coeffs
        self.indices = zernike_indices(self.kind, len(self.coeffs))

    def _norm_constant(self, n, m):
        return float(_norm_constant(self.kind, n, m))

    @staticmethod
    def _radial_term(n, m, r):
        """base.py:215-239: value = 0 + a_0 r^n + a_1 r^(n-2) + ... in that order."""
        a, _ = radial_coefficients(int(n), abs(int(m)))
        if _is_tensor(r):
            value = torch.zeros_like(r)
        elif isinstance(r, (int, float)):
            value = 0.0
        else:
            r = np.asarray(r)
            value = np.zeros_like(r)
        for k, coeff in enumerate(a):
            value = value + coeff * (r ** (int(n) - 2 * k))
        return value

    @staticmethod
    def _azimuthal_term(m=0, phi=0):
        """base.py:241-258."""
        m = int(m)
        if _is_tensor(phi):
            return torch.cos(m * phi) if m >= 0 else torch.sin(abs(m) * phi)
        return np.cos(m * np.asarray(phi)) if m >= 0 else np.sin(abs(m) * np.asarray(phi))

    def get_term(self, coeff=0, n=0, m=0, r=0, phi=0):
        """base.py:42-68."""
        return (coeff * self._norm_constant(n, m) * self._radial_term(n, m, r)
                * self._azimuthal_term(m, phi))

    def _coefficients_for(self, r):
        """The coefficients as factors of r's kind: Python floats for NumPy / scalar points
        (one read-back of a tensor), 0-dim tensors for tensor points."""
        c = self.coeffs
        if _is_tensor(r):
            if not _is_tensor(c):
                c = torch.tensor(np.asarray(c, dtype=np.float64))
            return list(c.to(device=r.device, dtype=torch.float64).unbind(0))
        if _is_tensor(c):
            return c.detach().cpu().tolist()
        return [float(v) for v in c]

    def terms(self, r=0, phi=0):
        """base.py:70-88: the list of term values, in coefficient order."""
        coeffs = self._coefficients_for(r)
        return [self.get_term(c, n, m, r, phi)
                for c, (n, m) in zip(coeffs, self.indices, strict=True)]

    def poly(self, r=0, phi=0):
        """base.py:90-102: sum(terms), Python's left-to-right sum from int 0."""
        return sum(self.terms(r, phi))


class ZernikeStandard(BaseZernike):
    """zernike/standard.py (OSA/ANSI indices)."""

    kind = "standard"


class ZernikeFringe(BaseZernike):
    """zernike/fringe.py (Fringe / University of Arizona indices, no normalisation)."""

    kind = "fringe"


class ZernikeNoll(BaseZernike):
    """zernike/noll.py (Noll indices)."""

    kind = "noll"


ZERNIKE_CLASSES = {"fringe": ZernikeFringe, "standard": ZernikeStandard, "noll": ZernikeNoll}


def design_matrix(kind, num_terms, radius, phi):
    """fit.py:105-106: the unit-coefficient terms of a scheme stacked on axis 1, [N, T]
    float64 on the host."""
    basis = ZERNIKE_CLASSES[kind](np.ones(num_terms))
    terms = basis.terms(np.asarray(radius, dtype=np.float64), np.asarray(phi, dtype=np.float64))
    if not terms:
        return np.zeros((np.size(radius), 0))
    return np.stack(terms, axis=1)


class ZernikeFit:
    """zernike/fit.py:33-118. Attributes as the reference's: x, y, z (flattened, of the
    inputs' kind), radius, phi, num_pts, num_terms, zernike_type, zernike (the basis holding
    the fitted coefficients) and coeffs (float64 tensor on the inputs' device)."""

    def __init__(self, x, y, z, zernike_type="fringe", num_terms=36):
        device = next((v.device for v in (x, y, z) if _is_tensor(v)), torch.device("cpu"))

        def flat(v):
            if _is_tensor(v):
                return v.detach().reshape(-1).to(dtype=torch.float64)
            return torch.as_tensor(np.asarray(v, dtype=np.float64).reshape(-1))

        self.x, self.y, self.z = (flat(v).to(device) for v in (x, y, z))
        if self.x.shape != self.y.shape or self.x.shape != self.z.shape:
            raise ValueError("`x`, `y`, and `z` must have the same number of elements.")
        self.num_terms = num_terms
        self.num_pts = int(self.x.numel())
        # the one read-back; the polar coordinates with NumPy's operations (fit.py:77-78)
        xh, yh, zh = torch.stack([self.x, self.y, self.z]).cpu().numpy()
        radius = np.sqrt(xh**2 + yh**2)
        phi = np.arctan2(yh, xh)
        self.radius = torch.as_tensor(radius, device=device)
        self.phi = torch.as_tensor(phi, device=device)
        if zernike_type not in ZERNIKE_CLASSES:
            raise ValueError(f"Invalid Zernike type '{zernike_type}'. "
                             f"Choose from: {list(ZERNIKE_CLASSES)}")
        self.zernike_type = zernike_type
        self.zernike = ZERNIKE_CLASSES[zernike_type](
            torch.ones(num_terms, dtype=torch.float64, device=device))
        self._fit(radius, phi, zh, device)

    @property
    def coeffs(self):
        return self.zernike.coeffs

    def _fit(self, radius, phi, z, device):
        """fit.py:101-118: A c = z in the least-squares sense."""
        A = design_matrix(self.zernike_type, self.num_terms, radius, phi)
        coeffs = np.linalg.lstsq(A, z, rcond=None)[0]
        self.zernike.coeffs = torch.as_tensor(np.ascontiguousarray(coeffs, dtype=np.float64),
                                              device=device)
