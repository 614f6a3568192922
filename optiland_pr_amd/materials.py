"""Materials: n(lambda) and k(lambda) evaluated on the HOST into small tables.

Mirrors the reference interface optiland/materials/{base,ideal,material_file,material}.py
(BaseMaterial.n / .k, IdealMaterial(n, k), Material(name, reference)). The reference
evaluates n and k per ray and caches them by the whole wavelength array
(materials/base.py:73-119, ~60% of its DoubleGauss trace time); here they are
evaluated once per (material, wavelength) in NumPy and handed to the kernel as
n_tab / alpha_tab columns.

Catalog glasses come from optiland_pr_amd/data/glasses.json, baked from the reference's
refractiveindex.info database by tests/golden/gen_golden.py (formula id, coefficients,
tabulated k). The dispersion formulas restate material_file.py:250-428.
"""

from __future__ import annotations

import json
import os

import numpy as np

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "glasses.json")
_GLASSES = None


def _glass_db():
    global _GLASSES
    if _GLASSES is None:
        with open(_DATA) as f:
            _GLASSES = json.load(f)
    return _GLASSES


class HomogeneousPropagation:
    """propagation/homogeneous.py:18-57: straight-line propagation with absorption, the
    only propagation model of the trace core (BaseMaterial.propagation_model)."""

    def __init__(self, material):
        self.material = material


class BaseMaterial:
    """materials/base.py:23-119 interface: n(wavelength), k(wavelength),
    propagation_model (base.py:60-71: HomogeneousPropagation by default)."""

    @property
    def propagation_model(self):
        return HomogeneousPropagation(self)

    def n(self, wavelength):
        w = np.atleast_1d(np.asarray(wavelength, dtype=np.float64))
        return self._calculate_n(w)

    def k(self, wavelength):
        w = np.atleast_1d(np.asarray(wavelength, dtype=np.float64))
        return self._calculate_k(w)

    def n_scalar(self, wavelength: float) -> float:
        return float(np.ravel(self.n(np.array([float(wavelength)])))[0])

    def k_scalar(self, wavelength: float) -> float:
        return float(np.ravel(self.k(np.array([float(wavelength)])))[0])

    def key(self):
        raise NotImplementedError


class IdealMaterial(BaseMaterial):
    """materials/ideal.py:21-70: constant n and k."""

    def __init__(self, n: float, k: float = 0.0):
        self.index = np.array([n], dtype=np.float64)
        self.absorp = np.array([k], dtype=np.float64)

    def _calculate_n(self, w):
        return np.full_like(w, self.index[0])

    def _calculate_k(self, w):
        return np.full_like(w, self.absorp[0])

    def key(self):
        return ("ideal", float(self.index[0]), float(self.absorp[0]))

    def lower(self):
        """-> (kind, coefficients, k wavelengths, k values, n_const, k_const)."""
        return 0, [], [], [], float(self.index[0]), float(self.absorp[0])

    def __repr__(self):
        return f"IdealMaterial(n={self.index[0]}, k={self.absorp[0]})"


class Material(BaseMaterial):
    """Catalog glass (materials/material.py:22-75 + material_file.py:31-428).

    By name, only glasses baked into data/glasses.json are available (the sample lenses'
    glasses); other names raise ValueError, as the reference does for an unknown name.
    Any other refractiveindex.info material comes in as a record of the same fields
    through Material.from_entry.
    """

    def __init__(self, name: str, reference: str | None = None):
        db = _glass_db()
        key = name if reference is None else f"{name}|{reference}"
        if key not in db:
            # the reference's robust search ignores a reference it cannot match
            cands = [k for k in db if k.split("|")[0].lower() == name.lower()]
            if not cands:
                raise ValueError(f"No matching material found for {name!r} ({reference!r}).")
            key = cands[0]
        self._set_entry(db[key])

    @classmethod
    def from_entry(cls, entry):
        """A Material from a record with the fields of a data/glasses.json entry: name,
        reference, source (the file's path in the database: the material's identity,
        key()), formula ("formula 1" .. "formula 9", "tabulated n", "tabulated nk"),
        coefficients as the file lists them, and the k_wavelength / k and n_wavelength / n
        tables (None where the file has none)."""
        m = cls.__new__(cls)
        m._set_entry(entry)
        return m

    def _set_entry(self, e):
        arr = lambda v: None if v is None else np.array(v, dtype=np.float64)  # noqa: E731
        self.name = e["name"]
        self.reference = e.get("reference")
        self.source = e["source"]
        self._n_formula = e["formula"]
        self.coefficients = arr(e.get("coefficients"))
        self._k_wavelength = arr(e.get("k_wavelength"))
        self._k = arr(e.get("k"))
        self._n_wavelength = arr(e.get("n_wavelength"))
        self._n = arr(e.get("n"))

    def key(self):
        return ("glass", self.source)

    def lower(self):
        return lower_dispersion(self._n_formula, self.coefficients, self._k_wavelength,
                                self._k, self._n_wavelength, self._n)

    def __repr__(self):
        return f"Material({self.name!r}, {self.reference!r})"

    # -- material_file.py:219-249 --
    def _calculate_k(self, w):
        if self._k is None or self._k_wavelength is None:
            return np.zeros_like(w)
        return np.interp(w, self._k_wavelength, self._k)

    def _calculate_n(self, w):
        f = {
            "formula 1": self._formula_1, "formula 2": self._formula_2,
            "formula 3": self._formula_3, "formula 4": self._formula_4,
            "formula 5": self._formula_5, "formula 6": self._formula_6,
            "formula 7": self._formula_7, "formula 8": self._formula_8,
            "formula 9": self._formula_9, "tabulated n": self._tabulated_n,
            "tabulated nk": self._tabulated_n,
        }[self._n_formula]
        return f(w)

    # The coefficient arrays are kept as shape-(1,) arrays, as the reference's
    # parser leaves them, so NumPy evaluates the same broadcasted expressions.
    def _c(self):
        return [np.array([v]) for v in self.coefficients]

    def _formula_1(self, w):  # material_file.py:250-268 (Sellmeier)
        c = self._c()
        n = 1 + c[0]
        for k in range(1, len(c), 2):
            n = n + c[k] * w**2 / (w**2 - c[k + 1] ** 2)
        return np.sqrt(n)

    def _formula_2(self, w):  # :270-288 (Sellmeier-2)
        c = self._c()
        n = 1 + c[0]
        for k in range(1, len(c), 2):
            n = n + c[k] * w**2 / (w**2 - c[k + 1])
        return np.sqrt(n)

    def _formula_3(self, w):  # :290-308 (polynomial)
        c = self._c()
        n = c[0]
        for k in range(1, len(c), 2):
            n = n + c[k] * w ** c[k + 1]
        return np.sqrt(n)

    def _formula_4(self, w):  # :310-333 (RefractiveIndex.INFO)
        c = self._c()
        n = (c[0] + c[1] * w ** c[2] / (w**2 - c[3] ** c[4])
             + c[5] * w ** c[6] / (w**2 - c[7] ** c[8]))
        for k in range(9, len(c), 2):
            n = n + c[k] * w ** c[k + 1]
        return np.sqrt(n)

    def _formula_5(self, w):  # :335-352 (Cauchy)
        c = self._c()
        n = c[0]
        for k in range(1, len(c), 2):
            n = n + c[k] * w ** c[k + 1]
        return n

    def _formula_6(self, w):  # :354-371 (gases)
        c = self._c()
        n = 1 + c[0]
        for k in range(1, len(c), 2):
            n = n + c[k] / (c[k + 1] - w**-2)
        return n

    def _formula_7(self, w):  # :373-390 (Herzberger)
        c = self._c()
        n = c[0] + c[1] / (w**2 - 0.028) + c[2] * (1 / (w**2 - 0.028)) ** 2
        for k in range(3, len(c)):
            n = n + c[k] * w ** (2 * (k - 2))
        return n

    def _formula_8(self, w):  # :392-405 (retro)
        c = self._c()
        b = c[0] + c[1] * w**2 / (w**2 - c[2]) + c[3] * w**2
        return np.sqrt((1 + 2 * b) / (1 - b))

    def _formula_9(self, w):  # :407-420 (exotic)
        c = self._c()
        n = c[0] + c[1] / (w**2 - c[2]) + c[3] * (w - c[4]) / ((w - c[4]) ** 2 + c[5])
        return np.sqrt(n)

    def _tabulated_n(self, w):  # :422-428
        return np.interp(w, self._n_wavelength, self._n)


_ABBE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "abbe_coefficients.json")
_ABBE_COEF = None


class AbbeMaterial(BaseMaterial):
    """materials/abbe.py:19-126: a model glass from nd and the Abbe number, n(w) a cubic
    polynomial in w whose coefficients are a fixed linear map (the reference's
    database/glass_model_coefficients.npy, baked into data/abbe_coefficients.json) of
    (nd, vd, nd^2, vd^2, nd^3, vd^3); valid for 0.380 <= w <= 0.750 um, k = 0."""

    def __init__(self, n, abbe):
        global _ABBE_COEF
        if _ABBE_COEF is None:
            with open(_ABBE) as f:
                _ABBE_COEF = np.array(json.load(f)["coefficients"], dtype=np.float64)
        self.index = np.array([n], dtype=np.float64)
        self.abbe = np.array([abbe], dtype=np.float64)
        x = np.ravel(np.array([self.index, self.abbe, self.index**2, self.abbe**2,
                               self.index**3, self.abbe**3]))
        self._p = np.matmul(x, _ABBE_COEF)  # abbe.py:67-98

    def _calculate_n(self, w):  # abbe.py:37-51
        if np.any(w < 0.380) or np.any(w > 0.750):
            raise ValueError("Wavelength out of range for this model.")
        return np.atleast_1d(np.polyval(self._p, w))

    def _calculate_k(self, w):  # abbe.py:53-65 (zeros_like(0))
        return np.zeros_like(w)

    def key(self):
        return ("abbe", float(self.index[0]), float(self.abbe[0]))

    def lower(self):
        """ORT_MAT_ABBE: the 4 polynomial coefficients (highest power first)."""
        return 11, [float(v) for v in self._p], [], [], 0.0, 0.0

    def __repr__(self):
        return f"AbbeMaterial(n={self.index[0]}, abbe={self.abbe[0]})"


def lower_dispersion(formula, coefficients, k_wavelength, k, n_wavelength, n):
    """Per-ray dispersion record of a catalog material (include/optiland_rt.h
    ort_material) -> (kind, coefficients, k wavelengths, k values, n_const, k_const):
    the formula id and its coefficients with the wavelength-independent subexpressions
    formed here in NumPy exactly as the reference forms them on every call
    (material_file.py:250-428: 1 + C0, C ** 2, C3 ** C4, C7 ** C8), and the tabulated k
    data (:219-249)."""
    kw = [] if k is None or k_wavelength is None else [float(v) for v in np.ravel(k_wavelength)]
    kv = [] if not kw else [float(v) for v in np.ravel(k)]
    if formula in ("tabulated n", "tabulated nk"):
        return (10, [float(v) for v in np.ravel(n_wavelength)] + [float(v) for v in np.ravel(n)],
                kw, kv, 0.0, 0.0)
    fid = int(str(formula).split()[-1])
    c = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in np.ravel(coefficients)]
    f1 = lambda v: float(np.ravel(v)[0])  # noqa: E731
    if fid in (1, 2, 3, 5, 6) and len(c) % 2 == 0:
        raise ValueError(f"Invalid coefficients for dispersion formula {fid}.")
    if fid in (1, 2, 6):  # n0 = 1 + C0, pairs (B, C); C ** 2 for the Sellmeier form
        out = [f1(1 + c[0])]
        for i in range(1, len(c), 2):
            out += [f1(c[i]), f1(c[i + 1] ** 2 if fid == 1 else c[i + 1])]
    elif fid == 4:
        if len(c) < 9 or len(c) % 2 == 0:
            raise ValueError("Invalid coefficients for dispersion formula 4.")
        out = [f1(c[0]), f1(c[1]), f1(c[2]), f1(c[3] ** c[4]), f1(c[5]), f1(c[6]),
               f1(c[7] ** c[8])] + [f1(v) for v in c[9:]]
    elif fid == 8 and len(c) != 4:
        raise ValueError("Invalid coefficients for dispersion formula 8.")
    else:  # 3, 5, 7, 8, 9: the coefficients as they are
        out = [f1(v) for v in c]
    return fid, out, kw, kv, 0.0, 0.0


def configure_material(spec):
    """surfaces/factories/material_factory.py:64-90 (_configure_post_material)."""
    if isinstance(spec, BaseMaterial):
        return spec
    if isinstance(spec, tuple):
        return Material(name=spec[0], reference=spec[1])
    if isinstance(spec, str):
        if spec.lower() == "air":
            return IdealMaterial(n=1.0, k=0.0)
        if spec.lower() == "mirror":
            return None
        return Material(spec)
    raise ValueError(f"Unrecognized material specification: {spec}")
