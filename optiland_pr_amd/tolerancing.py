"""Tolerancing: the reference's optiland/tolerancing interface (core.py, perturbation.py,
sensitivity_analysis.py, monte_carlo.py) on the lens-ensemble trace.

The reference loops over trials: reset, perturbation.apply(), evaluate the operands. Each
trial traces a few hundred rays through one slightly different lens, which on a GPU is one
launch-latency-bound trace, three reduction launches and a device-to-host read per operand.
run(..., batched=True) instead draws every trial's values first (trial-major, perturbation
order within a trial: every sampler's stream is the sequential loop's), applies each trial to
the Optic and lowers it once (lower_surface_group, segment_params: per variant, so the rays
are the loop's bit for bit), stacks the tables ([V][S] surface records, [V][n_lambda][S]
optics rows, per-variant frame ops and ray-generation scalars) and traces all variants of
all operands that share (num_rays, distribution) in ONE ort_trace_ensemble launch, whose
stats rows are read back once.

Samplers, Perturbation, Tolerancing, SensitivityAnalysis and MonteCarlo mirror the
reference's classes; compensators (scipy) and the view_* plots are not part of this module.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi, _calls, _native
from .lowering import lower_apodization, lower_surface_group, pupil_scalars, segment_params

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None


# --------------------------------------------------------------------------------------
# samplers (tolerancing/perturbation.py:20-132)
# --------------------------------------------------------------------------------------
class BaseSampler:
    def sample(self):  # pragma: no cover
        raise NotImplementedError


class ScalarSampler(BaseSampler):
    """Always the same value."""

    def __init__(self, value):
        self.value = value
        self.size = 1

    def sample(self):
        return self.value


class RangeSampler(BaseSampler):
    """numpy.linspace(start, end, steps), one value per sample(), wrapping around."""

    def __init__(self, start, end, steps):
        self.values = np.linspace(start, end, steps)
        self.index = 0
        self.size = steps

    def sample(self):
        if self.index >= len(self.values):
            self.index = 0  # loop over values
        value = self.values[self.index]
        self.index += 1
        return value


class DistributionSampler(BaseSampler):
    """One scalar per sample() from numpy.random.default_rng(seed): "normal" (loc, scale) or
    "uniform" (low, high), drawn as the reference's NumPy backend draws them
    (backend/numpy_backend.py random_normal / random_uniform: generator.normal(loc, scale,
    None), generator.uniform(low, high, None))."""

    def __init__(self, distribution, seed=None, **params):
        self.generator = np.random.default_rng(seed)
        self.distribution = distribution
        self.params = params
        for param in params:
            if param not in ("loc", "scale", "low", "high"):
                raise ValueError(f"Invalid parameter: {param}")

    def sample(self):
        if self.distribution == "normal":
            return self.generator.normal(self.params.get("loc", 0.0),
                                         self.params.get("scale", 1.0), None)
        if self.distribution == "uniform":
            return self.generator.uniform(self.params.get("low", 0.0),
                                          self.params.get("high", 1.0), None)
        raise ValueError(f"Unknown distribution: {self.distribution}")


# --------------------------------------------------------------------------------------
# variables (optimization/variable/*.py with the IdentityScaler a Perturbation gives them)
# --------------------------------------------------------------------------------------
class _Variable:
    label = ""

    def __init__(self, optic, surface_number, **kwargs):
        self.optic = optic
        self.surface_number = surface_number

    @property
    def _surface(self):
        return self.optic.surface_group.surfaces[self.surface_number]

    def __str__(self):
        return f"{self.label}, Surface {self.surface_number}"


class RadiusVariable(_Variable):
    label = "Radius of Curvature"

    def get_value(self):
        return self.optic.surface_group.radii[self.surface_number]

    def update_value(self, v):
        self.optic.set_radius(v, self.surface_number)


class ConicVariable(_Variable):
    label = "Conic Constant"

    def get_value(self):
        return self._surface.geometry.k

    def update_value(self, v):
        self.optic.set_conic(v, self.surface_number)


class ThicknessVariable(_Variable):
    label = "Thickness"

    def get_value(self):
        t = self.optic.surface_group.positions
        return (t[self.surface_number + 1] - t[self.surface_number])[0]

    def update_value(self, v):
        self.optic.set_thickness(v, self.surface_number)


class _AxisVariable(_Variable):
    axes = ()
    kind = ""

    def __init__(self, optic, surface_number, axis=None, **kwargs):
        super().__init__(optic, surface_number)
        self.axis = axis
        if axis not in self.axes:
            raise ValueError(f'Invalid axis "{axis}" for {self.kind} variable.')

    def get_value(self):
        return getattr(self._surface.geometry.cs, self.attr)

    def update_value(self, v):
        setattr(self._surface.geometry.cs, self.attr, float(v))

    def __str__(self):
        return f"{self.label} {self.axis.upper()}, Surface {self.surface_number}"


class TiltVariable(_AxisVariable):
    label, kind, axes = "Tilt", "tilt", ("x", "y")

    @property
    def attr(self):
        return "r" + self.axis


class DecenterVariable(_AxisVariable):
    label, kind, axes = "Decenter", "decenter", ("x", "y", "z")

    @property
    def attr(self):
        return self.axis


class IndexVariable(_Variable):
    """The index after a surface at one wavelength; an update replaces the surface's post
    material with an ideal one (optic_updater.py:87-98)."""

    label = "Refractive Index"

    def __init__(self, optic, surface_number, wavelength=None, **kwargs):
        super().__init__(optic, surface_number)
        if wavelength is None:
            raise TypeError("the index variable needs wavelength=")
        self.wavelength = wavelength

    def get_value(self):
        return self.optic.n(self.wavelength)[self.surface_number]

    def update_value(self, v):
        from .materials import IdealMaterial

        self._surface.material_post = IdealMaterial(n=float(v), k=0)


VARIABLE_TYPES = {"radius": RadiusVariable, "conic": ConicVariable,
                  "thickness": ThicknessVariable, "tilt": TiltVariable,
                  "decenter": DecenterVariable, "index": IndexVariable}


class Variable:
    """optimization/variable/variable.py with the identity scaler: value, update, reset (to
    the value at construction) and the reference's str()."""

    def __init__(self, optic, type_name, **kwargs):
        cls = VARIABLE_TYPES.get(type_name)
        if cls is None:
            raise ValueError(f'Invalid variable type "{type_name}"')
        self.optic = optic
        self.type = type_name
        self.variable = cls(optic, **kwargs)
        self.initial_value = self.value

    @property
    def value(self):
        return self.variable.get_value()

    def update(self, new_value):
        self.variable.update_value(new_value)

    def reset(self):
        self.update(self.initial_value)

    def __str__(self):
        return str(self.variable)


class Perturbation:
    """tolerancing/perturbation.py:135-175: a sampled value REPLACES the parameter."""

    def __init__(self, optic, variable_type, sampler, **kwargs):
        self.optic = optic
        self.type = variable_type
        self.sampler = sampler
        self.variable = Variable(optic, variable_type, **kwargs)
        self.value = None

    def apply(self):
        self.set(self.sampler.sample())

    def set(self, value):
        """Apply a value drawn earlier (the batched runs draw every trial's first)."""
        self.value = value
        self.variable.update(value)

    def reset(self):
        self.variable.reset()
        self.value = self.variable.variable.get_value()


# --------------------------------------------------------------------------------------
# operands
# --------------------------------------------------------------------------------------
def _is_image(optic, surface_number):
    return surface_number in (-1, len(optic.surface_group.surfaces) - 1)


def _pupil_points(distribution, num_rays):
    """The reference's pupil points (NumPy, host) of a distribution name or object."""
    from .distribution import create_distribution

    d = distribution
    if isinstance(d, str):
        d = create_distribution(d)
        d.generate_points(num_rays)
    return (np.ascontiguousarray(d.x, dtype=np.float64),
            np.ascontiguousarray(d.y, dtype=np.float64))


# (the name tests/test_gpu_ensemble.py and tools/ensemble_rate.py upload their segments with)
_bytes_tensor = _calls.bytes_tensor


def image_points_host(optic, surface_number, Hx, Hy, num_rays, wavelength,
                      distribution="hexapolar"):
    """The image points (x, y) RayOperand.rms_spot_size reduces, traced on the host build
    (liboptiland_host.so): the image surface and one wavelength."""
    from . import host

    if wavelength == "all" or not _is_image(optic, surface_number):
        raise NotImplementedError("the host build evaluates rms_spot_size on the image surface "
                                  "at one wavelength")
    table = lower_surface_group(optic.surface_group, [wavelength])
    table.apod = lower_apodization(optic)
    EPL, EPD = pupil_scalars(optic)
    seg = _calls.bytes_tensor(np.stack([segment_params(optic, float(Hx), float(Hy), 0, EPL, EPD)]))
    px, py = (torch.from_numpy(v) for v in _pupil_points(distribution, num_rays))
    apod = None if table.apod is None else _calls.bytes_tensor(table.apod)
    n = px.numel()
    outs, _ = host.trace_pupil(host.HostLens(table), seg, px, py, n, n, False, apod=apod)
    return outs[0], outs[1]


def _rms_spot_host(**input_data):
    """RayOperand.rms_spot_size on the host build (ort_host_rms_spot of image_points_host)."""
    from . import host

    return float(host.rms_spot(*image_points_host(**input_data))[0])


class Operand:
    """optimization/operand/operand.py as far as tolerancing uses it: a value and a name."""

    def __init__(self, operand_type, target, min_val, max_val, weight, input_data, device=None):
        if operand_type != "rms_spot_size":
            raise ValueError(f'operand type "{operand_type}" is not supported by '
                             'tolerancing (supported: "rms_spot_size")')
        self.operand_type = operand_type
        self.target = target
        self.min_val = min_val
        self.max_val = max_val
        self.weight = weight
        self.input_data = input_data
        self.device = device

    @property
    def value(self):
        if self.device is not None and torch.device(self.device).type == "cpu":
            return _rms_spot_host(**self.input_data)
        from .operands import RayOperand

        return float(RayOperand.rms_spot_size(**self.input_data))

    def __str__(self):
        return self.operand_type.replace("_", " ")


# --------------------------------------------------------------------------------------
# the lens ensemble: V lowered variants stacked for ort_trace_ensemble
# --------------------------------------------------------------------------------------
class UnsupportedEnsemble(ValueError):
    """The variants cannot go through ort_trace_ensemble (the per-trial loop serves)."""


class EnsembleTable:
    """V LensTables of one lens stacked as ort_trace_ensemble reads them (include/
    optiland_rt.h): surfaces [V][S], optics [V][n_lambda][S], n_tab / alpha_tab
    [V][n_lambda][n_mat], cs_ops [V][cs_stride] (a variant's offsets relative to its own
    block), final_thickness [V]; coef, zern, the material records and the wavelengths are
    variant 0's, shared. frame_flags and form_flags are ANDed over the variants (one tilted
    variant makes the ensemble non-axial). Raises UnsupportedEnsemble for lenses outside the
    entry point's scope or variants that do not stack."""

    def __init__(self, tables):
        t0 = tables[0]
        V, S = len(tables), t0.n_surfaces
        ok_geom = (1 << _abi.GEOM_PLANE) | (1 << _abi.GEOM_STANDARD)
        n_mat = max(t.n_tab.shape[1] for t in tables)
        n_lambda = t0.n_tab.shape[0]
        stride = max(len(t.cs_ops) for t in tables)
        self.surfaces = np.zeros((V, S), dtype=_abi.SURFACE)
        self.optics = np.zeros((V, n_lambda, S), dtype=_abi.SURFACE_OPTICS)
        self.n_tab = np.zeros((V, n_lambda, n_mat))
        self.alpha_tab = np.zeros((V, n_lambda, n_mat))
        self.cs_ops = np.zeros((V, stride), dtype=_abi.CS_OP)
        self.final_thickness = np.zeros(V)
        frame, form, mask = ~0, ~0, 0
        for v, t in enumerate(tables):
            if t.n_surfaces != S or t.n_tab.shape[0] != n_lambda:
                raise UnsupportedEnsemble("the variants differ in surfaces or wavelengths")
            for g in np.unique(t.surfaces["geometry"]):
                mask |= 1 << int(g)
            if mask & ~ok_geom or t.interaction_mask & ~(1 << _abi.IA_REFRACT_REFLECT):
                raise UnsupportedEnsemble("only plane / standard surfaces with refractive or "
                                          "reflective interactions trace as an ensemble")
            if t.has_bsdf or (t.coatings is not None
                              and np.any(t.coatings["kind"] != _abi.COAT_NONE)):
                raise UnsupportedEnsemble("BSDF surfaces and coatings trace one lens at a time")
            if t.n_rec or t.final_mat < 0:
                raise UnsupportedEnsemble("recorded surfaces trace one lens at a time")
            surf, n_t, a_t = t.surfaces.copy(), t.n_tab, t.alpha_tab
            if t.final_mat != t0.final_mat:
                # final_mat is one value per launch: this variant's image-space medium moves
                # to variant 0's column (the columns swapped, the surfaces' ids with them)
                f, f0 = t.final_mat, t0.final_mat
                if f0 >= n_t.shape[1]:
                    raise UnsupportedEnsemble("the variants' material tables do not align")
                perm = np.arange(n_t.shape[1])
                perm[[f, f0]] = perm[[f0, f]]
                n_t, a_t = n_t[:, perm], a_t[:, perm]
                for col in ("mat_pre", "mat_post"):
                    surf[col] = perm[surf[col]]
            # aperture programs live in the shared coef: every variant's must be variant 0's
            prog = (surf["flags"] & _abi.SURF_APERTURE_PROG) != 0
            for o, ln in zip(surf["ap_off"][prog], surf["ap_len"][prog], strict=True):
                if o + ln > len(t0.coef) or not np.array_equal(t.coef[o:o + ln],
                                                               t0.coef[o:o + ln]):
                    raise UnsupportedEnsemble("the variants' aperture programs differ")
            self.surfaces[v] = surf
            self.n_tab[v, :, :n_t.shape[1]] = n_t
            self.alpha_tab[v, :, :n_t.shape[1]] = a_t
            self.cs_ops[v, :len(t.cs_ops)] = t.cs_ops
            self.final_thickness[v] = t.final_thickness
            frame &= t.frame_flags
            form &= t.form_flags
        pre, post = self.surfaces["mat_pre"], self.surfaces["mat_post"]
        for v in range(V):  # LensTable.optics, per variant, from the stacked tables
            o = self.optics[v]
            o["n_pre"] = self.n_tab[v][:, pre[v]]
            o["n_post"] = self.n_tab[v][:, post[v]]
            o["u"] = o["n_pre"] / o["n_post"]
            o["alpha_pre"] = self.alpha_tab[v][:, pre[v]]
            o["u_sq"] = o["u"] * o["u"]
        self.n_variants, self.n_surfaces, self.n_lambda, self.n_mat = V, S, n_lambda, n_mat
        self.cs_stride = stride
        self.final_mat = int(t0.final_mat)
        self.geometry_mask = mask
        self.interaction_mask = 1 << _abi.IA_REFRACT_REFLECT
        self.frame_flags = frame
        self.form_flags = form if frame & _abi.LENS_PLAIN else 0
        self.coef = np.ascontiguousarray(t0.coef, dtype=np.float64)
        self.zern = t0.zern
        self.mat_table = t0.mat_table if t0.mat_table is not None else np.zeros(1, _abi.MATERIAL)
        self.wavelengths = np.asarray(t0.wavelengths, dtype=np.float64)
        self.apod = t0.apod
        for t in tables:
            same = (t.apod is None) == (t0.apod is None) and (
                t.apod is None or t.apod.tobytes() == t0.apod.tobytes())
            if not same:
                raise UnsupportedEnsemble("the variants' apodizations differ")

    def meta(self, pairs):
        """ops.trace_ensemble's lens_meta."""
        return [self.n_surfaces, self.n_lambda, self.n_mat, self.final_mat, self.geometry_mask,
                self.interaction_mask, self.frame_flags, self.form_flags, self.n_variants,
                int(pairs), self.cs_stride]

    def tensors(self, device):
        """The nine tables in DeviceLens.lens_tensors' order (structured ones as bytes) and
        final_thickness [V], on `device`."""
        def up(a):
            return (_calls.bytes_tensor(a) if a.dtype.fields else
                    torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy())).to(device)

        lens = [up(a) for a in (self.surfaces, self.cs_ops, self.coef, self.zern, self.n_tab,
                                self.alpha_tab, self.optics, self.mat_table, self.wavelengths)]
        return lens, up(self.final_thickness)


def trace_ensemble(lens, meta, final_thickness, seg, apod, px, py, want_rays=False):
    """ort_trace_ensemble on device tensors (EnsembleTable.tensors / .meta): stats
    [V][P][5] and, with want_rays, the rays [8][V * P * n_pupil] (else None)."""
    (S, n_lambda, n_mat, final_mat, gmask, imask, frame, form, V, P, stride) = meta
    dev = px.device
    if dev.type != "cuda":
        raise RuntimeError("ort_trace_ensemble runs on the GPU; the host build traces one "
                           "lens per call (there is no fallback between them)")
    lib = _native.load()
    n_pupil = int(px.numel())
    lens_c = _native.ort_lens(*(t.data_ptr() for t in lens[:7]), S, n_lambda, n_mat, final_mat,
                              gmask, imask, 0.0, lens[7].data_ptr(), lens[8].data_ptr(), frame,
                              form)
    ens = _native.ort_ensemble(V, P, stride, 0, final_thickness.data_ptr())
    size = int(lib.ort_ensemble_workspace_size(C.byref(ens), n_pupil))
    _native.check(size if size < 0 else 0, "ort_ensemble_workspace_size")
    ws = _calls.workspace("ensemble", dev, size)
    stats = torch.empty((V, P, 5), dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rays = rays_c = None
    if want_rays:
        rays = torch.empty((8, V * P * n_pupil), dtype=torch.float64, device=dev)
        rays_c = C.byref(_calls.rays_struct(list(rays.unbind(0))))
    rc = lib.ort_trace_ensemble(C.byref(lens_c), C.byref(ens), px.data_ptr(), py.data_ptr(),
                                n_pupil, seg.data_ptr(), _calls.addr(apod), rays_c,
                                stats.data_ptr(), ws.data_ptr(), ws.numel(), status.data_ptr(),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "ort_trace_ensemble")
    return stats, rays, status


# --------------------------------------------------------------------------------------
# Tolerancing (tolerancing/core.py)
# --------------------------------------------------------------------------------------
class Tolerancing:
    """Operands (metrics) and perturbations of an Optic. device: None traces on the GPU
    (the default, as Optic.trace); "cpu" evaluates every operand on the host build, one lens
    at a time."""

    def __init__(self, optic, method="generic", tol=1e-5, device=None):
        self.optic = optic
        self.method = method
        self.tol = tol
        self.device = device
        self.operands = []
        self.perturbations = []

    def add_operand(self, operand_type, input_data=None, target=None, weight=1.0, min_val=None,
                    max_val=None):
        op = Operand(operand_type, target, min_val, max_val, weight,
                     {} if input_data is None else input_data, self.device)
        if target is None:
            op.target = op.value
        self.operands.append(op)

    def add_perturbation(self, variable_type, sampler, **kwargs):
        self.perturbations.append(Perturbation(self.optic, variable_type, sampler, **kwargs))

    def add_compensator(self, variable_type, **kwargs):
        raise NotImplementedError("compensators (the reference's scipy CompensatorOptimizer) "
                                  "are not implemented")

    def apply_compensators(self):
        return {}

    def evaluate(self):
        return [float(op.value) for op in self.operands]

    def reset(self):
        for p in self.perturbations:
            p.reset()

    # -- the batched evaluation ------------------------------------------------------------
    def _on_host(self):
        return self.device is not None and torch.device(self.device).type == "cpu"

    def _ensemble_plan(self):
        """Operands grouped by (num_rays, distribution) with each group's distinct (Hx, Hy,
        wavelength) pairs, or None when some operand needs the per-trial loop."""
        groups = {}
        for k, op in enumerate(self.operands):
            d = op.input_data
            dist = d.get("distribution", "hexapolar")
            if (d.get("optic") is not self.optic or d["wavelength"] == "all"
                    or not _is_image(self.optic, d["surface_number"])
                    or not isinstance(dist, str)):
                return None
            pair = (float(d["Hx"]), float(d["Hy"]), float(d["wavelength"]))
            g = groups.setdefault((int(d["num_rays"]), dist), {"pairs": [], "ops": []})
            if pair not in g["pairs"]:
                g["pairs"].append(pair)
            g["ops"].append((k, g["pairs"].index(pair)))
        return groups

    def lower_variant(self, pairs):
        """The Optic as it stands, lowered for the pairs (Hx, Hy, wavelength): its LensTable
        over the pairs' distinct wavelengths and one segment per pair."""
        optic = self.optic
        if getattr(optic, "polarization", "ignore") != "ignore":
            raise UnsupportedEnsemble("a polarization state traces one lens at a time")
        wls = []
        for _, _, w in pairs:
            if w not in wls:
                wls.append(w)
        table = lower_surface_group(optic.surface_group, wls)
        table.apod = lower_apodization(optic)
        EPL, EPD = pupil_scalars(optic)
        segs = np.stack([segment_params(optic, hx, hy, wls.index(w), EPL, EPD)
                         for hx, hy, w in pairs])
        return table, segs

    def evaluate_trials(self, trials, batched=True):
        """Operand values [len(trials)][operands] of the trials, each a list of one value per
        perturbation (None: that perturbation stays at its nominal value): reset, set the
        values, evaluate. batched: every trial through the ensemble launch where the lens,
        the operands and the device allow it, else the per-trial loop of Operand.value. The
        nominal lens is restored at the end. self.timing holds the host seconds spent
        lowering and the mode used."""
        import time

        plan = self._ensemble_plan() if batched and not self._on_host() and trials else None
        out = np.empty((len(trials), len(self.operands)))
        self.timing = {"mode": "loop", "lowering_s": 0.0}

        def apply(values):
            self.reset()
            for p, v in zip(self.perturbations, values, strict=True):
                if v is not None:
                    p.set(v)

        try:
            if plan is not None:
                try:
                    t0 = time.perf_counter()
                    lowered = {key: [] for key in plan}
                    for values in trials:
                        apply(values)
                        for key, g in plan.items():
                            lowered[key].append(self.lower_variant(g["pairs"]))
                    stacked = {key: (EnsembleTable([t for t, _ in lv]),
                                     np.stack([s for _, s in lv]))
                               for key, lv in lowered.items()}
                    self.timing["lowering_s"] = time.perf_counter() - t0
                except UnsupportedEnsemble:
                    plan = None
            if plan is not None:
                from .raytrace import get_device

                dev = get_device()
                results = []
                for key, g in plan.items():
                    ens, segs = stacked[key]
                    px, py = (torch.from_numpy(v).to(dev) for v in _pupil_points(key[1], key[0]))
                    lens, ft = ens.tensors(dev)
                    apod = None if ens.apod is None else _calls.bytes_tensor(ens.apod).to(dev)
                    stats = torch.ops.ort.trace_ensemble(
                        lens, ens.meta(len(g["pairs"])), ft, _calls.bytes_tensor(segs).to(dev), apod,
                        px, py, False)[0]
                    results.append((g, stats))
                for g, stats in results:  # one read-back per launch, after every launch
                    rms = stats.cpu().numpy()[:, :, 3]
                    for k, q in g["ops"]:
                        out[:, k] = rms[:, q]
                self.timing["mode"] = "ensemble"
                return out
            for i, values in enumerate(trials):
                apply(values)
                out[i] = self.evaluate()
            return out
        finally:
            self.reset()


# --------------------------------------------------------------------------------------
# SensitivityAnalysis / MonteCarlo (sensitivity_analysis.py, monte_carlo.py)
# --------------------------------------------------------------------------------------
class SensitivityAnalysis:
    """One perturbation at a time over its RangeSampler. results: a dict of columns in the
    reference's DataFrame order -- perturbation_type (str), perturbation_value, then
    "{i}: {operand}" -- every numeric column a float64 array."""

    def __init__(self, tolerancing):
        self.tolerancing = tolerancing
        self.operand_names = [f"{i}: {op}" for i, op in enumerate(tolerancing.operands)]
        self.results = {}
        self._validate()

    def _columns(self, head, values):
        cols = dict(head)
        for k, name in enumerate(self.operand_names):
            cols[name] = np.ascontiguousarray(values[:, k], dtype=np.float64)
        self.results = cols

    def run(self, batched=True):
        t = self.tolerancing
        types, trials = [], []
        for k, p in enumerate(t.perturbations):
            if not isinstance(p.sampler, RangeSampler):
                raise ValueError("Only range samplers are supported.")
            for _ in range(p.sampler.size):
                values = [None] * len(t.perturbations)
                values[k] = p.sampler.sample()
                types.append(str(p.variable))
                trials.append(values)
        got = t.evaluate_trials(trials, batched)
        pv = np.array([next(v for v in tr if v is not None) for tr in trials], dtype=np.float64)
        self._columns({"perturbation_type": np.array(types, dtype=object),
                       "perturbation_value": pv}, got)

    def get_results(self):
        """A pandas DataFrame of the columns when pandas imports, else the dict."""
        try:
            import pandas as pd
        except ImportError:
            return self.results
        return pd.DataFrame(self.results)

    def _validate(self):
        if not self.tolerancing.operands:
            raise ValueError("No operands found in the tolerancing system.")
        if not self.tolerancing.perturbations:
            raise ValueError("No perturbations found in the tolerancing system.")
        if len(self.tolerancing.operands) > 6:
            raise ValueError("Sensitivity analysis is limited to 6 operands.")
        if len(self.tolerancing.perturbations) > 6:
            raise ValueError("Sensitivity analysis is limited to 6 perturbations.")


class MonteCarlo(SensitivityAnalysis):
    """Every perturbation sampled per trial. results: one column per perturbation (its
    str()), then "{i}: {operand}"."""

    def run(self, num_iterations, batched=True):
        t = self.tolerancing
        # trial-major, perturbation order within a trial: each sampler's sequential stream
        trials = [[p.sampler.sample() for p in t.perturbations] for _ in range(num_iterations)]
        got = t.evaluate_trials(trials, batched)
        head = {}
        for k, p in enumerate(t.perturbations):
            head[str(p.variable)] = np.array([float(tr[k]) for tr in trials], dtype=np.float64)
        self._columns(head, got)

    def _validate(self):
        if not self.tolerancing.operands:
            raise ValueError("No operands found in the tolerancing system.")
        if not self.tolerancing.perturbations:
            raise ValueError("No perturbations found in the tolerancing system.")
