"""Polarization states, coatings and polarized rays.

Mirrors optiland/rays/polarization_state.py, optiland/coatings.py and
optiland/rays/polarized_rays.py: the same class names, constructor arguments, validation,
registry and to_dict / from_dict keys. What a coating does to a ray and the per-surface
update of the polarization matrix run in the trace kernels (csrc/ort_polar.h,
trace_kernel<F_POL>); `PolarizedRays.update_intensity` / `get_output_field` are torch
operations on the tensors the kernel returned, for callers who hold a PolarizedRays.
This module calls no library entry itself: trace_pupil_polarized and
trace_sequential_polarized build the ort_polarization struct, allocate the outputs and hand
both to raytrace.trace_pupil_on / trace_rays_on, which trace on the lens's own library
(raytrace.py for a DeviceLens, host.py for a HostLens).

Reference behaviour kept as it is: a polarized state's intensity
replaces the traced one (apodization, absorption and clipping are lost), an unpolarized
state scales by the *initial* intensity, the Fresnel coefficients use the real index only,
and a surface with a SimpleCoating does not update the polarization matrix.
"""

from __future__ import annotations

import numpy as np

from . import _abi, _native
from ._calls import addr
from .raytrace import RealRays

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None


# --------------------------------------------------------------------------------------
# polarization state (rays/polarization_state.py)
# --------------------------------------------------------------------------------------
class PolarizationState:
    """polarization_state.py:15-80."""

    def __init__(self, is_polarized=False, Ex=None, Ey=None, phase_x=None, phase_y=None):
        if is_polarized:
            if any(v is None for v in (Ex, Ey, phase_x, phase_y)):
                raise ValueError("All parameters must be provided for a polarized state.")
        elif not all(v is None for v in (Ex, Ey, phase_x, phase_y)):
            raise ValueError(
                "Ex, Ey, phase_x, and phase_y must be None for a non-polarized state.")
        self.is_polarized = is_polarized
        self.Ex = np.array(Ex, dtype=np.float64) if Ex is not None else None
        self.Ey = np.array(Ey, dtype=np.float64) if Ey is not None else None
        self.phase_x = np.array(phase_x, dtype=np.float64) if phase_x is not None else None
        self.phase_y = np.array(phase_y, dtype=np.float64) if phase_y is not None else None
        if self.Ex is not None and self.Ey is not None:
            mag = np.sqrt(self.Ex**2 + self.Ey**2)
            self.Ex = self.Ex / mag
            self.Ey = self.Ey / mag

    def __str__(self):
        if self.is_polarized:
            return (f"Polarized Light: Ex: {self.Ex}, Ey: {self.Ey}, "
                    f"Phase x: {self.phase_x}, Phase y: {self.phase_y}")
        return "Unpolarized Light"

    __repr__ = __str__

    def field(self):
        """(Ex e^{i phase_x}, Ey e^{i phase_y}) as the reference forms them
        (polarized_rays.py:177-180)."""
        return (complex(self.Ex * np.exp(1j * self.phase_x)),
                complex(self.Ey * np.exp(1j * self.phase_y)))


def create_polarization(pol_type: str):
    """polarization_state.py:83-149."""
    if pol_type == "unpolarized":
        return PolarizationState(is_polarized=False)
    table = {
        "H": (1, 0, 0, 0),
        "V": (0, 1, 0, 0),
        "L+45": (1, 1, 0, 0),
        "L-45": (1, -1, 0, 0),
        "RCP": (np.sqrt(2) / 2, np.sqrt(2) / 2, 0, -np.pi / 2),
        "LCP": (np.sqrt(2) / 2, np.sqrt(2) / 2, 0, np.pi / 2),
    }
    if pol_type not in table:
        raise ValueError("Invalid polarization type. Must be H, V, L+45, L-45, RCP or LCP.")
    Ex, Ey, px, py = table[pol_type]
    return PolarizationState(is_polarized=True, Ex=Ex, Ey=Ey, phase_x=px, phase_y=py)


# --------------------------------------------------------------------------------------
# coatings (coatings.py)
# --------------------------------------------------------------------------------------
class BaseCoating:
    """coatings.py:21-153: the registry by class name behind from_dict."""

    _registry: dict = {}

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        BaseCoating._registry[cls.__name__] = cls

    def to_dict(self):
        return {"type": type(self).__name__}

    @classmethod
    def from_dict(cls, data):
        return cls._registry[data["type"]].from_dict(data)


class SimpleCoating(BaseCoating):
    """coatings.py:156-255: the intensity times the transmittance (reflective surface:
    the reflectance)."""

    def __init__(self, transmittance, reflectance=0):
        self.transmittance = transmittance
        self.reflectance = reflectance
        self.absorptance = 1 - reflectance - transmittance

    def to_dict(self):
        return {"type": type(self).__name__, "transmittance": self.transmittance,
                "reflectance": self.reflectance}

    @classmethod
    def from_dict(cls, data):
        return cls(data["transmittance"], data["reflectance"])


class BaseCoatingPolarized(BaseCoating):
    """coatings.py:258-342."""


class FresnelCoating(BaseCoatingPolarized):
    """coatings.py:345-394: the Fresnel equations between the coating's two materials."""

    def __init__(self, material_pre, material_post):
        self.material_pre = material_pre
        self.material_post = material_post

    def to_dict(self):
        from .lensio import material_to_dict

        return {"type": type(self).__name__,
                "material_pre": material_to_dict(self.material_pre),
                "material_post": material_to_dict(self.material_post)}

    @classmethod
    def from_dict(cls, data):
        from .lensio import material_from_dict

        return cls(material_from_dict(data["material_pre"]),
                   material_from_dict(data["material_post"]))


def create_coating(coating, material_pre, material_post):
    """surfaces/factories/coating_factory.py:35-60."""
    if isinstance(coating, BaseCoating):
        return coating
    if isinstance(coating, str) and coating.lower() == "fresnel":
        return FresnelCoating(material_pre, material_post)
    return None


def polarization_mode(state, intensity=True):
    """The kernels' mode for Optic.polarization: "ignore" -> IGNORE; a state -> POLARIZED
    / UNPOLARIZED, or MATRICES without the intensity update (trace_generic)."""
    if state == "ignore" or state is None:
        return _abi.POL_IGNORE
    if not isinstance(state, PolarizationState):
        raise ValueError('Invalid polarization state. Must be either PolarizationState or '
                         '"ignore".')
    if not intensity:
        return _abi.POL_MATRICES
    return _abi.POL_POLARIZED if state.is_polarized else _abi.POL_UNPOLARIZED


def polarization_struct(mode, state, coatings_ptr, p_out_ptr, field=None):
    ex = ey = 0j
    if field is not None:
        ex, ey = field
    elif mode == _abi.POL_POLARIZED:
        ex, ey = state.field()
    return _native.ort_polarization(int(mode), 0, ex.real, ex.imag, ey.real, ey.imag,
                                    coatings_ptr, p_out_ptr)


# --------------------------------------------------------------------------------------
# polarized rays (rays/polarized_rays.py)
# --------------------------------------------------------------------------------------
def planes_to_p(planes, n):
    """[18][n] float64 planes (re, im of the nine elements) -> complex128 [n, 3, 3]."""
    return torch.view_as_complex(planes.view(9, 2, n).permute(2, 0, 1).contiguous()).view(n, 3, 3)


class PolarizedRays(RealRays):
    """rays/polarized_rays.py:17-182 on torch tensors: `.p` is complex128 [N, 3, 3]."""

    def __init__(self, x, y, z, L, M, N, intensity, wavelength, device=None):
        super().__init__(x, y, z, L, M, N, intensity, wavelength, device=device)
        n = self.x.numel()
        self.p = torch.eye(3, dtype=torch.complex128, device=self.x.device).repeat(n, 1, 1)
        self._i0 = self.i.clone()
        self._L0, self._M0, self._N0 = self.L.clone(), self.M.clone(), self.N.clone()

    def get_output_field(self, E):
        """polarized_rays.py:56-66: P E per ray, E [N, 3] complex."""
        return torch.matmul(self.p, E.to(torch.complex128).unsqueeze(-1)).squeeze(-1)

    def _get_3d_electric_field(self, state):
        """polarized_rays.py:153-182."""
        k = torch.stack([self._L0, self._M0, self._N0]).T
        x = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64, device=k.device).expand_as(k)
        p = torch.linalg.cross(k, x)
        norms = torch.linalg.norm(p, dim=1)
        if bool((norms == 0).any()):
            raise ValueError("k-vector parallel to x-axis is not currently supported.")
        p = p / norms.unsqueeze(-1)
        s = torch.linalg.cross(p, k)
        ex, ey = state.field()
        return ex * s.to(torch.complex128) + ey * p.to(torch.complex128)

    def update_intensity(self, state):
        """polarized_rays.py:68-108."""
        if state.is_polarized:
            E1 = self.get_output_field(self._get_3d_electric_field(state))
            self.i = torch.sum(torch.abs(E1) ** 2, dim=1)
            return
        sx = PolarizationState(True, 1.0, 0.0, 0.0, 0.0)
        sy = PolarizationState(True, 0.0, 1.0, 0.0, 0.0)
        E1x = self.get_output_field(self._get_3d_electric_field(sx))
        E1y = self.get_output_field(self._get_3d_electric_field(sy))
        self.i = ((torch.sum(torch.abs(E1x) ** 2, dim=1)
                   + torch.sum(torch.abs(E1y) ** 2, dim=1)) * self._i0 / 2)


# --------------------------------------------------------------------------------------
# the polarized trace of an Optic (ray_generator.py:99-105, real_ray_tracer.py:37-133)
# --------------------------------------------------------------------------------------
def needs_polarized_trace(optic):
    """A state is set or some surface has a coating: the F_POL kernel family traces it."""
    sg = optic.surface_group
    return optic.polarization != "ignore" or any(
        getattr(getattr(s, "interaction_model", None), "coating", None) is not None
        for s in sg.surfaces)


def check_polarization(optic):
    """ray_generator.py:99-104."""
    if optic.polarization == "ignore" and optic.surface_group.uses_polarization:
        raise ValueError("Polarization must be set when surfaces have "
                         "polarization-dependent coatings.")


def _coatings_of(lens):
    return lens.resident("coatings", np.ascontiguousarray(lens.table.coatings).view(np.uint8))


def trace_pupil_polarized(lens, segs, px, py, n, seg_len, mode, state, pupil_per_ray=False,
                          rec=None, want_p=True, keys=(), newton_mode="reference",
                          field=None, coat=None, apod="lens", outs=None, planes=None):
    """Generate and trace with coatings / polarization: `lens` a raytrace.DeviceLens (HIP)
    or a host.HostLens (the host build). Returns the 8 ray tensors and the [18][n] planes
    of P (None without want_p). field: (ex, ey) complex instead of `state`; coat / apod:
    the COATING / APODIZATION records as uint8 tensors on the lens's device instead of the
    lens's own (the custom op hands them over as tensors); outs / planes: preallocated
    outputs (8 tensors of n, one of 18 n)."""
    from . import raytrace

    dev = lens.device
    if outs is None:
        outs = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(8)]
    if planes is None and want_p:
        planes = torch.empty(18 * n, dtype=torch.float64, device=dev)
    if coat is None:
        coat = _coatings_of(lens)
    if isinstance(apod, str):
        apod = lens.apod
    # (coat, planes and apod stay referenced here until the launch is enqueued)
    pol = polarization_struct(mode, state, addr(coat), addr(planes), field)
    raytrace.trace_pupil_on(lens, segs, px, py, outs, n, seg_len, pupil_per_ray, rec, keys,
                            newton_mode, pol=pol, apod=apod)
    return outs, planes


def trace_sequential_polarized(lens, rays_in, mode, state, rec=None, want_p=True,
                               start_surface=0, newton_mode="reference"):
    """ort_trace_sequential_polarized / its host build: resident rays (8 tensors) traced
    with P started from the identity and the incoming direction as the initial one."""
    from . import raytrace

    dev = lens.device
    n = rays_in[0].numel()
    outs = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(8)]
    planes = torch.empty(18 * n, dtype=torch.float64, device=dev) if want_p else None
    coat = _coatings_of(lens)  # (with planes: referenced until the launch is enqueued)
    pol = polarization_struct(mode, state, addr(coat), addr(planes))
    raytrace.trace_rays_on(lens, rays_in, outs, start_surface, rec, newton_mode, pol=pol)
    return outs, planes


def trace(optic, Hx, Hy, wavelength, num_rays=100, distribution="hexapolar", device=None):
    """Optic.trace of a coated or polarized lens on `device`: None for the GPU (what
    Optic.trace itself does), "cpu" for the host build of the kernels' code."""
    from .raytrace import RealRayTracer

    Hx, Hy = np.broadcast_arrays(np.atleast_1d(np.asarray(Hx, dtype=np.float64)),
                                 np.atleast_1d(np.asarray(Hy, dtype=np.float64)))
    return RealRayTracer(optic)._trace_polarized(Hx, Hy, wavelength, num_rays, distribution,
                                                 device)


def trace_generic(optic, Hx, Hy, Px, Py, wavelength, device=None):
    """Optic.trace_generic of a coated or polarized lens on `device` (see trace)."""
    from .raytrace import RealRayTracer

    return RealRayTracer(optic).trace_generic(Hx, Hy, Px, Py, wavelength, _device=device)


def lens_of(optic, wavelength, record, device=None):
    """The lowered lens of a coated / polarized Optic on `device`: a cached DeviceLens
    (raytrace.lens_for) or, for the CPU, a HostLens."""
    from . import raytrace
    from .lowering import lower_apodization, lower_surface_group

    if device is not None and torch.device(device).type == "cpu":
        from .host import HostLens

        table = lower_surface_group(optic.surface_group, [wavelength], record=record,
                                    polarized=True)
        table.apod = lower_apodization(optic)
        return HostLens(table)
    return raytrace.lens_for(optic, [wavelength], record=record, polarized=True)


def trace_optic(optic, segs, px, py, n, seg_len, wavelength, pupil_per_ray, intensity, keys,
                newton_mode="reference", device=None):
    """RealRayTracer.trace / trace_generic of a coated or polarized Optic: PolarizedRays
    when a state is set (with .i per the state when `intensity`), plain RealRays with the
    coatings' intensity factors for "ignore"; the surface records as the tracer fills
    them, the image row's intensity being the returned one (real_ray_tracer.py:94-95)."""
    from . import raytrace

    check_polarization(optic)
    sg = optic.surface_group
    record = sg.record == "all"
    n_traced = len(sg.surfaces) - 1
    lens = lens_of(optic, wavelength, True if record else [n_traced - 1], device)
    dev = lens.device
    px = px.to(dev)
    py = py.to(dev)
    state = optic.polarization
    mode = polarization_mode(state, intensity)
    rec = torch.empty(lens.table.n_rec * 8 * n, dtype=torch.float64, device=dev)
    polarized = mode != _abi.POL_IGNORE
    outs, planes = trace_pupil_polarized(lens, segs, px, py, n, seg_len, mode, state,
                                         pupil_per_ray=pupil_per_ray, rec=rec,
                                         want_p=polarized, keys=keys, newton_mode=newton_mode)
    out = (PolarizedRays if polarized else RealRays).of(
        outs, torch.full((n,), float(wavelength), dtype=torch.float64, device=dev))
    rays0 = None
    if record or polarized:
        # the generated rays themselves (the object-surface record, PolarizedRays._L0 ...)
        rays0 = RealRays.empty(n, 0.0, device=dev)
        raytrace.generate_rays(segs, px, py, rays0, n, seg_len, pupil_per_ray, apod=lens.apod)
    if polarized:
        out.p = planes_to_p(planes, n)
        out._i0, out._L0, out._M0, out._N0 = rays0.i, rays0.L, rays0.M, rays0.N
    if not record:
        sg.reset()
        rays0 = None
    # the image row is the image surface's own record, before update_intensity: the
    # tracer's surface_group.intensity[-1, :] = rays.i writes into a temporary stack
    # (real_ray_tracer.py:94-95)
    raytrace._record_into(sg, rec, n, lens.table.rec_surfaces, rays0)
    return out
