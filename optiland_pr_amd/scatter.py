"""BSDF surface scattering (the reference's optiland/scatter.py) on the trace core.

LambertianBSDF and GaussianBSDF(sigma) are applied inside the fused trace launch, after the
refraction / reflection of their surface (csrc/ort_scatter.h, trace_kernel<F_SCAT>), and
BaseBSDF.scatter(rays, nx, ny, nz) runs the same step on its own (ort_bsdf_scatter).

The deliberate difference from the reference: it draws from Numba's global generator, so no
two of its traces agree. Here the two uniforms of every (ray, surface, attempt) are one
Philox4x32-10 block keyed by Optic.scatter_seed, so the same seed gives the same trace --
bit for bit under any launch shape, any split of a batch (ray_offset) and a Newton verify
round's re-trace. philox4x32 and bsdf_uniforms restate the stream in NumPy.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi, _native
from ._calls import addr

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None

DEFAULT_MAX_ATTEMPTS = 1024
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


class ScatterAttemptsError(ValueError):
    """ORT_STATUS_SCATTER_ATTEMPTS: a ray's rejection loop used up max_attempts draws."""


def philox4x32(counter, key):
    """Philox4x32-10 of counter [..., 4] and key [..., 2] (uint32 words; broadcast over the
    leading axes) -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        kk0 = (k0 + np.uint64((_W0 * r) & 0xFFFFFFFF)) & _MASK
        kk1 = (k1 + np.uint64((_W1 * r) & 0xFFFFFFFF)) & _MASK
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ kk0, p1 & _MASK,
                          (p0 >> np.uint64(32)) ^ c3 ^ kk1, p0 & _MASK)
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def _uniform(hi, lo):
    m = ((hi.astype(np.uint64) >> np.uint64(5)) << np.uint64(26)) | \
        (lo.astype(np.uint64) >> np.uint64(6))
    return (m + np.uint64(1)).astype(np.float64) * 2.0 ** -53


def words_to_uniforms(o):
    """(u1, u2) in (0, 1] of output words [..., 4]: 53 bits each, exact in float64."""
    o = np.asarray(o, dtype=np.uint32)
    return _uniform(o[..., 0], o[..., 1]), _uniform(o[..., 2], o[..., 3])


def bsdf_uniforms(seed, ray, surface, attempt):
    """The two uniforms the trace core draws for `ray` (its index in the batch plus the ray
    offset) at traced surface `surface` (0-based index in the lowered lens, i.e. the
    Optic's surface number minus one) in rejection round `attempt`; arrays broadcast."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ray = np.asarray(ray, dtype=np.uint64)
    ray, surface, attempt = np.broadcast_arrays(ray, np.asarray(surface, dtype=np.uint64),
                                                np.asarray(attempt, dtype=np.uint64))
    ctr = np.stack([ray & _MASK, ray >> np.uint64(32), surface, attempt], axis=-1)
    return words_to_uniforms(philox4x32(ctr, [seed & 0xFFFFFFFF, seed >> 32]))


class BaseBSDF:
    """scatter.py:138-209."""

    _registry: dict = {}
    kind = _abi.BSDF_NONE

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        BaseBSDF._registry[cls.__name__] = cls

    def lower(self):
        """-> (ort_bsdf.kind, ort_bsdf.sigma)."""
        return self.kind, float(getattr(self, "sigma", 0.0))

    def scatter(self, rays, nx, ny, nz, seed=0, surface_index=0, ray_offset=0,
                max_attempts=DEFAULT_MAX_ATTEMPTS):
        """scatter.py:158-194: rays.L, M, N replaced by the scattered directions about the
        normals (scalars or one per ray), on the rays' device (HIP kernel, or the host
        build for CPU tensors). Ray r draws as bsdf_uniforms(seed, r + ray_offset,
        surface_index, attempt)."""
        n = rays.L.numel()
        dev = rays.L.device
        nrm = [torch.as_tensor(v, dtype=torch.float64, device=dev).expand(n).contiguous()
               if not torch.is_tensor(v) or v.numel() != n
               else v.to(device=dev, dtype=torch.float64).contiguous() for v in (nx, ny, nz)]
        outs = bsdf_scatter(rays.L, rays.M, rays.N, *nrm, self, seed=seed,
                            surface_index=surface_index, ray_offset=ray_offset,
                            max_attempts=max_attempts)
        rays.L, rays.M, rays.N = outs
        return rays

    def to_dict(self):
        return {"type": type(self).__name__}

    @classmethod
    def from_dict(cls, data):
        return cls._registry[data["type"]].from_dict(data)

    def __repr__(self):
        return f"{type(self).__name__}()"


class LambertianBSDF(BaseBSDF):
    """scatter.py:212-236: a uniform point of the unit disk."""

    kind = _abi.BSDF_LAMBERTIAN

    @classmethod
    def from_dict(cls, data):
        return cls()


class GaussianBSDF(BaseBSDF):
    """scatter.py:239-265: a 2-D Gaussian of standard deviation sigma (Box-Muller)."""

    kind = _abi.BSDF_GAUSSIAN

    def __init__(self, sigma):
        self.sigma = float(sigma)

    def to_dict(self):
        return {"type": "GaussianBSDF", "sigma": self.sigma}

    @classmethod
    def from_dict(cls, data):
        return cls(data["sigma"])

    def __repr__(self):
        return f"GaussianBSDF(sigma={self.sigma!r})"


def has_bsdf(optic_or_group):
    sg = getattr(optic_or_group, "surface_group", optic_or_group)
    return any(getattr(s, "bsdf", None) is not None for s in sg.surfaces)


def settings_of(host):
    """(seed, max_attempts) of an Optic (or anything with those attributes; defaults)."""
    seed = int(getattr(host, "scatter_seed", 0))
    cap = int(getattr(host, "scatter_max_attempts", DEFAULT_MAX_ATTEMPTS))
    if not 0 <= seed < 2 ** 64:
        raise ValueError("scatter_seed must be an unsigned 64-bit integer")
    if not 1 <= cap < 2 ** 31:
        raise ValueError("scatter_max_attempts must be at least 1")
    return seed, cap


def scatter_struct(lens, ray_offset=0):
    """ort_scatter of a DeviceLens / HostLens whose table has BSDF surfaces: the lens's
    (seed, max_attempts) (lens.scatter; the defaults without) and its BSDF records on the
    lens's device. Returns the struct and the tensor it points to (keep it alive)."""
    seed, cap = getattr(lens, "scatter", (0, DEFAULT_MAX_ATTEMPTS))
    if ray_offset < 0:
        raise ValueError("ray_offset must be >= 0")
    tab = lens.resident("bsdf", np.ascontiguousarray(lens.table.bsdf).view(np.uint8))
    return _native.ort_scatter(seed, int(ray_offset), cap, 0, addr(tab)), tab


def describe(table):
    """The table's scattering surfaces, by the Optic's surface numbers."""
    out = []
    for si, row in enumerate(table.bsdf):
        if row["kind"] == _abi.BSDF_GAUSSIAN:
            out.append(f"surface {si + 1} (GaussianBSDF, sigma={float(row['sigma'])!r})")
        elif row["kind"] == _abi.BSDF_LAMBERTIAN:
            out.append(f"surface {si + 1} (LambertianBSDF)")
    return ", ".join(out)


def attempts_error(what, max_attempts):
    return ScatterAttemptsError(
        f"BSDF scattering: a ray was rejected {max_attempts} times (scatter_max_attempts) at "
        f"{what}; its direction is NaN. A Lambertian draw is accepted with probability >= "
        "0.39, so this means a sigma far too large for a direction cosine.")


def bsdf_scatter(L, M, N, nx, ny, nz, bsdf, seed=0, surface_index=0, ray_offset=0,
                 max_attempts=DEFAULT_MAX_ATTEMPTS, check=True):
    """ort_bsdf_scatter / ort_host_bsdf_scatter by the tensors' device: the scattered
    (L, M, N) of n directions and normals (float64 tensors of one device). check=False:
    rays that used up max_attempts stay NaN without the ScatterAttemptsError."""
    dev = L.device
    n = L.numel()
    ins = [t.detach().to(device=dev, dtype=torch.float64).contiguous().reshape(-1)
           for t in (L, M, N, nx, ny, nz)]
    if any(t.numel() != n for t in ins):
        raise ValueError("bsdf_scatter: L, M, N, nx, ny, nz must hold one value per ray")
    kind, sigma = bsdf.lower()
    rec = np.zeros(1, dtype=_abi.BSDF)
    rec[0] = (kind, 0, sigma)
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be an unsigned 64-bit integer")
    sc = _native.ort_scatter(seed, int(ray_offset), int(max_attempts), 0, None)
    outs = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3)]
    if dev.type == "cpu":
        status = np.zeros(1, dtype=np.int32)
        rc = _native.load_host().ort_host_bsdf_scatter(
            *(addr(t) for t in ins), n, int(surface_index), addr(rec), C.byref(sc),
            *(addr(t) for t in outs), addr(status))
        _native.check(rc, "ort_host_bsdf_scatter")
        st = int(status[0])
    else:
        from .raytrace import _stream_handle

        status = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = _native.load().ort_bsdf_scatter(
            *(addr(t) for t in ins), n, int(surface_index), addr(rec), C.byref(sc),
            *(addr(t) for t in outs), addr(status), _stream_handle())
        _native.check(rc, "ort_bsdf_scatter")
        st = int(status.item())
    if check and st & _abi.STATUS_SCATTER_ATTEMPTS:
        raise attempts_error(f"surface index {int(surface_index)} ({bsdf!r})", max_attempts)
    return outs
