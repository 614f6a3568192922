"""Host (CPU) side of the trace core: the CPU dispatch key of torch.ops.ort.trace_sequential
and of its VJP (include/optiland_host.h, liboptiland_host.so).

The reference runs its torch backend on the CPU by default (backend/torch_backend.py:66-77)
and its own tests force it there (tests/conftest.py:5-19), so `SurfaceGroup.trace`
(surfaces/surface_group.py:232-244) reaches the op with CPU tensors as often as with device
ones. A HostLens is the lowered lens in host memory (the same LensTable bytes a DeviceLens
uploads); the calls below hand host pointers to the C ABI of the host library, which runs
the GPU kernels' per-ray source compiled with g++ (csrc/ort_host.cpp). This is not a
fallback of the device path: device tensors never come here, and host tensors never reach
the HIP library.

trace_pupil and trace_sequential are the only callers of the host library's six forward
entries (plain, polarized, scatter), through _calls.FORWARD / call_forward and the one
status path _calls.raise_status; raytrace.py is their counterpart for the device library.
The scatter struct comes from the lens, a polarization struct from the caller
(polarization.py).
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _abi, _calls, _native
from ._calls import addr, rays_struct

_rays_c = rays_struct  # (the name tests/test_polarization_cpu.py builds its structs with)


class HostLens:
    """A LensTable held in host memory for liboptiland_host.so (the counterpart of
    raytrace.DeviceLens for CPU tensors)."""

    def __init__(self, table):
        self.table = table
        self.device = torch.device("cpu")
        keep = []

        def arr(a, dtype=None):
            a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))
            keep.append(a)
            return a

        surfaces = arr(table.surfaces)
        cs_ops = arr(table.cs_ops)
        coef = arr(table.coef, np.float64)
        zern = arr(table.zern)
        n_tab = arr(table.n_tab, np.float64)
        alpha_tab = arr(table.alpha_tab, np.float64)
        optics = arr(table.optics)
        mats = arr(table.mat_table if table.mat_table is not None else np.zeros(1, _abi.MATERIAL))
        lambdas = arr(np.asarray(table.wavelengths, dtype=np.float64))
        mask = 0
        for g in np.unique(table.surfaces["geometry"]):
            mask |= 1 << int(g)
        self.geometry_mask = mask
        self.c = _native.ort_lens(
            addr(surfaces), addr(cs_ops), addr(coef), addr(zern), addr(n_tab), addr(alpha_tab), addr(optics),
            table.n_surfaces, len(table.wavelengths), table.n_tab.shape[1], table.final_mat,
            mask, table.interaction_mask, table.final_thickness, addr(mats), addr(lambdas),
            table.frame_flags, table.form_flags)
        self._keep = keep
        # the same nine tables as torch CPU tensors sharing these arrays' memory (the lens as
        # the torch ops take it: ops.lens_args)
        self._tensors = [torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a)
                         for a in (surfaces, cs_ops, coef, zern, n_tab.reshape(-1),
                                   alpha_tab.reshape(-1), optics.reshape(-1), mats, lambdas)]
        # the pupil apodization record (ort_batch.apod of generating calls), as DeviceLens.apod
        self.apod = None if table.apod is None else _calls.bytes_tensor(table.apod)
        self.newton = table.newton_surfaces
        self.last_schedule = None
        self.last_schedule_dev = None
        self.last_schedule_private = False
        self._resident: dict = {}

    def lens_tensors(self):
        """[surfaces, cs_ops, coef, zern, n_tab, alpha_tab, optics, materials, wavelengths]
        as CPU tensors (structured tables as their bytes)."""
        return self._tensors

    def resident(self, slot, arr):
        """A CPU tensor copy of a small host table, reused while its bytes are unchanged
        (DeviceLens.resident's counterpart)."""
        a = np.ascontiguousarray(arr)
        raw = a.tobytes()
        hit = self._resident.get(slot)
        if hit is not None and hit[0] == raw and hit[1] == a.dtype:
            return hit[2]
        # (a structured table: its records' bytes)
        t = _calls.bytes_tensor(a) if a.dtype.fields is not None else torch.from_numpy(a.copy())
        self._resident[slot] = (raw, a.dtype, t)
        return t


def _scatter_of(hl, ray_offset):
    """(ort_scatter, its records) of a lens with BSDF surfaces, else None."""
    if not hl.table.has_bsdf:
        return None
    from . import scatter

    return scatter.scatter_struct(hl, ray_offset)


def _forward(hl, kind, src, outs, batch, start_surface, rec, updates, pol, scat):
    """One forward entry of the host library (_calls.FORWARD) and its status check. scat:
    _scatter_of's pair, kept alive through the call."""
    entry, extra = _calls.forward_entry("host", kind, pol, scat and scat[0])
    status = np.zeros(1, dtype=np.int32)
    opt = _native.ort_options(_abi.NEWTON_SCHEDULE, int(start_surface), None)
    _calls.call_forward(_native.load_host(), entry, hl.c, src, rays_struct(outs), batch, opt,
                        rec, updates, status, extra)
    _calls.raise_status(int(status[0]), hl.table, scat and scat[0].max_attempts)


def trace_sequential(hl: HostLens, rays_in, w, per_ray_w, start_surface, rec, ray_offset=0,
                     pol=None, outs=None):
    """ort_host_trace_sequential of resident CPU rays (8 contiguous float64 tensors):
    returns the 8 output tensors (outs: preallocated ones) and the Newton update counts [S]
    (int32 tensor) the reference's stop rule made. A lens with BSDF surfaces takes
    ort_host_trace_sequential_scatter (ray r draws as r + ray_offset); pol, the
    ort_polarization of a lens lowered with polarized=True (its caller keeps the coatings
    and planes alive), ort_host_trace_sequential_polarized."""
    n = rays_in[0].numel()
    if outs is None:
        outs = [torch.empty(n, dtype=torch.float64) for _ in range(8)]
    batch = _calls.resident_batch(n)
    w_keep = None
    if per_ray_w:
        w_keep = _calls.per_ray_wavelengths(hl.table, w, n, hl.device, validate=True)
        batch.w = addr(w_keep)
    updates = torch.zeros(hl.table.n_surfaces, dtype=torch.int32)
    scat = _scatter_of(hl, ray_offset)
    if scat is not None and per_ray_w:
        raise ValueError("BSDF surfaces trace one wavelength per call")
    _forward(hl, "sequential", rays_struct(rays_in), outs, batch, start_surface, rec, updates,
             pol, scat)
    del w_keep  # (read by the call above)
    return outs, updates


def trace_sequential_vjp(hl: HostLens, rays_in, w, per_ray_w, start_surface, sched, tabs,
                         need, n_param, mode, cot, rec_cot, rec, grad, gin):
    """ort_host_trace_sequential_vjp: grad += J^T cot, gin = input-ray cotangents.
    tabs: (zern_param, surf_tangent, final_tangent) CPU tensors or None."""
    lib = _native.load_host()
    n = rays_in[0].numel()
    batch = _calls.resident_batch(n)
    w_keep = None
    if per_ray_w:
        w_keep = _calls.per_ray_wavelengths(hl.table, w, n, hl.device, validate=False)
        batch.w = addr(w_keep)
    sched_c = sched if sched is not None and sched.numel() else None
    opt = _native.ort_options(_abi.NEWTON_SCHEDULE, int(start_surface), addr(sched_c))
    params = _calls.vjp_params(hl.table, n_param, mode, tabs, need, grad_init=False)
    rc = lib.ort_host_trace_sequential_vjp(
        C.byref(hl.c), C.byref(rays_struct(rays_in)), C.byref(batch), C.byref(opt),
        C.byref(params), C.byref(rays_struct(cot)), addr(rec_cot),
        addr(rec if rec_cot is not None else None), addr(grad),
        C.byref(rays_struct(gin if gin is not None else [None] * 8)))
    _native.check(rc, "ort_host_trace_sequential_vjp")
    del w_keep


def trace_pupil(hl: HostLens, seg, px, py, n, seg_len, pupil_per_ray, apod=None, ray_offset=0,
                rec=None, pol=None, outs=None):
    """ort_host_trace_pupil: rays generated from the pupil samples by the segments (SEGMENT
    records as a uint8 CPU tensor, or a host array) and traced as one reference trace call
    (one Newton group); returns the 8 output tensors (outs: preallocated ones) and the update
    counts [S] (int32). BSDF surfaces / pol: the _scatter / _polarized entry, as
    trace_sequential; rec ([n_rec][8][n] or None) is theirs -- the plain entry has none."""
    if outs is None:
        outs = [torch.empty(n, dtype=torch.float64) for _ in range(8)]
    # one Newton group: the whole call, as RealRayTracer.trace traces every field of a
    # wavelength in one SurfaceGroup.trace (real_ray_tracer.py:37-97)
    seg = _calls.segments_of(hl, seg)  # (kept alive through the call, as apod by the caller)
    batch = _calls.pupil_batch(n, seg_len, n, seg, pupil_per_ray, apod)
    S = hl.table.n_surfaces
    n_groups = 1 if n else 0
    updates = torch.zeros(max(1, n_groups) * S, dtype=torch.int32)
    _forward(hl, "pupil", (px, py), outs, batch, 0, rec, updates, pol,
             _scatter_of(hl, ray_offset))
    return outs, updates[:n_groups * S]


def trace_pupil_vjp(hl: HostLens, seg, px, py, n, seg_len, pupil_per_ray, sched, tabs, need,
                    n_param, mode, cot, grad, apod=None, rms=None):
    """ort_host_trace_pupil_vjp: grad = J^T cot of the pupil trace (grad overwritten).
    rms: (stats[5], g[1]) of an rms spot size of the outputs, folded into the x, y
    cotangents (ort_vjp_params.rms_stats / rms_grad; the adjoint mode)."""
    lib = _native.load_host()
    batch = _calls.pupil_batch(n, seg_len, n, seg, pupil_per_ray, apod)
    sched_c = sched if sched is not None and sched.numel() else None
    opt = _native.ort_options(_abi.NEWTON_SCHEDULE, 0, addr(sched_c))
    params = _calls.vjp_params(hl.table, n_param, mode, tabs, need, grad_init=True, rms=rms)
    rc = lib.ort_host_trace_pupil_vjp(C.byref(hl.c), addr(px), addr(py), C.byref(batch),
                                      C.byref(opt), C.byref(params), C.byref(rays_struct(cot)),
                                      addr(grad))
    _native.check(rc, "ort_host_trace_pupil_vjp")


def rms_spot(x, y):
    """ort_host_rms_spot: (rms scalar, stats[5]) of contiguous float64 CPU tensors."""
    lib = _native.load_host()
    stats = torch.empty(5, dtype=torch.float64)
    rms = torch.empty((), dtype=torch.float64)
    rc = lib.ort_host_rms_spot(addr(x), addr(y), x.numel(), addr(stats), addr(rms))
    _native.check(rc, "ort_host_rms_spot")
    return rms, stats


def rms_spot_vjp(x, y, stats, g):
    lib = _native.load_host()
    gx, gy = torch.empty_like(x), torch.empty_like(y)
    rc = lib.ort_host_rms_spot_vjp(addr(x), addr(y), x.numel(), addr(stats), addr(g), addr(gx), addr(gy))
    _native.check(rc, "ort_host_rms_spot_vjp")
    return gx, gy


def huygens_psf(image, pupil, wavelength_mm, rp):
    """ort_host_huygens_psf: raw |field|^2 [n_image] of contiguous float64 CPU tensors
    (image = x, y, z; pupil = x, y, z, amp, opd in mm)."""
    lib = _native.load_host()
    psf = torch.empty(image[0].numel(), dtype=torch.float64)
    rc = lib.ort_host_huygens_psf(*(addr(t) for t in image), image[0].numel(),
                                  *(addr(t) for t in pupil), pupil[0].numel(),
                                  float(wavelength_mm), float(rp), addr(psf))
    _native.check(rc, "ort_host_huygens_psf")
    return psf


def dft_psf(amp, opd_waves, batch, n, m, pad):
    """ort_host_dft_psf: the raw |field|^2 [batch * m * m] of contiguous float64 CPU tensors
    amp, opd_waves [batch * n * n]."""
    lib = _native.load_host()
    out = torch.empty(batch * m * m, dtype=torch.float64)
    rc = lib.ort_host_dft_psf(addr(amp), addr(opd_waves), batch, n, m, float(pad), addr(out))
    _native.check(rc, "ort_host_dft_psf")
    return out


def sampled_otf(tensors, batch, n_terms, terms, radial):
    """ort_host_sampled_otf: the complex OTF [batch * F * 2] of contiguous float64 CPU tensors
    (x, y [N], intensity, opd_waves [batch * N], coeffs [batch * n_terms], shift_x, shift_y
    [F]); terms: the _abi.ZERNIKE_TERM records and radial their weights (NumPy arrays,
    ops._otf_terms)."""
    lib = _native.load_host()
    x, y, intensity, opd_waves, coeffs, shift_x, shift_y = tensors
    n, f = x.numel(), shift_x.numel()
    out = torch.empty(batch * f * 2, dtype=torch.float64)
    rc = lib.ort_host_sampled_otf(addr(x), addr(y), n, addr(intensity), addr(opd_waves), batch,
                                  addr(terms), addr(radial), addr(coeffs), n_terms,
                                  addr(shift_x), addr(shift_y), f, addr(out))
    _native.check(rc, "ort_host_sampled_otf")
    return out


def irradiance_bin(x, y, power, x_edges, y_edges, mode, pixel_area=0.0):
    """ort_host_irradiance_bin: the flat map [nx * ny] of contiguous float64 CPU tensors
    (histogram: index ix * ny + iy; bilinear: iy * nx + ix)."""
    lib = _native.load_host()
    nx, ny = x_edges.numel() - 1, y_edges.numel() - 1
    out = torch.empty(max(nx * ny, 0), dtype=torch.float64)
    rc = lib.ort_host_irradiance_bin(addr(x), addr(y), addr(power), x.numel(), addr(x_edges), nx,
                                     addr(y_edges), ny, int(mode), float(pixel_area), addr(out))
    _native.check(rc, "ort_host_irradiance_bin")
    return out


def irradiance_bin_vjp(x, y, power, x_edges, y_edges, grad, pixel_area=0.0):
    """ort_host_irradiance_bin_vjp: (g_x, g_y, g_power) of the bilinear map."""
    lib = _native.load_host()
    nx, ny = x_edges.numel() - 1, y_edges.numel() - 1
    gx, gy, gp = (torch.empty(x.numel(), dtype=torch.float64) for _ in range(3))
    rc = lib.ort_host_irradiance_bin_vjp(addr(x), addr(y), addr(power), x.numel(), addr(x_edges), nx,
                                         addr(y_edges), ny, float(pixel_area), addr(grad), addr(gx),
                                         addr(gy), addr(gp))
    _native.check(rc, "ort_host_irradiance_bin_vjp")
    return gx, gy, gp
