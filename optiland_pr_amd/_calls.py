"""The Python call layer of the two C ABIs: the argument structs of include/optiland_rt.h
(and of include/optiland_host.h, which takes the same ones) built from tensors, and the one
place that knows how a forward-trace entry point is called -- the Python counterpart of
csrc/ort_args.h, which reads these structs for both libraries.

FORWARD names the 12 forward entries (device / host, pupil / sequential, plain / polarized /
scatter) with their two signature differences, call_forward builds their argument list and
makes the call, and raise_status turns the status word any of them leaves into its
exception. Only raytrace.py (device) and host.py (host) call a forward entry; polarization.py,
scatter.py, ops.py and tolerancing.py build their extra struct and hand it to those two.
Flat functions over _native's ctypes structs: no torch ops and no GPU-runtime calls here,
only the library call a caller hands in.
"""

from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _abi, _native

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None


def addr(t):
    """The address of a tensor's or a numpy array's first element for a c_void_p field or
    argument; None (NULL) for None."""
    if t is None:
        return None
    return t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data


def bytes_tensor(arr):
    """A numpy array's bytes (a structured table: its records) as a uint8 CPU tensor of its
    own memory."""
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(arr).tobytes(),
                                          dtype=np.uint8).copy())


def segments_of(lens, segs):
    """The SEGMENT records of a generating launch on the lens's device (DeviceLens or
    HostLens): a tensor goes as it is, a host array through lens.resident (no copy while
    its bytes are unchanged). The caller keeps the result alive until its launch is
    enqueued."""
    if torch.is_tensor(segs):
        return segs
    return lens.resident("segments", np.asarray(segs, dtype=_abi.SEGMENT))


def rays_struct(ts):
    """ort_rays of 8 tensors (x, y, z, L, M, N, i, opd); None: a NULL field."""
    return _native.ort_rays(*(addr(t) for t in ts))


def _batch(n, seg_len, group_len, seg, pupil_per_ray, apod):
    if n == 0:
        # an empty batch: no ray reads the lengths, and the C front end (ort_args.h
        # fill_args) wants both >= 1. With rays they go as given, so that it still refuses
        # a caller's zero instead of indexing the segments by it.
        seg_len, group_len = max(seg_len, 1), max(group_len, 1)
    n_seg = 0 if seg is None else seg.numel() // _abi.SEGMENT.itemsize
    return _native.ort_batch(n, seg_len, group_len, n_seg, int(pupil_per_ray), addr(seg), None,
                             addr(apod))


def pupil_batch(n, seg_len, group_len, seg, pupil_per_ray=False, apod=None):
    """ort_batch of rays generated from pupil samples: ray r belongs to segment r // seg_len
    of `seg` (SEGMENT records as a uint8 tensor), Newton groups of group_len rays; apod: the
    APODIZATION record (uint8 tensor) or None."""
    return _batch(n, seg_len, group_len, seg, pupil_per_ray, apod)


def resident_batch(n, group_len=None, seg=None, seg_len=None):
    """ort_batch of resident rays: one segment and one Newton group of all n unless given
    (seg / seg_len: per-segment wavelength rows, as pupil_batch). Per-ray wavelengths go
    into its `w` field (per_ray_wavelengths)."""
    return _batch(n, seg_len or max(n, 1), group_len or max(n, 1), seg, False, None)


class ForwardEntry(NamedTuple):
    """One forward-trace entry point: its symbol and what its signature differs in."""
    name: str
    kind: str       # "pupil": (px, py) generate the rays; "sequential": resident rays_in
    host: bool      # update counts where the device takes Newton statistics; no stream
    has_rec: bool   # False for ort_host_trace_pupil alone: a `rec` given there is dropped


# (library, kind, extra) -> ForwardEntry; extra: None, "polarized" (an ort_polarization
# follows the status) or "scatter" (an ort_scatter does)
FORWARD = {
    (library, kind, extra): ForwardEntry(name, kind, library == "host",
                                         name != "ort_host_trace_pupil")
    for library, kind, extra, name in (
        ("device", "pupil", None, "ort_trace_pupil"),
        ("device", "pupil", "polarized", "ort_trace_pupil_polarized"),
        ("device", "pupil", "scatter", "ort_trace_pupil_scatter"),
        ("device", "sequential", None, "ort_trace_sequential"),
        ("device", "sequential", "polarized", "ort_trace_sequential_polarized"),
        ("device", "sequential", "scatter", "ort_trace_sequential_scatter"),
        ("host", "pupil", None, "ort_host_trace_pupil"),
        ("host", "pupil", "polarized", "ort_host_trace_pupil_polarized"),
        ("host", "pupil", "scatter", "ort_host_trace_pupil_scatter"),
        ("host", "sequential", None, "ort_host_trace_sequential"),
        ("host", "sequential", "polarized", "ort_host_trace_sequential_polarized"),
        ("host", "sequential", "scatter", "ort_host_trace_sequential_scatter"),
    )}
GENERATE = {"device": "ort_generate_rays", "host": "ort_host_generate_rays"}


def forward_entry(library, kind, pol=None, scat=None):
    """(the FORWARD entry, its extra struct) of a trace with an optional ort_polarization
    or ort_scatter (one dict hit; no entry takes both)."""
    if pol is not None:
        if scat is not None:
            raise ValueError("BSDF surfaces together with coatings or a polarization state "
                             "are not supported")
        return FORWARD[library, kind, "polarized"], pol
    if scat is not None:
        return FORWARD[library, kind, "scatter"], scat
    return FORWARD[library, kind, None], None


def call_forward(lib, entry, lens_c, src, out_c, batch, opt, rec, counts, status, extra=None,
                 stream=None):
    """Call a FORWARD entry of `lib` and check its return code. src: (px, py) for a pupil
    entry, the ort_rays of the resident rays for a sequential one; counts: the Newton
    statistics (device) or update counts (host); extra: the entry's ort_polarization /
    ort_scatter; stream: the device entries' last argument."""
    name, kind, host, has_rec = entry
    args = [C.byref(lens_c)]
    args += (addr(src[0]), addr(src[1])) if kind == "pupil" else (C.byref(src),)
    args += (C.byref(out_c), C.byref(batch), C.byref(opt))
    if has_rec:
        args.append(addr(rec))
    args += (addr(counts), addr(status))
    if extra is not None:
        args.append(C.byref(extra))
    if not host:
        args.append(stream)
    _native.check(getattr(lib, name)(*args), name)


def call_generate(lib, library, px, py, out_c, batch, stream=None):
    """ort_generate_rays / ort_host_generate_rays (GENERATE[library]) of `lib`."""
    name = GENERATE[library]
    args = [addr(px), addr(py), C.byref(out_c), C.byref(batch)]
    if library == "device":
        args.append(stream)
    _native.check(getattr(lib, name)(*args), name)


class ZernikeRangeError(ValueError):
    pass


class ChebyshevRangeError(ValueError):
    pass


_CHEBYSHEV_MSG = ("Chebyshev input coordinates must be normalized to [-1, 1]. Consider "
                  "updating the normalization factors.")  # chebyshev.py:203-215
_ZERNIKE_MSG = ("Zernike coordinates must be normalized to [-1, 1]. Consider updating the "
                "normalization radius to 1.1x the surface aperture.")


def raise_status(v, table=None, max_attempts=None):
    """The exception of a status word (ORT_STATUS_* bits) a trace left, for both libraries
    and the deferred device checks; nothing for 0. table / max_attempts: the traced
    LensTable and its scatter_max_attempts -- with BSDF surfaces a used-up rejection loop
    is reported by surface and sigma."""
    if not v:
        return
    if v & _abi.STATUS_BAD_APODIZATION:
        raise ValueError("the apodization record holds a kind the trace core does not know")
    if v & _abi.STATUS_BAD_GEOMETRY:
        raise ValueError("the lens table holds a geometry id the trace core does not know "
                         "(library / host ABI mismatch?)")
    if v & _abi.STATUS_ZERNIKE_RANGE:
        raise ZernikeRangeError(_ZERNIKE_MSG)
    if v & _abi.STATUS_CHEBYSHEV_RANGE:
        raise ChebyshevRangeError(_CHEBYSHEV_MSG)
    if v & _abi.STATUS_SCATTER_ATTEMPTS:
        from . import scatter

        if table is not None and table.has_bsdf:
            raise scatter.attempts_error(scatter.describe(table),
                                         max_attempts or scatter.DEFAULT_MAX_ATTEMPTS)
        raise scatter.ScatterAttemptsError("BSDF scattering used up its attempts")


def decreasing_tables(table):
    """{material index: name} of the lens materials with tabulated n or k data whose
    wavelengths decrease somewhere (45 of the refractiveindex.info database's 2,631 tables
    are not strictly increasing; repeated wavelengths are fine, a decreasing step is not).
    Found once per LensTable."""
    hit = getattr(table, "_decreasing_tables", None)
    if hit is not None:
        return hit
    hit = {}
    mt = table.mat_table
    for mi in range(0 if mt is None else len(mt)):
        m = mt[mi]
        spans = [(int(m["k_off"]), int(m["k_len"]))]
        if int(m["kind"]) == _abi.MAT_TABULATED:
            spans.append((int(m["coef_off"]), int(m["n_coef"])))
        if any(np.any(np.diff(table.coef[o:o + ln]) < 0) for o, ln in spans if ln > 1):
            mats = getattr(table, "materials", None) or []
            m = mats[mi] if mi < len(mats) else None
            if m is None:
                hit[mi] = f"material {mi}"
            else:  # a wrapped reference material has no repr of its own: its file instead
                own = type(m).__repr__ is not object.__repr__
                hit[mi] = repr(m) if own else str(m.key())
    table._decreasing_tables = hit
    return hit


def refuse_decreasing_tables(table, mats=None):
    """Per-ray wavelengths (ort_batch.w, ort_material_nk) through a table whose wavelengths
    decrease are refused: numpy.interp, which the reference calls, searches such a table
    from the index its previous query found, so its value depends on the order of the
    queries -- nothing a per-ray kernel can reproduce (csrc/ort_material.h np_interp). The
    per-wavelength n / alpha tables are host NumPy and stay available. mats: only these
    material indices (None: every material of the lens)."""
    bad = decreasing_tables(table)
    names = [v for k, v in bad.items() if mats is None or k in mats]
    if names:
        raise ValueError(f"{', '.join(names)}: the tabulated wavelengths decrease, so "
                         "numpy.interp depends on the query order; per-ray wavelengths are "
                         "refused for this material (per-wavelength tables still work).")


def per_ray_wavelengths(table, w, n, device, validate):
    """ort_batch.w: `w` as n contiguous float64 wavelengths on `device` (one value: expanded;
    already so: the same memory, no copy). The caller keeps the result alive until its
    launches are ordered on the stream.

    validate: refuse wavelengths outside the Abbe model's 0.380-0.750 um when the lens has
    such a material, as the reference does before it uses any index (abbe.py:47-48; the
    device would only give NaN). That reads `w` -- a device synchronisation -- so the
    forward traces validate and the VJPs do not: a backward's `w` is the one its forward
    checked. This is the one intended difference between the call sites.

    Every call site refuses a lens with a decreasing wavelength table
    (refuse_decreasing_tables; host data only, no synchronisation)."""
    refuse_decreasing_tables(table)
    w = w.detach().to(device=device, dtype=torch.float64).reshape(-1)
    w = w.expand(n).contiguous() if w.numel() == 1 else w.contiguous()
    if w.numel() != n:
        raise ValueError("rays.w must hold one wavelength per ray")
    mt = table.mat_table
    if validate and mt is not None and np.any(mt["kind"] == _abi.MAT_ABBE):
        if bool(((w < 0.380) | (w > 0.750)).any()):
            raise ValueError("Wavelength out of range for this model.")
    return w


def vjp_params(table, n_param, mode, tabs, need, grad_init, tape=None, primal=None, rms=None):
    """ort_vjp_params without its workspace (attach_vjp_workspace). tabs: (zern_param,
    surf_tangent, final_tangent) tensors or None; need: slot_need or None; grad_init: the
    gradient is overwritten; tape / primal: the adjoint tape the forward wrote and its 8
    outputs (the device's adjoint mode); rms: (stats[5], g[1]) of an rms spot size folded
    into the x, y cotangents. n_mono is the adjoint mode's: no unrolled path of either
    library reads it (ort_args.h vjp_fill_unrolled, ort_api.hip adj_layout)."""
    from .ops import mono_slot_count

    zp, st, ft = tabs
    p = _native.ort_vjp_params(int(n_param), int(mode), addr(zp), addr(st), addr(ft),
                               0 if zp is None else int(zp.numel()), int(bool(grad_init)),
                               None, 0, addr(need))
    if mode == _abi.VJP_ADJOINT:
        p.n_mono = mono_slot_count(table, zp)
    if tape is not None:
        p.tape, p.primal = addr(tape), rays_struct(primal)
    if rms is not None:
        p.rms_stats, p.rms_grad = addr(rms[0]), addr(rms[1])
    return p


_WORKSPACES: dict = {}


def workspace(pool, device, nbytes):
    """Scratch bytes on `device`, grown on demand and reused by every later call of the same
    pool (at least 8 bytes, so never a NULL address). One pool per op that owns a buffer:
    "pupil_vjp", "seq_vjp", "rms"."""
    ws = _WORKSPACES.get((pool, device))
    if ws is None or ws.numel() < nbytes:
        _WORKSPACES.pop((pool, device), None)
        ws = torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=device)
        _WORKSPACES[(pool, device)] = ws
    return ws


def attach_vjp_workspace(lib, lens_c, batch, params, pool, device):
    """Give `params` the device workspace its VJP call needs (ort_vjp_workspace_size; both
    modes take one), from `pool`."""
    size = lib.ort_vjp_workspace_size(C.byref(lens_c), C.byref(batch), C.byref(params))
    _native.check(int(size) if size < 0 else 0, "ort_vjp_workspace_size")
    ws = workspace(pool, device, size)
    params.workspace, params.workspace_size = ws.data_ptr(), ws.numel()
