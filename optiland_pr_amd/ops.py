"""PyTorch custom ops over the C ABI: ``torch.ops.ort.trace_sequential`` and
``torch.ops.ort.trace_pupil`` (SURVEY.md 8b "Torch custom op").

The reference differentiates a trace by running every ``be.*`` primitive of
``SurfaceGroup.trace`` (surfaces/surface_group.py:232-244) under torch autograd
(backend/torch_backend.py:45-148, driven by optimization/optimizer/torch/base.py:116-131).
Here the whole trace is ONE dispatcher op whose CUDA (HIP) kernel is the fused trace
(ort_trace_sequential / ort_trace_pupil) and whose autograd formula is the adjoint (or
forward-mode) VJP of the trace core (ort_trace_sequential_vjp / ort_trace_pupil_vjp), so
autograd sees one node per trace call:

  ort::trace_sequential(lens, lens_meta, final_thickness, lens_key, rays[8], w, params,
                        spec, start_surface, per_ray_w)
      -> (x, y, z, L, M, N, i, opd, rec, sched)
      resident rays in (SurfaceGroup.trace, the drop-in seam); rec = every traced
      surface's record [S][8][n] (standard_surface.py:266-286); differentiable w.r.t. the
      input rays, the record buffer's cotangents included, and the lens parameters in
      `params`.
  ort::trace_pupil(lens, lens_meta, final_thickness, lens_key, seg, apod, px, py, params,
                   spec, plan_meta, plan_key)
      -> (x, y, z, L, M, N, i, opd, sched, tape, rms, rms_stats)
      rays generated from pupil samples in the same launch (Optic.trace's fused path,
      raytrace/real_ray_tracer.py:37-97); differentiable w.r.t. the lens parameters.

The ops are self-describing: ``lens`` is the lowered lens as tensors (lens_args: the nine
uploaded tables, a few KB the kernels read from HBM) with its scalars in ``lens_meta``;
``seg`` / ``apod`` / ``plan_meta`` describe the pupil plan the same way. ``lens_key`` /
``plan_key`` are integer cache keys only -- the handle of the live host object holding the
Newton schedule caches; a key that names no live object of these tensors makes the op
rebuild the lens from the tensors. ``params`` are the lens-parameter tensors that require
grad and ``spec`` says which lens value each one is, as flattened (kind, traced-surface
index) pairs with kind in SPEC_KINDS: the forward ignores their values (the lowered lens
already holds them), the backward returns d loss / d each.

ort::trace_sequential has two kernels, one per dispatch key: CUDA (HIP) runs
the fused GPU trace on a DeviceLens handle, CPU runs the host build of the same per-ray
source (host.py, liboptiland_host.so, include/optiland_host.h) on a HostLens handle, with
its VJP on the host too. Neither falls back to the other: the dispatcher picks the kernel
by the tensors' device, and a handle of the other kind raises. trace_pupil and rms_spot
are CUDA-only.

ort::huygens_psf(image_x, image_y, image_z, pupil_x, pupil_y, pupil_z, amp, opd_mm,
wavelength_mm, rp) -> psf is HuygensPSF's summation (psf/huygens_fresnel_strategies.py:97-172,
ort_huygens_psf) on both keys; it has no autograd formula yet and refuses inputs that require
grad.

ort::sampled_otf(x, y, intensity, opd_waves, coeffs, kind, shift_x, shift_y) -> otf is
SampledMTF's overlap sum over pupil shears (mtf/sampled.py:162-205, ort_sampled_otf) on both
keys, forward only like the two PSF ops.

ort::dft_psf(amp, opd_waves, image_size, pad_size) -> psf is the pupil-to-image transform of
FFTPSF, MMDFTPSF and FFTMTF (psf/fft.py:169-234, psf/mmdft.py:164-184, ort_dft_psf) on both
keys, of one (n, n) pupil or a batch (B, n, n); it refuses inputs that require grad.

ort::irradiance_bin(x, y, power, x_edges, y_edges, mode, pixel_area=None) -> map is
IncoherentIrradiance's binning (analysis/irradiance.py:243-330, ort_irradiance_bin) on both
keys: mode _abi.BIN_HISTOGRAM ([nx, ny], numpy.histogram2d's pixels) or _abi.BIN_BILINEAR
([ny, nx], get_bilinear_weights' splat), fixed-point sums that do not depend on the order of
the rays. The bilinear mode is differentiable in x, y and power through
ort::irradiance_bin_vjp (a gather); the histogram mode refuses inputs that require grad.
"""

from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np
import torch

from . import _abi, _calls, _native
from ._calls import addr

SPEC_KINDS = ("zernike", "radius", "conic", "thickness", "vertex")

# handle -> host object (DeviceLens / pupil plan); weak, so a handle never keeps a lens
# alive (the autograd context holds the object itself for the backward)
_HANDLES: "weakref.WeakValueDictionary[int, object]" = weakref.WeakValueDictionary()


def handle(obj) -> int:
    """Integer handle of a host object for the ops' `lens` / `plan` argument."""
    h = id(obj)
    _HANDLES[h] = obj
    return h


def _lookup(h):
    obj = _HANDLES.get(int(h))
    if obj is None:
        raise RuntimeError(f"ort op: stale handle {h} (the lens / plan object was freed)")
    return obj


class PupilPlan:
    """Everything ort::trace_pupil needs besides the parameter tensors."""

    def __init__(self, dlens, seg_dev, px, py, n, seg_len, keys=(), pupil_per_ray=False,
                 newton_mode="reference"):
        self.dlens = dlens
        self.seg_dev = seg_dev
        self.px = px
        self.py = py
        self.n = int(n)
        self.seg_len = int(seg_len)
        self.keys = list(keys)
        self.pupil_per_ray = bool(pupil_per_ray)
        self.newton_mode = newton_mode
        self.want_tape = False  # set by the caller when the backward is an adjoint sweep
        self.want_rms = False  # the rms spot size in the taped forward's epilogue (F_RMS)
        self.tape = None


def _spec_pairs(spec):
    if len(spec) % 2:
        raise ValueError("spec holds (kind, surface) pairs")
    return [(SPEC_KINDS[int(spec[i])], int(spec[i + 1])) for i in range(0, len(spec), 2)]


def encode_spec(pairs):
    """[(kind name, traced-surface index)] -> the flat int list the ops take."""
    out = []
    for kind, si in pairs:
        out += [SPEC_KINDS.index(kind), int(si)]
    return out


def tangent_tables(table, pairs, params):
    """ort_vjp_params tables for the parameter tensors: (zern_param, surf_tangent,
    final_tangent, n_param) -- numpy arrays or None. "vertex" is the vertex z of one
    surface (its coordinate system's z, coordinate_system.py:73-107); "thickness" moves
    every later vertex (optic_updater.py set_thickness)."""
    S = table.n_surfaces
    n_param = sum(int(t.numel()) for t in params)
    zp = surf = final = None
    off = 0
    for (kind, si), t in zip(pairs, params, strict=True):
        n = int(t.numel())
        row = table.surfaces[si]
        if kind == "zernike":
            if int(row["geometry"]) != _abi.GEOM_ZERNIKE:
                raise ValueError(f"surface {si}: Zernike coefficients of a non-Zernike surface")
            if zp is None:
                zp = np.full(max(1, len(table.zern)), -1, dtype=np.int32)
            if n != int(row["n_coef"]):
                raise ValueError(f"surface {si}: {n} coefficients, lowered {int(row['n_coef'])}")
            base = int(row["coef_off"])
            zp[base:base + n] = np.arange(off, off + n, dtype=np.int32)
        else:
            if n != 1:
                raise ValueError(f"surface {si}: {kind} must be a scalar tensor")
            if surf is None:
                surf = np.zeros((n_param, S, 3), dtype=np.float64)
            g = int(row["geometry"])
            if kind in ("radius", "conic"):
                if g in (_abi.GEOM_PLANE, _abi.GEOM_BICONIC, _abi.GEOM_TOROIDAL, _abi.GEOM_GRID_SAG,
                         _abi.GEOM_NURBS):
                    raise NotImplementedError(f"surface {si}: {kind} of this geometry is not a "
                                              "differentiable parameter of the trace core")
                if int(row["interaction"]) == _abi.IA_DIFFRACTIVE:
                    # the grating vector's groove-tangent constants are formed from them on
                    # the host (standard_grating.py:93-146): no tangent reaches them
                    raise NotImplementedError(f"surface {si}: {kind} of a grating surface is not "
                                              "a differentiable parameter of the trace core")
                surf[off, si, 0 if kind == "radius" else 1] = 1.0
            elif kind == "vertex":
                surf[off, si, 2] = 1.0
            else:  # thickness after surface si moves every later vertex
                surf[off, si + 1:, 2] = 1.0
                if si == S - 1:  # the image surface's thickness: the final propagate
                    if final is None:
                        final = np.zeros(n_param, dtype=np.float64)
                    final[off] = 1.0
        off += n
    return zp, surf, final, n_param


# ORT_ADJ_MONO=0 (A/B checks): Zernike coefficient adjoints in per-term slots instead of
# the Cartesian monomial basis (ort_vjp_params.n_mono, ABI v18)
ADJ_MONO = os.environ.get("ORT_ADJ_MONO", "1") != "0"


def mono_slot_count(table, zp):
    """ort_vjp_params.n_mono: the monomial-basis slots of the lens's Zernike surfaces with a
    Cartesian block (2 K = (zm_deg + 1)(zm_deg + 2) each, in surface order), 0 without
    Zernike parameters (or with ORT_ADJ_MONO=0)."""
    if zp is None or not ADJ_MONO:
        return 0
    s = table.surfaces
    # (blocks above ort_sweep.h kMonoMaxDeg = 6 take the per-term slots)
    d = s["zm_deg"][(s["geometry"] == _abi.GEOM_ZERNIKE) & (s["zm_deg"] >= 0)
                    & (s["zm_deg"] <= 6)].astype(np.int64)
    return int(np.sum((d + 1) * (d + 2)))


def slot_need(table, zp, surf, final):
    """ort_vjp_params.slot_need of the tangent tables: nonzero for every slot (radius,
    conic, vertex z of each surface; each Zernike term; the final thickness; the monomial
    slots of the Cartesian Zernike surfaces) some parameter depends on. Host NumPy, kept
    resident with the tables."""
    S = table.n_surfaces
    n_z = 0 if zp is None else len(zp)
    n_mono = mono_slot_count(table, zp)
    need = np.zeros(3 * S + n_z + 1 + n_mono, dtype=np.int32)
    if surf is not None:
        need[:3 * S] = np.any(surf != 0.0, axis=0).reshape(-1)
    if zp is not None:
        need[3 * S:3 * S + n_z] = zp >= 0
    if final is not None:
        need[3 * S + n_z] = np.any(final != 0.0)
    if n_mono:
        off = 3 * S + n_z + 1
        for row in table.surfaces:
            if int(row["geometry"]) != _abi.GEOM_ZERNIKE or int(row["zm_deg"]) < 0:
                continue
            d = int(row["zm_deg"])
            c0, nt = int(row["coef_off"]), int(row["n_coef"])
            if np.any(zp[c0:c0 + nt] >= 0):
                need[off:off + (d + 1) * (d + 2)] = 1
                # the per-term slots of this surface are not summed (the monomials are)
                need[3 * S + c0:3 * S + c0 + nt] = 0
            off += (d + 1) * (d + 2)
    return need


def tape_rows(table):
    """Rows of the adjoint tape per ray (ort_options.tape, ABI v19): 7 per plane / conic
    surface, 11 per Newton surface -- every one written by the taped trace."""
    g = table.surfaces["geometry"]
    closed = (g == _abi.GEOM_PLANE) | (g == _abi.GEOM_STANDARD)
    return int(7 * len(g) + 4 * np.count_nonzero(~closed))


def tape_doubles(dl, n):
    """Doubles of the adjoint tape of an n-ray trace of this lens: exactly the rows the
    taped trace writes (ort_vjp_tape_size bytes bound it for any lens of this many
    surfaces)."""
    return tape_rows(dl.table) * int(n)


def _check_differentiable(table, adjoint=False):
    """Refuse what no derivative kernel covers. adjoint: the reverse-mode pass is needed
    (input-ray cotangents), which has no reverse for thin-lens / phase / grating surfaces
    (their parameter gradients come from the forward-mode VJP, autodiff.vjp_mode)."""
    if np.any(table.surfaces["geometry"] == _abi.GEOM_GRID_SAG):
        raise NotImplementedError("autograd through grid-sag surfaces is not implemented by "
                                  "the trace core (no derivative kernels)")
    if np.any(table.surfaces["geometry"] == _abi.GEOM_NURBS):
        raise NotImplementedError("autograd through NURBS surfaces is not implemented by "
                                  "the trace core (no derivative kernels)")
    if adjoint and table.interaction_mask & ~(1 << _abi.IA_REFRACT_REFLECT):
        raise NotImplementedError("input-ray gradients through thin-lens, phase or grating "
                                  "surfaces are not implemented by the trace core (the "
                                  "forward-mode VJP carries parameter tangents only)")


# --------------------------------------------------------------------------------------
# the lens as the ops take it (the op is self-describing)
# --------------------------------------------------------------------------------------
# lens_meta: the host-side scalars of the ort_lens struct, in this order
LENS_META = ("n_surfaces", "n_lambda", "n_mat", "final_mat", "geometry_mask",
             "interaction_mask", "frame_flags", "n_rec", "newton", "tape_rows")
NEWTON_MODES = ("reference", "device", "wave")


def lens_args(dl, scatter=False):
    """(lens, lens_meta, final_thickness, lens_key) of a DeviceLens / HostLens: the nine
    lowered tables as tensors on the lens's device -- surfaces, cs_ops, zern, optics and
    materials as their bytes (uint8), coef, n_tab, alpha_tab and the wavelengths as float64
    -- the ort_lens scalars, the image-space thickness and the handle of the object that
    holds the host-side state (Newton schedule caches), used only as a cache key."""
    t = dl.table
    if t.has_bsdf and not scatter:  # (scatter: the *_scatter ops, which take the BSDF records)
        raise ValueError("the lens has BSDF surfaces: the differentiable trace ops do not carry "
                         "them (Optic.trace, trace_generic and SurfaceGroup.trace do)")
    meta = [int(t.n_surfaces), len(t.wavelengths), int(t.n_tab.shape[1]), int(t.final_mat),
            int(dl.geometry_mask), int(t.interaction_mask), int(t.frame_flags), int(t.n_rec),
            1 if dl.newton else 0, tape_rows(t)]
    return dl.lens_tensors(), meta, float(t.final_thickness), handle(dl)


# lenses rebuilt from their tensors (a handle that names no live object of those tensors:
# e.g. a traced graph run in another process), keyed by the tables' addresses
_REBUILT: "weakref.WeakValueDictionary[tuple, object]" = weakref.WeakValueDictionary()


def _table_from_tensors(lens, meta, final_thickness):
    from .lowering import LensTable

    def raw(t, dt):
        return np.frombuffer(t.detach().cpu().numpy().tobytes(), dtype=dt).copy()

    S, n_lambda, n_mat = meta[0], meta[1], meta[2]
    surfaces = raw(lens[0], _abi.SURFACE)
    rec = [i for i in range(S) if int(surfaces[i]["flags"]) & _abi.SURF_RECORD]
    mats = raw(lens[7], _abi.MATERIAL)
    return LensTable(
        surfaces=surfaces, cs_ops=raw(lens[1], _abi.CS_OP),
        coef=lens[2].detach().cpu().numpy().astype(np.float64).copy(),
        zern=raw(lens[3], _abi.ZERNIKE_TERM),
        n_tab=lens[4].detach().cpu().numpy().reshape(n_lambda, n_mat).copy(),
        alpha_tab=lens[5].detach().cpu().numpy().reshape(n_lambda, n_mat).copy(),
        wavelengths=[float(v) for v in lens[8].detach().cpu().numpy()],
        final_mat=int(meta[3]), final_thickness=float(final_thickness), mat_table=mats,
        n_rec=int(meta[7]), rec_surfaces=rec)


def _has_data(t):
    """False for tensors without storage (fake / functional tensors while tracing)."""
    try:
        t.data_ptr()
        return True
    except RuntimeError:
        return False


def _resolve(lens, meta, final_thickness, key):
    """The DeviceLens / HostLens these tensors are: the object named by `key` when it holds
    exactly these tables, else one rebuilt from the tensors (cached by their addresses).
    While tracing (fake tensors: no data to compare or rebuild from), the object the key
    names -- the backward formulas only read its host-side tables."""
    obj = _HANDLES.get(int(key))
    if not _has_data(lens[0]):
        if obj is None or not hasattr(obj, "lens_tensors"):
            raise RuntimeError("ort op traced with a lens key that names no live lens")
        return obj
    if obj is not None and hasattr(obj, "lens_tensors"):
        mine = obj.lens_tensors()
        if all(a.data_ptr() == b.data_ptr() and a.device == b.device
               for a, b in zip(mine, lens, strict=True)):
            return obj
    ck = tuple((t.device.type, t.data_ptr()) for t in lens)
    hit = _REBUILT.get(ck)
    if hit is None:
        table = _table_from_tensors(lens, meta, final_thickness)
        if lens[0].device.type == "cpu":
            from .host import HostLens

            hit = HostLens(table)
        else:
            from .raytrace import DeviceLens

            hit = DeviceLens(table, device=lens[0].device)
        hit._source_tensors = list(lens)  # the rebuilt object keeps its source alive
        _REBUILT[ck] = hit
    return hit


def _schedule_tensor(dl):
    """The Newton schedule the last trace of `dl` settled on, as a fresh int32 tensor on the
    lens's device that the caller owns (empty: no Newton surfaces)."""
    if dl.last_schedule_dev is not None:  # device-verified: the settled device schedule
        return (dl.last_schedule_dev if dl.last_schedule_private  # a per-call copy
                else dl.last_schedule_dev.clone())
    if dl.last_schedule is None:
        return torch.empty(0, dtype=torch.int32, device=dl.device)
    # host-verified: a device clone of the resident copy its last launch read (no upload)
    return dl.resident("sched", dl.last_schedule.reshape(-1)).clone()


def _split_param_grads(g, shapes):
    """The flat parameter gradient cut back into the parameters' (shape, dtype, device)."""
    res = []
    off = 0
    for shape, dtype, pdev in shapes:
        k = int(np.prod(shape)) if len(shape) else 1
        res.append(g[off:off + k].reshape(shape).to(device=pdev, dtype=dtype))
        off += k
    return res


# --------------------------------------------------------------------------------------
# ort::trace_sequential
# --------------------------------------------------------------------------------------
@torch.library.custom_op("ort::trace_sequential", mutates_args=(), device_types="cuda")
def trace_sequential(lens: list[torch.Tensor], lens_meta: list[int], final_thickness: float,
                     lens_key: int, rays: list[torch.Tensor], w: torch.Tensor | None,
                     params: list[torch.Tensor], spec: list[int], start_surface: int,
                     per_ray_w: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                                               torch.Tensor, torch.Tensor, torch.Tensor,
                                               torch.Tensor, torch.Tensor, torch.Tensor,
                                               torch.Tensor]:
    from .raytrace import RealRays, trace_rays

    dl = _resolve(lens, lens_meta, final_thickness, lens_key)
    if len(rays) != 8:
        raise ValueError("rays: x, y, z, L, M, N, i, opd")
    n = rays[0].numel()
    dev = dl.device
    rin = RealRays.of(
        [t.detach().to(device=dev, dtype=torch.float64).reshape(-1).contiguous() for t in rays],
        w.detach() if w is not None else torch.zeros(1, dtype=torch.float64, device=dev))
    rout = RealRays.of([torch.empty(n, dtype=torch.float64, device=dev) for _ in range(8)])
    n_rec = dl.table.n_rec
    rec = torch.empty(n_rec * 8 * n, dtype=torch.float64, device=dev)
    trace_rays(dl, rin, rout, rec=rec if n_rec else None, start_surface=int(start_surface),
               per_ray_w=bool(per_ray_w))
    return (*(getattr(rout, a) for a in _abi.RAY_FIELDS), rec, _schedule_tensor(dl))


@trace_sequential.register_kernel("cpu")
def _trace_sequential_cpu(lens, lens_meta, final_thickness, lens_key, rays, w, params, spec,
                          start_surface, per_ray_w):
    """The CPU dispatch key: the host build of the trace core (host.py) on the lens's CPU
    tensors."""
    from . import host

    hl = _resolve(lens, lens_meta, final_thickness, lens_key)
    if not isinstance(hl, host.HostLens):
        raise RuntimeError("ort::trace_sequential: CPU rays need the lens's tables on the CPU "
                           f"(got a {type(hl).__name__})")
    if len(rays) != 8:
        raise ValueError("rays: x, y, z, L, M, N, i, opd")
    n = rays[0].numel()
    rin = [t.detach().to(dtype=torch.float64).reshape(-1).contiguous() for t in rays]
    if any(t.numel() != n for t in rin):
        raise ValueError("ray fields of different sizes")
    n_rec = hl.table.n_rec
    rec = torch.empty(n_rec * 8 * n, dtype=torch.float64)
    outs, updates = host.trace_sequential(hl, rin, w, bool(per_ray_w), int(start_surface),
                                          rec if n_rec else None)
    hl.last_schedule = updates.numpy().reshape(1, -1) if hl.newton else None
    sched = updates if hl.newton else torch.empty(0, dtype=torch.int32)
    return (*outs, rec, sched)


@trace_sequential.register_fake
def _(lens, lens_meta, final_thickness, lens_key, rays, w, params, spec, start_surface,
      per_ray_w):
    n = rays[0].numel()
    outs = [rays[0].new_empty(n, dtype=torch.float64) for _ in range(8)]
    rec = rays[0].new_empty(lens_meta[7] * 8 * n, dtype=torch.float64)
    ns = lens_meta[0] if lens_meta[8] else 0
    return (*outs, rec, rays[0].new_empty(ns, dtype=torch.int32))


def _seq_setup(ctx, inputs, output):
    lens, meta, ft, key, rays, w, params, spec, start_surface, per_ray_w = inputs
    ctx.lens_meta, ctx.final_thickness, ctx.lens_key = list(meta), float(ft), int(key)
    ctx.n_lens = len(lens)
    ctx.pairs = _spec_pairs(spec)
    ctx.start_surface = int(start_surface)
    ctx.per_ray_w = bool(per_ray_w)
    ctx.shapes = [(p.shape, p.dtype, p.device) for p in params]
    ctx.n_spec = len(spec)
    ctx.ray_meta = [(r.shape, r.dtype) for r in rays]
    ctx.set_materialize_grads(False)
    rec, sched = output[8], output[9]
    saved = list(lens) + [r.detach() for r in rays] + [rec, sched]
    if w is not None:
        saved.append(w.detach())
    ctx.has_w = w is not None
    ctx.save_for_backward(*saved)


def _seq_backward(ctx, *grads):
    saved = ctx.saved_tensors
    nl = ctx.n_lens
    lens = list(saved[:nl])
    rays_in, rec, sched = list(saved[nl:nl + 8]), saved[nl + 8], saved[nl + 9]
    w = saved[nl + 10] if ctx.has_w else None
    dl = _resolve(lens, ctx.lens_meta, ctx.final_thickness, ctx.lens_key)
    table = dl.table
    want_rays = any(ctx.needs_input_grad[4])  # list inputs: one bool per element
    want_params = any(ctx.needs_input_grad[6]) and len(ctx.shapes) > 0
    cot = [None if g is None else g.detach().to(torch.float64).reshape(-1).contiguous()
           for g in grads[:8]]
    rec_cot = grads[8]
    if rec_cot is not None:
        rec_cot = rec_cot.detach().to(torch.float64).reshape(-1).contiguous()
    # Tensor-list arguments take a list of Nones; the int lists are one leaf each, except an
    # empty `spec` (then it reads as an empty tensor list)
    none_rays, none_params = [None] * 8, [None] * len(ctx.shapes)
    none_spec = [] if ctx.n_spec == 0 else None
    nothing = ([None] * ctx.n_lens, None, None, None)
    if not (want_rays or want_params) or (all(c is None for c in cot) and rec_cot is None):
        return (*nothing, none_rays, None, none_params, none_spec, None, None)
    _check_differentiable(table, adjoint=want_rays)
    params_like = [torch.empty(s, dtype=d, device="meta") for s, d, _ in ctx.shapes]
    zp, st, ft, n_param = tangent_tables(table, ctx.pairs, params_like)
    from .autodiff import schedule_for_mode, vjp_mode

    mode = vjp_mode(table, schedule_for_mode(table, sched))
    if not (want_params and n_param):
        zp = st = ft = None
        n_param = 0
        mode = _abi.VJP_ADJOINT  # input-ray cotangents: the reverse-mode pass
    tabs = _tables_cpu(zp, st, ft, slot_need(table, zp, st, ft) if mode == _abi.VJP_ADJOINT
                       else None)
    g, gin = torch.ops.ort.trace_sequential_vjp(
        lens, ctx.lens_meta, ctx.final_thickness, ctx.lens_key, rays_in, w, sched, rec, cot,
        rec_cot, tabs, n_param, int(mode), ctx.start_surface, ctx.per_ray_w, bool(want_rays))
    if want_rays and mode != _abi.VJP_ADJOINT:
        # input-ray cotangents come from the reverse-mode pass (forward mode carries only the
        # parameter tangents): one adjoint launch with no parameters
        _, gin = torch.ops.ort.trace_sequential_vjp(
            lens, ctx.lens_meta, ctx.final_thickness, ctx.lens_key, rays_in, w, sched, rec,
            cot, rec_cot, [None, None, None, None], 0, int(_abi.VJP_ADJOINT),
            ctx.start_surface, ctx.per_ray_w, True)
    ray_grads = none_rays
    if want_rays:
        ray_grads = [gi.reshape(s).to(d) for gi, (s, d) in zip(gin, ctx.ray_meta, strict=True)]
    param_grads = _split_param_grads(g, ctx.shapes) if want_params else none_params
    return (*nothing, ray_grads, None, param_grads, none_spec, None, None)


def _tables_cpu(zp, st, ft, need):
    """The tangent tables as host tensors (the VJP ops' `tables` argument)."""
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a))
            for a in (zp, st, ft, need)]


trace_sequential.register_autograd(_seq_backward, setup_context=_seq_setup)


# --------------------------------------------------------------------------------------
# ort::trace_sequential_vjp -- the backward as its own op (traceable: fake + kernels)
# --------------------------------------------------------------------------------------
@torch.library.custom_op("ort::trace_sequential_vjp", mutates_args=(), device_types="cuda")
def trace_sequential_vjp(lens: list[torch.Tensor], lens_meta: list[int], final_thickness: float,
                         lens_key: int, rays_in: list[torch.Tensor], w: torch.Tensor | None,
                         sched: torch.Tensor, rec: torch.Tensor,
                         cot: list[torch.Tensor | None], rec_cot: torch.Tensor | None,
                         tables: list[torch.Tensor | None], n_param: int, mode: int,
                         start_surface: int, per_ray_w: bool,
                         want_rays: bool) -> tuple[torch.Tensor, list[torch.Tensor]]:
    """ort_trace_sequential_vjp: (grad [max(1, n_param)] = J^T cot w.r.t. the parameters of
    the tangent tables (zern_param, surf_tangent, final_tangent, slot_need), the input-ray
    cotangents [8][n] when want_rays, else [])."""
    dl = _resolve(lens, lens_meta, final_thickness, lens_key)
    return _seq_vjp_run(dl, rays_in, w, sched, rec, cot, rec_cot, tables, n_param, mode,
                        start_surface, per_ray_w, want_rays)


# the CPU dispatch key: the same function (_seq_vjp hands a HostLens to the host library)
trace_sequential_vjp.register_kernel("cpu")(trace_sequential_vjp._init_fn)


@trace_sequential_vjp.register_fake
def _(lens, lens_meta, final_thickness, lens_key, rays_in, w, sched, rec, cot, rec_cot, tables,
      n_param, mode, start_surface, per_ray_w, want_rays):
    n = rays_in[0].numel()
    g = rays_in[0].new_empty(max(1, n_param), dtype=torch.float64)
    gin = [rays_in[0].new_empty(n, dtype=torch.float64) for _ in range(8)] if want_rays else []
    return g, gin


def _seq_vjp_run(dl, rays_in, w, sched, rec, cot, rec_cot, tables, n_param, mode,
                 start_surface, per_ray_w, want_rays):
    dev = dl.device
    n = rays_in[0].numel()
    rays_in = [t.detach().to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
               for t in rays_in]
    cot = [None if c is None else c.detach().to(device=dev, dtype=torch.float64).reshape(-1)
           .contiguous() for c in cot]
    g = torch.zeros(max(1, n_param), dtype=torch.float64, device=dev)
    gin = [torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(8)] if want_rays else None
    zp, st, ft, need = (None if t is None else t.detach().cpu().numpy() for t in tables)
    _seq_vjp(dl, rays_in, w, per_ray_w, start_surface, sched, zp, st, ft, n_param, cot,
             rec_cot, rec, g if n_param else None, gin, mode, need)
    return g, (gin if want_rays else [])


def _seq_vjp(dl, rays_in, w, per_ray_w, start_surface, sched, zp, st, ft, n_param, cot,
             rec_cot, rec, grad, gin, mode, need=None):
    """One ort_trace_sequential_vjp call (grad += J^T cot, gin = input-ray cotangents); on
    a HostLens the host library's ort_host_trace_sequential_vjp."""
    from . import host
    from .raytrace import _stream_handle

    if need is None and mode == _abi.VJP_ADJOINT and zp is not None:
        need = slot_need(dl.table, zp, st, ft)
    tabs = [None if a is None else dl.resident(("seq_tangent", i), a)
            for i, a in enumerate((zp, st, ft))]
    need_t = None if need is None else dl.resident("seq_need", need)
    if isinstance(dl, host.HostLens):
        host.trace_sequential_vjp(dl, rays_in, w, per_ray_w, start_surface, sched, tabs, need_t,
                                  n_param, mode, cot, rec_cot, rec, grad, gin)
        return

    lib = _native.load()
    n = rays_in[0].numel()
    batch = _calls.resident_batch(n)
    w_keep = None
    if per_ray_w:
        w_keep = _calls.per_ray_wavelengths(dl.table, w, n, dl.device, validate=False)
        batch.w = addr(w_keep)
    sched_dev = sched if sched is not None and sched.numel() else None
    opt = _native.ort_options(_abi.NEWTON_SCHEDULE, int(start_surface), addr(sched_dev))
    params = _calls.vjp_params(dl.table, n_param, mode, tabs, need_t, grad_init=False)
    _calls.attach_vjp_workspace(lib, dl.c, batch, params, "seq_vjp", dl.device)
    rin_c = _calls.rays_struct(rays_in)
    cot_c = _calls.rays_struct(cot)
    gin_c = _calls.rays_struct(gin if gin is not None else [None] * 8)
    rc = lib.ort_trace_sequential_vjp(C.byref(dl.c), C.byref(rin_c), C.byref(batch),
                                      C.byref(opt), C.byref(params), C.byref(cot_c),
                                      addr(rec_cot), addr(rec if rec_cot is not None else None),
                                      addr(grad), C.byref(gin_c), _stream_handle())
    _native.check(rc, "ort_trace_sequential_vjp")
    del w_keep, tabs  # ordered on the stream before any reuse of their memory


# --------------------------------------------------------------------------------------
# ort::trace_pupil
# --------------------------------------------------------------------------------------
def plan_args(plan):
    """(seg, apod, plan_meta, plan_key) of a PupilPlan: the segment descriptors (SEGMENT
    records as bytes on the lens's device), the apodization record (or None), [n, seg_len,
    pupil_per_ray, newton mode index, want_tape, want_rms] and the plan's handle (its Newton
    schedule cache keys; a cache key only)."""
    dl = plan.dlens
    seg = _calls.segments_of(dl, plan.seg_dev)
    apod = dl.apod
    meta = [plan.n, plan.seg_len, int(plan.pupil_per_ray),
            NEWTON_MODES.index(plan.newton_mode), int(bool(plan.want_tape)),
            int(bool(plan.want_rms))]
    return seg, apod, meta, handle(plan)


def _want_rms(plan_meta):
    """plan_meta's want_rms entry (absent: 0)"""
    return int(plan_meta[5]) if len(plan_meta) > 5 else 0


def _plan_keys(plan_key):
    """The Newton schedule cache keys of the plan (raytrace._run falls back to per-group
    keys when there are none)."""
    p = _HANDLES.get(int(plan_key))
    return list(getattr(p, "keys", ()) or ())


@torch.library.custom_op("ort::trace_pupil", mutates_args=(), device_types="cuda")
def trace_pupil(lens: list[torch.Tensor], lens_meta: list[int], final_thickness: float,
                lens_key: int, seg: torch.Tensor, apod: torch.Tensor | None, px: torch.Tensor,
                py: torch.Tensor, params: list[torch.Tensor], spec: list[int],
                plan_meta: list[int], plan_key: int) -> tuple[
        torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
        torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Optic.trace's fused generation + trace (ort_trace_pupil): outputs the 8 ray columns,
    the verified Newton schedule, the adjoint tape (empty unless plan_meta asks for it:
    the backward is then the reverse sweep only; every row written, tape_rows per ray),
    and RayOperand.rms_spot_size of the final points with its stats[5] (empty
    unless plan_meta's want_rms: the rows in the taped kernel's epilogue, ort_rms_finish;
    its gradient folds into the backward's x, y cotangents)."""
    from .raytrace import RealRays
    from .raytrace import trace_pupil as _trace

    dl = _resolve(lens, lens_meta, final_thickness, lens_key)
    n, seg_len, ppr, mode, want_tape = plan_meta[:5]
    want_rms = _want_rms(plan_meta)
    if want_rms and not want_tape:
        raise ValueError("ort::trace_pupil: want_rms needs the taped forward (want_tape)")
    out = RealRays.of([torch.empty(n, dtype=torch.float64, device=dl.device) for _ in range(8)])
    tape = torch.empty(tape_doubles(dl, n) if want_tape else 0, dtype=torch.float64,
                       device=dl.device)
    rms = torch.empty(() if want_rms else 0, dtype=torch.float64, device=dl.device)
    rms_stats = torch.empty(5 if want_rms else 0, dtype=torch.float64, device=dl.device)
    if want_rms and n == 0:  # the mean over no points: NaN (no finish launch runs)
        rms.fill_(float("nan"))
        rms_stats.fill_(float("nan"))
    _trace(dl, seg, px, py, out, n, seg_len, n, keys=_plan_keys(plan_key),
           pupil_per_ray=bool(ppr), newton_mode=NEWTON_MODES[mode],
           tape=tape if want_tape else None, rms=(rms, rms_stats) if want_rms else None)
    return (*(getattr(out, a) for a in _abi.RAY_FIELDS), _schedule_tensor(dl), tape, rms,
            rms_stats)


@trace_pupil.register_kernel("cpu")
def _trace_pupil_cpu(lens, lens_meta, final_thickness, lens_key, seg, apod, px, py, params,
                     spec, plan_meta, plan_key):
    """The CPU dispatch key: rays generated and traced by the host build (host.py), the
    Newton stop rule evaluated exactly per (field, wavelength) group; no tape (the host
    backward re-traces); want_rms: ort_host_rms_spot of the outputs."""
    from . import host

    hl = _resolve(lens, lens_meta, final_thickness, lens_key)
    n, seg_len, ppr = plan_meta[:3]
    outs, updates = host.trace_pupil(hl, seg, px.detach().contiguous(), py.detach().contiguous(),
                                     n, seg_len, bool(ppr), apod)
    sched = updates if hl.newton else torch.empty(0, dtype=torch.int32)
    if _want_rms(plan_meta):
        rms, rms_stats = host.rms_spot(outs[0], outs[1])
    else:
        rms, rms_stats = (torch.empty(0, dtype=torch.float64) for _ in range(2))
    return (*outs, sched, torch.empty(0, dtype=torch.float64), rms, rms_stats)


@trace_pupil.register_fake
def _(lens, lens_meta, final_thickness, lens_key, seg, apod, px, py, params, spec, plan_meta,
      plan_key):
    n, seg_len, _, _, want_tape = plan_meta[:5]
    want_rms = _want_rms(plan_meta)
    outs = [px.new_empty(n, dtype=torch.float64) for _ in range(8)]
    S = lens_meta[0]
    ns = S if lens_meta[8] else 0  # one Newton group per call (group_len = n)
    nt = lens_meta[9] * n if (want_tape and px.device.type != "cpu") else 0  # tape_rows
    return (*outs, px.new_empty(ns, dtype=torch.int32), px.new_empty(nt, dtype=torch.float64),
            px.new_empty(() if want_rms else 0, dtype=torch.float64),
            px.new_empty(5 if want_rms else 0, dtype=torch.float64))


def _pupil_setup(ctx, inputs, output):
    lens, meta, ft, key, seg, apod, px, py, params, spec, plan_meta, plan_key = inputs
    ctx.lens_meta, ctx.final_thickness, ctx.lens_key = list(meta), float(ft), int(key)
    ctx.plan_meta, ctx.plan_key = list(plan_meta), int(plan_key)
    ctx.n_lens = len(lens)
    ctx.pairs = _spec_pairs(spec)
    ctx.n_spec = len(spec)
    ctx.shapes = [(p.shape, p.dtype, p.device) for p in params]
    ctx.has_apod = apod is not None
    ctx.set_materialize_grads(False)
    ctx.mark_non_differentiable(output[8], output[9], output[11])
    saved = [*lens, seg, px.detach(), py.detach(), output[8], output[9], output[11],
             *output[:8]]
    if apod is not None:
        saved.append(apod)
    ctx.save_for_backward(*saved)


def _pupil_backward(ctx, *grads):
    saved = ctx.saved_tensors
    nl = ctx.n_lens
    lens = list(saved[:nl])
    seg, px, py, sched, tape, rms_stats = saved[nl:nl + 6]
    primal = list(saved[nl + 6:nl + 14])
    apod = saved[nl + 14] if ctx.has_apod else None
    none_spec = [] if ctx.n_spec == 0 else None  # see _seq_backward
    nothing = ([None] * ctx.n_lens, None, None, None, None, None, None, None)
    if not any(ctx.needs_input_grad[8]) or not ctx.shapes:
        return (*nothing, [None] * len(ctx.shapes), none_spec, None, None)
    dl = _resolve(lens, ctx.lens_meta, ctx.final_thickness, ctx.lens_key)
    _check_differentiable(dl.table)
    params_like = [torch.empty(s, dtype=d, device="meta") for s, d, _ in ctx.shapes]
    zp, st, ft, n_param = tangent_tables(dl.table, ctx.pairs, params_like)
    from .autodiff import schedule_for_mode, vjp_mode

    hint = None
    if hasattr(dl, "cached_schedule"):
        hint = dl.cached_schedule(_plan_keys(ctx.plan_key))
    mode = vjp_mode(dl.table, schedule_for_mode(dl.table, sched, hint))
    tabs = _tables_cpu(zp, st, ft, slot_need(dl.table, zp, st, ft))
    cot = [None if gr is None else gr.to(torch.float64).contiguous() for gr in grads[:8]]
    g_rms = grads[10] if _want_rms(ctx.plan_meta) else None  # (AOT: zeros of an empty output)
    if g_rms is not None:
        g_rms = g_rms.detach().to(torch.float64).reshape(1)
    if all(c is None for c in cot) and g_rms is None:
        return (*nothing, [None] * len(ctx.shapes), none_spec, None, None)
    g = torch.ops.ort.trace_pupil_vjp(lens, ctx.lens_meta, ctx.final_thickness, ctx.lens_key,
                                      seg, apod, px, py, sched, tape, primal, cot, tabs,
                                      n_param, int(mode), ctx.plan_meta,
                                      rms_stats if g_rms is not None else None, g_rms)
    return (*nothing, _split_param_grads(g, ctx.shapes), none_spec, None, None)


trace_pupil.register_autograd(_pupil_backward, setup_context=_pupil_setup)


@torch.library.custom_op("ort::trace_pupil_vjp", mutates_args=(), device_types="cuda")
def trace_pupil_vjp(lens: list[torch.Tensor], lens_meta: list[int], final_thickness: float,
                    lens_key: int, seg: torch.Tensor, apod: torch.Tensor | None,
                    px: torch.Tensor, py: torch.Tensor, sched: torch.Tensor, tape: torch.Tensor,
                    primal: list[torch.Tensor], cot: list[torch.Tensor | None],
                    tables: list[torch.Tensor | None], n_param: int, mode: int,
                    plan_meta: list[int], rms_stats: torch.Tensor | None = None,
                    g_rms: torch.Tensor | None = None) -> torch.Tensor:
    """ort_trace_pupil_vjp: grad [n_param] = J^T cot (the reverse sweep over `tape` when the
    forward wrote one, else with its own re-trace). rms_stats / g_rms: the forward's rms
    spot size (its stats[5]) and its upstream gradient [1], folded into the x, y cotangents
    of the adjoint (ort_vjp_params.rms_stats / rms_grad)."""
    from .autodiff import vjp

    dl = _resolve(lens, lens_meta, final_thickness, lens_key)
    n, seg_len, ppr = plan_meta[:3]
    dev = dl.device
    tabs = tuple(None if t is None else dl.resident(("tangent", i), t.detach().cpu().numpy())
                 for i, t in enumerate(tables))
    g = torch.empty(max(1, n_param), dtype=torch.float64, device=dev)  # overwritten
    cot = [None if c is None else c.detach().to(device=dev, dtype=torch.float64).contiguous()
           for c in cot]
    taped = tape.numel() > 0 and mode == _abi.VJP_ADJOINT
    rms = None
    if g_rms is not None:
        if rms_stats is None or mode != _abi.VJP_ADJOINT:
            raise ValueError("ort::trace_pupil_vjp: g_rms needs rms_stats and the adjoint mode")
        rms = (rms_stats.detach().to(dev).contiguous(), g_rms.detach().to(dev).contiguous())
    vjp(dl, seg, px, py, n, seg_len, sched if sched.numel() else None, tabs, n_param, cot, g,
        pupil_per_ray=bool(ppr), mode=mode, tape=tape if taped else None,
        primal=primal if taped else None, overwrite=True, rms=rms)
    return g


@trace_pupil_vjp.register_kernel("cpu")
def _trace_pupil_vjp_cpu(lens, lens_meta, final_thickness, lens_key, seg, apod, px, py, sched,
                         tape, primal, cot, tables, n_param, mode, plan_meta, rms_stats=None,
                         g_rms=None):
    from . import host

    hl = _resolve(lens, lens_meta, final_thickness, lens_key)
    n, seg_len, ppr = plan_meta[:3]
    zp, st, ft, need = (None if t is None else t.detach().contiguous() for t in tables)
    g = torch.empty(max(1, n_param), dtype=torch.float64)
    cot = [None if c is None else c.detach().to(torch.float64).contiguous() for c in cot]
    host.trace_pupil_vjp(hl, seg, px.detach().contiguous(), py.detach().contiguous(), n,
                         seg_len, bool(ppr), sched, (zp, st, ft),
                         need if mode == _abi.VJP_ADJOINT else None, n_param, mode, cot, g, apod,
                         rms=None if g_rms is None else (rms_stats.detach().contiguous(),
                                                         g_rms.detach().contiguous()))
    return g


@trace_pupil_vjp.register_fake
def _(lens, lens_meta, final_thickness, lens_key, seg, apod, px, py, sched, tape, primal, cot,
      tables, n_param, mode, plan_meta, rms_stats=None, g_rms=None):
    return px.new_empty(max(1, n_param), dtype=torch.float64)


# --------------------------------------------------------------------------------------
# ort::rms_spot -- RayOperand.rms_spot_size's reduction (optimization/operand/ray.py:300-340)
# --------------------------------------------------------------------------------------
def _rms_workspace(device, n):
    lib = _native.load()
    size = int(lib.ort_rms_spot_workspace_size(int(n)))
    _native.check(size if size < 0 else 0, "ort_rms_spot_workspace_size")
    return _calls.workspace("rms", device, size), size


@torch.library.custom_op("ort::rms_spot", mutates_args=(), device_types="cuda")
def rms_spot(x: torch.Tensor, y: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(rms, stats[5] = n, mean x, mean y, rms, max radius): sqrt(mean((x - mean x)^2 +
    (y - mean y)^2)) as the reference's operand forms it, two deterministic passes on the
    device (ort_rms_spot), no host synchronisation."""
    from .raytrace import _stream_handle

    lib = _native.load()
    _check_rms_inputs(x, y)
    x = x.detach().reshape(-1).contiguous()
    y = y.detach().reshape(-1).contiguous()
    n = x.numel()
    ws, size = _rms_workspace(x.device, n)
    stats = torch.empty(5, dtype=torch.float64, device=x.device)
    rms = torch.empty((), dtype=torch.float64, device=x.device)
    rc = lib.ort_rms_spot(addr(x), addr(y), n, addr(ws), size, addr(stats), addr(rms),
                          _stream_handle())
    _native.check(rc, "ort_rms_spot")
    return rms, stats


@rms_spot.register_kernel("cpu")
def _rms_spot_cpu(x, y):
    """The CPU dispatch key: the same formula in the host library (sums in index order)."""
    from . import host

    _check_rms_inputs(x, y)
    return host.rms_spot(x.detach().reshape(-1).contiguous(), y.detach().reshape(-1).contiguous())


def _check_rms_inputs(x, y):
    """The kernels read x and y as n doubles each on one device: refuse anything else
    (a shorter y would be read past its end, a float32 record read as doubles)."""
    if x.dtype != torch.float64 or y.dtype != torch.float64:
        raise ValueError(f"ort::rms_spot: x and y must be float64 (got {x.dtype}, {y.dtype})")
    if x.numel() != y.numel():
        raise ValueError(f"ort::rms_spot: x has {x.numel()} points, y {y.numel()}")
    if x.device != y.device:
        raise ValueError(f"ort::rms_spot: x on {x.device}, y on {y.device}")


@rms_spot.register_fake
def _(x, y):
    _check_rms_inputs(x, y)
    return x.new_empty((), dtype=torch.float64), x.new_empty(5, dtype=torch.float64)


def _rms_setup(ctx, inputs, output):
    x, y = inputs
    ctx.shapes = (x.shape, y.shape)
    ctx.set_materialize_grads(False)
    # stats (n, centroid, rms, max radius) are reported, not differentiated: mark them so a
    # loss built on them raises instead of silently getting a zero gradient
    ctx.mark_non_differentiable(output[1])
    ctx.save_for_backward(x.detach(), y.detach(), output[1])


def _rms_backward(ctx, g_rms, g_stats):
    if g_rms is None:
        return None, None
    x, y, stats = ctx.saved_tensors
    gx, gy = torch.ops.ort.rms_spot_vjp(x, y, stats, g_rms.detach().to(torch.float64))
    return gx.reshape(ctx.shapes[0]), gy.reshape(ctx.shapes[1])


rms_spot.register_autograd(_rms_backward, setup_context=_rms_setup)


@torch.library.custom_op("ort::rms_spot_vjp", mutates_args=(), device_types="cuda")
def rms_spot_vjp(x: torch.Tensor, y: torch.Tensor, stats: torch.Tensor,
                 g: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """ort_rms_spot_vjp: g (x - mean x, y - mean y) / (n rms) (one kernel)."""
    from .raytrace import _stream_handle

    xf = x.detach().reshape(-1).contiguous()
    yf = y.detach().reshape(-1).contiguous()
    gg = g.detach().to(torch.float64).contiguous()
    gx = torch.empty_like(xf)
    gy = torch.empty_like(yf)
    rc = _native.load().ort_rms_spot_vjp(addr(xf), addr(yf), xf.numel(), addr(stats), addr(gg),
                                         addr(gx), addr(gy), _stream_handle())
    _native.check(rc, "ort_rms_spot_vjp")
    return gx, gy


@rms_spot_vjp.register_kernel("cpu")
def _rms_spot_vjp_cpu(x, y, stats, g):
    from . import host

    return host.rms_spot_vjp(x.detach().reshape(-1).contiguous(), y.detach().reshape(-1)
                             .contiguous(), stats.contiguous(), g.detach().to(torch.float64)
                             .reshape(1).contiguous())


@rms_spot_vjp.register_fake
def _(x, y, stats, g):
    return (x.new_empty(x.numel(), dtype=torch.float64),
            y.new_empty(y.numel(), dtype=torch.float64))


# --------------------------------------------------------------------------------------
# ort::huygens_psf -- HuygensPSF's summation (psf/huygens_fresnel_strategies.py:97-172)
# --------------------------------------------------------------------------------------
def _check_huygens_inputs(image, pupil, wavelength_mm):
    """The kernels read every array as doubles of one device: three image arrays of one
    size, five pupil arrays of one size."""
    for t in (*image, *pupil):
        if t.dtype != torch.float64:
            raise ValueError(f"ort::huygens_psf: every tensor must be float64 (got {t.dtype})")
        if t.device != image[0].device:
            raise ValueError(f"ort::huygens_psf: tensors on {image[0].device} and {t.device}")
    if any(t.shape != image[0].shape for t in image):
        raise ValueError("ort::huygens_psf: image_x, image_y, image_z of different shapes")
    if any(t.numel() != pupil[0].numel() for t in pupil):
        raise ValueError("ort::huygens_psf: pupil arrays of different sizes")
    if not wavelength_mm > 0.0:
        raise ValueError(f"ort::huygens_psf: wavelength_mm must be positive (got {wavelength_mm})")


def _flat(ts):
    return [t.detach().reshape(-1).contiguous() for t in ts]


@torch.library.custom_op("ort::huygens_psf", mutates_args=(), device_types="cuda")
def huygens_psf(image_x: torch.Tensor, image_y: torch.Tensor, image_z: torch.Tensor,
                pupil_x: torch.Tensor, pupil_y: torch.Tensor, pupil_z: torch.Tensor,
                amp: torch.Tensor, opd_mm: torch.Tensor, wavelength_mm: float,
                rp: float) -> torch.Tensor:
    """ort_huygens_psf: the raw |field|^2 at every image point (any shape; the output takes
    it) of the Huygens-Fresnel sum over the exit-pupil points -- one fused fp64 kernel over
    (image tile, pupil chunk) and a fixed-order sum of the chunk partials on the current
    stream, no host synchronisation. Not differentiable (yet): a requires_grad input
    raises NotImplementedError."""
    from .raytrace import _stream_handle

    lib = _native.load()
    image, pupil = (image_x, image_y, image_z), (pupil_x, pupil_y, pupil_z, amp, opd_mm)
    _check_huygens_inputs(image, pupil, wavelength_mm)
    fi, fp = _flat(image), _flat(pupil)
    n_i, n_p = fi[0].numel(), fp[0].numel()
    size = int(lib.ort_huygens_workspace_size(n_i, n_p))
    _native.check(size if size < 0 else 0, "ort_huygens_workspace_size")
    ws = torch.empty(max(size, 8), dtype=torch.uint8, device=image_x.device)
    psf = torch.empty(n_i, dtype=torch.float64, device=image_x.device)
    rc = lib.ort_huygens_psf(*(addr(t) for t in fi), n_i, *(addr(t) for t in fp), n_p,
                             float(wavelength_mm), float(rp), addr(psf), addr(ws), size,
                             _stream_handle())
    _native.check(rc, "ort_huygens_psf")
    return psf.reshape(image_x.shape)


@huygens_psf.register_kernel("cpu")
def _huygens_psf_cpu(image_x, image_y, image_z, pupil_x, pupil_y, pupil_z, amp, opd_mm,
                     wavelength_mm, rp):
    """The CPU dispatch key: the same term and summation order in the host library."""
    from . import host

    image, pupil = (image_x, image_y, image_z), (pupil_x, pupil_y, pupil_z, amp, opd_mm)
    _check_huygens_inputs(image, pupil, wavelength_mm)
    return host.huygens_psf(_flat(image), _flat(pupil), wavelength_mm, rp).reshape(image_x.shape)


@huygens_psf.register_fake
def _(image_x, image_y, image_z, pupil_x, pupil_y, pupil_z, amp, opd_mm, wavelength_mm, rp):
    _check_huygens_inputs((image_x, image_y, image_z), (pupil_x, pupil_y, pupil_z, amp, opd_mm),
                          wavelength_mm)
    return image_x.new_empty(image_x.shape, dtype=torch.float64)


_HUYGENS_NO_GRAD = ("ort::huygens_psf is not differentiable: autograd through the "
                    "Huygens-Fresnel PSF is not implemented (detach the inputs)")


def _huygens_setup(ctx, inputs, output):
    # refuse here, in the forward: a PSF that silently dropped its graph would give a loss
    # built on it a zero gradient
    if any(ctx.needs_input_grad):
        raise NotImplementedError(_HUYGENS_NO_GRAD)


def _huygens_backward(ctx, grad):
    raise NotImplementedError(_HUYGENS_NO_GRAD)


huygens_psf.register_autograd(_huygens_backward, setup_context=_huygens_setup)


# --------------------------------------------------------------------------------------
# ort::dft_psf -- the pupil-to-image transform of FFTPSF / MMDFTPSF / FFTMTF
# (psf/fft.py:169-234, psf/mmdft.py:164-184, 230-290)
# --------------------------------------------------------------------------------------
def _check_dft_inputs(amp, opd_waves, image_size, pad_size):
    """Two float64 contiguous tensors of one shape (n, n) or (B, n, n) on one device;
    -> (B, n, batched)."""
    for t in (amp, opd_waves):
        if t.dtype != torch.float64:
            raise ValueError(f"ort::dft_psf: every tensor must be float64 (got {t.dtype})")
        if not t.is_contiguous():
            raise ValueError("ort::dft_psf: amp and opd_waves must be contiguous")
    if amp.device != opd_waves.device:
        raise ValueError(f"ort::dft_psf: tensors on {amp.device} and {opd_waves.device}")
    if amp.shape != opd_waves.shape or amp.dim() not in (2, 3) or amp.shape[-1] != amp.shape[-2]:
        raise ValueError("ort::dft_psf: amp and opd_waves must both be (n, n) or (B, n, n) "
                         f"(got {tuple(amp.shape)} and {tuple(opd_waves.shape)})")
    n = int(amp.shape[-1])
    if n == 0:
        raise ValueError("ort::dft_psf: the pupil grid is empty (n == 0)")
    if not pad_size > 0.0 or pad_size == float("inf"):
        raise ValueError(f"ort::dft_psf: pad_size must be positive and finite (got {pad_size})")
    if image_size < 0 or max(n, image_size) > _abi.DFT_MAX_SIZE:
        raise ValueError(f"ort::dft_psf: n and image_size must lie in [0, {_abi.DFT_MAX_SIZE}] "
                         f"(got {n} and {image_size})")
    return (int(amp.shape[0]) if amp.dim() == 3 else 1), n, amp.dim() == 3


def _dft_shape(batch, batched, m):
    return (batch, m, m) if batched else (m, m)


@torch.library.custom_op("ort::dft_psf", mutates_args=(), device_types="cuda")
def dft_psf(amp: torch.Tensor, opd_waves: torch.Tensor, image_size: int,
            pad_size: float) -> torch.Tensor:
    """ort_dft_psf on the current stream: |sum_jk amp exp(-2 pi i opd_waves) exp(-2 pi i ((v -
    m/2)(j - n/2) + (u - m/2)(k - n/2)) / pad_size)|^2 for v, u in [0, image_size) -- the raw
    image intensity of FFTPSF (pad_size = image_size = grid_size) and MMDFTPSF, of one (n, n)
    pupil or a batch (B, n, n) in one pair of launches; no host synchronisation. Not
    differentiable: a requires_grad input raises NotImplementedError."""
    from .raytrace import _stream_handle

    lib = _native.load()
    batch, n, batched = _check_dft_inputs(amp, opd_waves, image_size, pad_size)
    m = int(image_size)
    out = torch.empty(_dft_shape(batch, batched, m), dtype=torch.float64, device=amp.device)
    size = int(lib.ort_dft_workspace_size(batch, n, m))
    _native.check(size if size < 0 else 0, "ort_dft_workspace_size")
    ws = torch.empty(max(size, 8), dtype=torch.uint8, device=amp.device)
    rc = lib.ort_dft_psf(addr(amp.detach()), addr(opd_waves.detach()), batch, n, m,
                         float(pad_size), addr(out), addr(ws), size, _stream_handle())
    _native.check(rc, "ort_dft_psf")
    return out


@dft_psf.register_kernel("cpu")
def _dft_psf_cpu(amp, opd_waves, image_size, pad_size):
    """The CPU dispatch key: the same terms and summation order in the host library."""
    from . import host

    batch, n, batched = _check_dft_inputs(amp, opd_waves, image_size, pad_size)
    m = int(image_size)
    out = host.dft_psf(amp.detach(), opd_waves.detach(), batch, n, m, pad_size)
    return out.reshape(_dft_shape(batch, batched, m))


@dft_psf.register_fake
def _(amp, opd_waves, image_size, pad_size):
    batch, _, batched = _check_dft_inputs(amp, opd_waves, image_size, pad_size)
    return amp.new_empty(_dft_shape(batch, batched, int(image_size)), dtype=torch.float64)


_DFT_NO_GRAD = ("ort::dft_psf is not differentiable: autograd through the FFT / MMDFT PSF is "
                "not implemented (detach the inputs)")


def _dft_setup(ctx, inputs, output):
    # refuse in the forward, as ort::huygens_psf does
    if any(ctx.needs_input_grad):
        raise NotImplementedError(_DFT_NO_GRAD)


def _dft_backward(ctx, grad):
    raise NotImplementedError(_DFT_NO_GRAD)


dft_psf.register_autograd(_dft_backward, setup_context=_dft_setup)


# --------------------------------------------------------------------------------------
# ort::sampled_otf -- SampledMTF's overlap sum over pupil shears (mtf/sampled.py:162-205)
# --------------------------------------------------------------------------------------
_OTF_KINDS = ("fringe", "standard", "noll")
_otf_term_cache: dict = {}


def _otf_terms(kind, n_terms, device):
    """The term structure of the first n_terms polynomials of a scheme for ort_sampled_otf:
    the ort_zernike_term records (c unused) and their radial weights a_k, from
    geometries._zernike_structure -- as NumPy arrays on the host, as (uint8 records, float64
    weights) tensors on a device; built once per (scheme, count, device)."""
    key = (kind, int(n_terms), str(device))
    hit = _otf_term_cache.get(key)
    if hit is not None:
        return hit
    from .geometries import _zernike_structure

    terms = np.zeros(max(1, n_terms), dtype=_abi.ZERNIKE_TERM)
    radial = []
    for j, (norm, n, m, a, _d) in enumerate(_zernike_structure(kind, int(n_terms))):
        terms[j] = (0.0, norm, n, m, len(radial), len(a))
        radial.extend(a)
    radial = np.asarray(radial or [0.0], dtype=np.float64)
    if torch.device(device).type == "cpu":
        out = (terms, radial)
    else:
        out = (_calls.bytes_tensor(terms).to(device), torch.from_numpy(radial).to(device))
    _otf_term_cache[key] = out
    return out


def _check_sampled_otf_inputs(x, y, intensity, opd_waves, coeffs, kind, shift_x, shift_y):
    """The kernels read every array as doubles of one device: x, y of one size N, intensity
    and opd_waves [N] or [B, N], coeffs [T] or [B, T], two shear arrays of one size.
    -> (B, N, T, F, batched)."""
    for t in (x, y, intensity, opd_waves, coeffs, shift_x, shift_y):
        if t.dtype != torch.float64:
            raise ValueError(f"ort::sampled_otf: every tensor must be float64 (got {t.dtype})")
        if t.device != x.device:
            raise ValueError(f"ort::sampled_otf: tensors on {x.device} and {t.device}")
    if kind not in _OTF_KINDS:
        raise ValueError(f"ort::sampled_otf: kind must be one of {list(_OTF_KINDS)} (got {kind!r})")
    if x.dim() != 1 or y.shape != x.shape:
        raise ValueError("ort::sampled_otf: x and y must be 1-D of one size")
    if shift_x.dim() != 1 or shift_y.shape != shift_x.shape:
        raise ValueError("ort::sampled_otf: shift_x and shift_y must be 1-D of one size")
    n = x.numel()
    batched = intensity.dim() == 2
    if (intensity.dim() not in (1, 2) or opd_waves.shape != intensity.shape
            or intensity.shape[-1] != n):
        raise ValueError("ort::sampled_otf: intensity and opd_waves must both be (N,) or (B, N) "
                         f"with N = {n} (got {tuple(intensity.shape)} and "
                         f"{tuple(opd_waves.shape)})")
    if coeffs.dim() != intensity.dim() or (batched and coeffs.shape[0] != intensity.shape[0]):
        raise ValueError("ort::sampled_otf: coeffs must be (T,) for unbatched and (B, T) for "
                         f"batched pupils (got {tuple(coeffs.shape)})")
    b = intensity.shape[0] if batched else 1
    return b, n, coeffs.shape[-1], shift_x.numel(), batched


def _otf_shape(b, f, batched):
    return (b, f, 2) if batched else (f, 2)


@torch.library.custom_op("ort::sampled_otf", mutates_args=(), device_types="cuda")
def sampled_otf(x: torch.Tensor, y: torch.Tensor, intensity: torch.Tensor,
                opd_waves: torch.Tensor, coeffs: torch.Tensor, kind: str,
                shift_x: torch.Tensor, shift_y: torch.Tensor) -> torch.Tensor:
    """ort_sampled_otf on the current stream: otf[b, f] = sum_j [r <= 1] I_bj exp(2 pi i (opd_bj
    - W_b(x_j - shift_x[f], y_j - shift_y[f]))) as (re, im), W_b the polynomial of scheme
    `kind` with coefficients coeffs[b] -- every frequency and batch entry in one launch pair,
    no host synchronisation. (N,) pupils give [F, 2], (B, N) pupils [B, F, 2]. Forward only: a
    requires_grad input raises NotImplementedError."""
    from .raytrace import _stream_handle

    lib = _native.load()
    b, n, t, f, batched = _check_sampled_otf_inputs(x, y, intensity, opd_waves, coeffs, kind,
                                                    shift_x, shift_y)
    terms, radial = _otf_terms(kind, t, x.device)
    out = torch.empty(_otf_shape(b, f, batched), dtype=torch.float64, device=x.device)
    size = int(lib.ort_sampled_otf_workspace_size(b, f, n))
    _native.check(size if size < 0 else 0, "ort_sampled_otf_workspace_size")
    ws = torch.empty(max(size, 8), dtype=torch.uint8, device=x.device)
    args = [v.detach().contiguous() for v in (x, y, intensity, opd_waves, coeffs, shift_x,
                                              shift_y)]
    rc = lib.ort_sampled_otf(addr(args[0]), addr(args[1]), n, addr(args[2]), addr(args[3]), b,
                             addr(terms), addr(radial), addr(args[4]), t, addr(args[5]),
                             addr(args[6]), f, addr(out), addr(ws), size, _stream_handle())
    _native.check(rc, "ort_sampled_otf")
    return out


@sampled_otf.register_kernel("cpu")
def _sampled_otf_cpu(x, y, intensity, opd_waves, coeffs, kind, shift_x, shift_y):
    """The CPU dispatch key: the same term and summation order in the host library."""
    from . import host

    b, n, t, f, batched = _check_sampled_otf_inputs(x, y, intensity, opd_waves, coeffs, kind,
                                                    shift_x, shift_y)
    terms, radial = _otf_terms(kind, t, "cpu")
    args = [v.detach().contiguous() for v in (x, y, intensity, opd_waves, coeffs, shift_x,
                                              shift_y)]
    return host.sampled_otf(args, b, t, terms, radial).reshape(_otf_shape(b, f, batched))


@sampled_otf.register_fake
def _(x, y, intensity, opd_waves, coeffs, kind, shift_x, shift_y):
    b, _, _, f, batched = _check_sampled_otf_inputs(x, y, intensity, opd_waves, coeffs, kind,
                                                    shift_x, shift_y)
    return x.new_empty(_otf_shape(b, f, batched), dtype=torch.float64)


_SAMPLED_OTF_NO_GRAD = ("ort::sampled_otf is not differentiable: autograd through the Zernike "
                        "fit and the pupil shear is not implemented (detach the inputs)")


def _sampled_otf_setup(ctx, inputs, output):
    # refuse in the forward, as ort::huygens_psf does
    if any(ctx.needs_input_grad):
        raise NotImplementedError(_SAMPLED_OTF_NO_GRAD)


def _sampled_otf_backward(ctx, grad):
    raise NotImplementedError(_SAMPLED_OTF_NO_GRAD)


sampled_otf.register_autograd(_sampled_otf_backward, setup_context=_sampled_otf_setup)


# --------------------------------------------------------------------------------------
# ort::irradiance_bin -- IncoherentIrradiance's binning (analysis/irradiance.py:243-330)
# --------------------------------------------------------------------------------------
def _check_irradiance_inputs(x, y, power, x_edges, y_edges, mode, op="ort::irradiance_bin"):
    """What the kernels assume of the shapes (no data is read: the fake kernels run this
    too). Returns (nx, ny)."""
    for t in (x, y, power, x_edges, y_edges):
        if t.dtype != torch.float64:
            raise ValueError(f"{op}: every tensor must be float64 (got {t.dtype})")
        if t.device != x.device:
            raise ValueError(f"{op}: tensors on {x.device} and {t.device}")
    if not (x.numel() == y.numel() == power.numel()):
        raise ValueError(f"{op}: x, y, power of different lengths "
                         f"({x.numel()}, {y.numel()}, {power.numel()})")
    if x_edges.dim() != 1 or y_edges.dim() != 1:
        raise ValueError(f"{op}: x_edges and y_edges must be one-dimensional")
    if mode not in (_abi.BIN_HISTOGRAM, _abi.BIN_BILINEAR):
        raise ValueError(f"{op}: mode must be BIN_HISTOGRAM (0) or BIN_BILINEAR (1), got {mode}")
    nx, ny = x_edges.numel() - 1, y_edges.numel() - 1
    lo = 2 if mode == _abi.BIN_BILINEAR else 1
    if nx < lo or ny < lo:
        raise ValueError(f"{op}: needs at least {lo} pixel(s) along each axis in this mode "
                         f"(got {nx} x {ny})")
    if nx * ny > _abi.IRRADIANCE_MAX_PIXELS:
        raise ValueError(f"{op}: {nx} x {ny} pixels exceed the supported "
                         f"{_abi.IRRADIANCE_MAX_PIXELS}")
    return nx, ny


_edges_checked = {}  # id(tensor) -> (weakref, version): edge tensors already found increasing


def _check_edges_increasing(op, *edges):
    """Strictly increasing edges (NaN fails). The comparison reads device data, so a tensor
    that passed is remembered by identity and version: repeated calls on the same edge
    tensors (a loop over fields, an optimisation) do not synchronise again."""
    for e in edges:
        hit = _edges_checked.get(id(e))
        if hit is not None and hit[0]() is e and hit[1] == e._version:
            continue
        if not bool(torch.all(e[1:] > e[:-1])):
            raise ValueError(f"{op}: edges must be strictly increasing")
        if len(_edges_checked) >= 64:
            _edges_checked.clear()
        _edges_checked[id(e)] = (weakref.ref(e), e._version)


def _irr_shape(nx, ny, mode):
    return (nx, ny) if mode == _abi.BIN_HISTOGRAM else (ny, nx)


@torch.library.custom_op("ort::irradiance_bin", mutates_args=(), device_types="cuda")
def irradiance_bin(x: torch.Tensor, y: torch.Tensor, power: torch.Tensor,
                   x_edges: torch.Tensor, y_edges: torch.Tensor, mode: int,
                   pixel_area: float | None = None) -> torch.Tensor:
    """ort_irradiance_bin on the current stream: the power of the rays at (x, y) (the
    detector's frame) summed per pixel and divided by the pixel area (None: the first
    pixel's, from the edges). BIN_HISTOGRAM returns [nx, ny] (X is the row index, as
    numpy.histogram2d), BIN_BILINEAR [ny, nx] (Y is the row index, as the reference's
    index_put): the reference's two paths differ in orientation and so do these."""
    from .raytrace import _stream_handle

    lib = _native.load()
    nx, ny = _check_irradiance_inputs(x, y, power, x_edges, y_edges, mode)
    _check_edges_increasing("ort::irradiance_bin", x_edges, y_edges)
    fx, fy, fp, ex, ey = _flat((x, y, power, x_edges, y_edges))
    size = int(lib.ort_irradiance_workspace_size(nx, ny))
    _native.check(size if size < 0 else 0, "ort_irradiance_workspace_size")
    ws = torch.empty(size, dtype=torch.uint8, device=x.device)
    out = torch.empty(nx * ny, dtype=torch.float64, device=x.device)
    rc = lib.ort_irradiance_bin(addr(fx), addr(fy), addr(fp), fx.numel(), addr(ex), nx,
                                addr(ey), ny, int(mode), float(pixel_area or 0.0), addr(out),
                                addr(ws), size, _stream_handle())
    _native.check(rc, "ort_irradiance_bin")
    return out.reshape(_irr_shape(nx, ny, mode))


@irradiance_bin.register_kernel("cpu")
def _irradiance_bin_cpu(x, y, power, x_edges, y_edges, mode, pixel_area=None):
    """The CPU dispatch key: the same pixels, quantisation and finish in the host library."""
    from . import host

    nx, ny = _check_irradiance_inputs(x, y, power, x_edges, y_edges, mode)
    _check_edges_increasing("ort::irradiance_bin", x_edges, y_edges)
    out = host.irradiance_bin(*_flat((x, y, power, x_edges, y_edges)), mode,
                              float(pixel_area or 0.0))
    return out.reshape(_irr_shape(nx, ny, mode))


@irradiance_bin.register_fake
def _(x, y, power, x_edges, y_edges, mode, pixel_area=None):
    nx, ny = _check_irradiance_inputs(x, y, power, x_edges, y_edges, mode)
    return x.new_empty(_irr_shape(nx, ny, mode), dtype=torch.float64)


def _check_irradiance_grad(grad, nx, ny, device):
    if grad.dtype != torch.float64 or grad.device != device or grad.shape != (ny, nx):
        raise ValueError(f"ort::irradiance_bin_vjp: grad must be a float64 [{ny}, {nx}] tensor "
                         f"on {device} (got {grad.dtype} {tuple(grad.shape)} on {grad.device})")


@torch.library.custom_op("ort::irradiance_bin_vjp", mutates_args=(), device_types="cuda")
def irradiance_bin_vjp(x: torch.Tensor, y: torch.Tensor, power: torch.Tensor,
                       x_edges: torch.Tensor, y_edges: torch.Tensor, grad: torch.Tensor,
                       pixel_area: float | None = None
                       ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """ort_irradiance_bin_vjp: the gradients of a scalar with respect to x, y and power, given
    its gradient `grad` [ny, nx] with respect to the BIN_BILINEAR map."""
    from .raytrace import _stream_handle

    lib = _native.load()
    op = "ort::irradiance_bin_vjp"
    nx, ny = _check_irradiance_inputs(x, y, power, x_edges, y_edges, _abi.BIN_BILINEAR, op)
    _check_irradiance_grad(grad, nx, ny, x.device)
    _check_edges_increasing(op, x_edges, y_edges)
    fx, fy, fp, ex, ey, fg = _flat((x, y, power, x_edges, y_edges, grad))
    gx, gy, gp = (torch.empty(fx.numel(), dtype=torch.float64, device=x.device)
                  for _ in range(3))
    rc = lib.ort_irradiance_bin_vjp(addr(fx), addr(fy), addr(fp), fx.numel(), addr(ex), nx,
                                    addr(ey), ny, float(pixel_area or 0.0), addr(fg),
                                    addr(gx), addr(gy), addr(gp), _stream_handle())
    _native.check(rc, op)
    return gx.reshape(x.shape), gy.reshape(y.shape), gp.reshape(power.shape)


@irradiance_bin_vjp.register_kernel("cpu")
def _irradiance_bin_vjp_cpu(x, y, power, x_edges, y_edges, grad, pixel_area=None):
    from . import host

    op = "ort::irradiance_bin_vjp"
    nx, ny = _check_irradiance_inputs(x, y, power, x_edges, y_edges, _abi.BIN_BILINEAR, op)
    _check_irradiance_grad(grad, nx, ny, x.device)
    _check_edges_increasing(op, x_edges, y_edges)
    gx, gy, gp = host.irradiance_bin_vjp(*_flat((x, y, power, x_edges, y_edges, grad)),
                                         float(pixel_area or 0.0))
    return gx.reshape(x.shape), gy.reshape(y.shape), gp.reshape(power.shape)


@irradiance_bin_vjp.register_fake
def _(x, y, power, x_edges, y_edges, grad, pixel_area=None):
    nx, ny = _check_irradiance_inputs(x, y, power, x_edges, y_edges, _abi.BIN_BILINEAR,
                                      "ort::irradiance_bin_vjp")
    _check_irradiance_grad(grad, nx, ny, x.device)
    return (x.new_empty(x.shape, dtype=torch.float64), y.new_empty(y.shape, dtype=torch.float64),
            power.new_empty(power.shape, dtype=torch.float64))


_IRRADIANCE_NO_GRAD = ("ort::irradiance_bin: the histogram mode (BIN_HISTOGRAM) is piecewise "
                       "constant in x, y and is not differentiable; use the bilinear mode "
                       "(BIN_BILINEAR) for inputs that require grad, or detach them")


def _irradiance_setup(ctx, inputs, output):
    x, y, power, x_edges, y_edges, mode, pixel_area = inputs
    if mode != _abi.BIN_BILINEAR:
        # refuse in the forward, as ort::huygens_psf does: a map that silently dropped its
        # graph would give a loss built on it a zero gradient
        if any(ctx.needs_input_grad):
            raise NotImplementedError(_IRRADIANCE_NO_GRAD)
        return
    if any(ctx.needs_input_grad[3:5]):
        raise NotImplementedError("ort::irradiance_bin: no gradient with respect to the edges")
    ctx.save_for_backward(x, y, power, x_edges, y_edges)
    ctx.pixel_area = pixel_area


def _irradiance_backward(ctx, grad):
    x, y, power, x_edges, y_edges = ctx.saved_tensors
    gx, gy, gp = torch.ops.ort.irradiance_bin_vjp(x, y, power, x_edges, y_edges,
                                                  grad.contiguous(), ctx.pixel_area)
    need = ctx.needs_input_grad
    return (gx if need[0] else None, gy if need[1] else None, gp if need[2] else None,
            None, None, None, None)


irradiance_bin.register_autograd(_irradiance_backward, setup_context=_irradiance_setup)


# --------------------------------------------------------------------------------------
# ort::trace_pupil_polarized (coatings / polarization; forward only)
# --------------------------------------------------------------------------------------
def polarized_args(lens, segs, px, py, n, seg_len, mode, state, pupil_per_ray=False,
                   want_p=True):
    """The arguments of torch.ops.ort.trace_pupil_polarized for a DeviceLens / HostLens of a
    table lowered with polarized=True: the lens tensors, its COATING records and the
    SEGMENT / APODIZATION records as uint8 tensors on the lens's device, the pupil, the
    input field (ex_re, ex_im, ey_re, ey_im) and plan_meta = [n, seg_len, pupil_per_ray,
    mode, want_p]."""
    from . import polarization as pz

    L, meta, ft, key = lens_args(lens)
    ex = ey = 0j
    if mode == _abi.POL_POLARIZED:
        ex, ey = state.field()
    return (L, meta, ft, key, pz._coatings_of(lens), _calls.segments_of(lens, segs), lens.apod,
            px, py,
            [ex.real, ex.imag, ey.real, ey.imag],
            [int(n), int(seg_len), int(bool(pupil_per_ray)), int(mode), int(bool(want_p))])


@torch.library.custom_op("ort::trace_pupil_polarized", mutates_args=(), device_types="cuda")
def trace_pupil_polarized(lens: list[torch.Tensor], lens_meta: list[int],
                          final_thickness: float, lens_key: int, coatings: torch.Tensor,
                          seg: torch.Tensor, apod: torch.Tensor | None, px: torch.Tensor,
                          py: torch.Tensor, field: list[float],
                          plan_meta: list[int]) -> tuple[torch.Tensor, torch.Tensor]:
    """Optic.trace's fused generation + trace of a coated / polarized lens
    (ort_trace_pupil_polarized): the rays [8, n] (x y z L M N i opd, i per the mode) and
    the planes of the polarization matrices [18, n] ([18, 0] unless plan_meta's want_p).
    Forward only: a backward through it raises."""
    from . import polarization as pz

    dl = _resolve(lens, lens_meta, final_thickness, lens_key)
    n, seg_len, ppr, mode, want_p = plan_meta[:5]
    rays = torch.empty((8, n), dtype=torch.float64, device=dl.device)
    planes = torch.empty((18, n if want_p else 0), dtype=torch.float64, device=dl.device)
    pz.trace_pupil_polarized(
        dl, seg, px.detach().contiguous(), py.detach().contiguous(), n, seg_len, mode, None,
        pupil_per_ray=bool(ppr), want_p=bool(want_p),
        field=(complex(field[0], field[1]), complex(field[2], field[3])), coat=coatings,
        apod=apod, outs=list(rays.unbind(0)), planes=planes.view(-1) if want_p else None)
    return rays, planes


@trace_pupil_polarized.register_kernel("cpu")
def _trace_pupil_polarized_cpu(lens, lens_meta, final_thickness, lens_key, coatings, seg, apod,
                               px, py, field, plan_meta):
    """The CPU dispatch key: the host build (ort_host_trace_pupil_polarized)."""
    return trace_pupil_polarized._init_fn(lens, lens_meta, final_thickness, lens_key, coatings,
                                          seg, apod, px, py, field, plan_meta)


@trace_pupil_polarized.register_fake
def _(lens, lens_meta, final_thickness, lens_key, coatings, seg, apod, px, py, field,
      plan_meta):
    n, want_p = plan_meta[0], plan_meta[4]
    return (px.new_empty((8, n), dtype=torch.float64),
            px.new_empty((18, n if want_p else 0), dtype=torch.float64))


def _polarized_backward(ctx, *grads):
    raise RuntimeError("ort::trace_pupil_polarized is forward only: autograd through "
                       "coatings / polarization is not supported")


trace_pupil_polarized.register_autograd(_polarized_backward)


# --------------------------------------------------------------------------------------
# ort::trace_pupil_scatter / trace_sequential_scatter / bsdf_scatter (BSDF surfaces; forward
# only)
# --------------------------------------------------------------------------------------
def _seed64(seed):
    """A 64-bit seed as the ops carry it (a signed 64-bit int: two's complement)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed - (1 << 64) if seed >= (1 << 63) else seed


def scatter_args(lens, segs, px, py, n, seg_len, pupil_per_ray=False, ray_offset=0):
    """The arguments of torch.ops.ort.trace_pupil_scatter for a DeviceLens / HostLens of a
    table with BSDF surfaces: the lens tensors, its BSDF records and the SEGMENT /
    APODIZATION records as uint8 tensors on the lens's device, the pupil, the seed
    (lens.scatter) and plan_meta = [n, seg_len, pupil_per_ray, ray_offset, max_attempts]."""
    from . import scatter as sc

    L, meta, ft, key = lens_args(lens, scatter=True)
    sct, bsdf = sc.scatter_struct(lens)  # (the lens's seed and cap; its resident records)
    return (L, meta, ft, key, bsdf, _calls.segments_of(lens, segs), lens.apod, px, py,
            _seed64(sct.seed),
            [int(n), int(seg_len), int(bool(pupil_per_ray)), int(ray_offset), int(sct.max_attempts)])


def sequential_scatter_args(lens, rays_in, start_surface=0, ray_offset=0):
    """The arguments of torch.ops.ort.trace_sequential_scatter: rays_in [8, n] (x y z L M N
    i opd) on the lens's device; plan_meta = [start_surface, ray_offset, max_attempts]."""
    from . import scatter as sc

    L, meta, ft, key = lens_args(lens, scatter=True)
    sct, bsdf = sc.scatter_struct(lens)
    return (L, meta, ft, key, bsdf, rays_in, _seed64(sct.seed),
            [int(start_surface), int(ray_offset), int(sct.max_attempts)])


def _scatter_lens(lens, lens_meta, final_thickness, lens_key, bsdf, seed, cap):
    """The resolved lens carrying the op's BSDF records, seed and attempt cap (a lens
    rebuilt from its tensors has none of its own)."""
    dl = _resolve(lens, lens_meta, final_thickness, lens_key)
    rec = np.frombuffer(bsdf.detach().cpu().numpy().tobytes(), dtype=_abi.BSDF).copy()
    if dl.table.bsdf is None or dl.table.bsdf.tobytes() != rec.tobytes():
        dl.table.bsdf = rec
    dl.scatter = (int(seed) & 0xFFFFFFFFFFFFFFFF, int(cap))
    return dl


@torch.library.custom_op("ort::trace_pupil_scatter", mutates_args=(), device_types="cuda")
def trace_pupil_scatter(lens: list[torch.Tensor], lens_meta: list[int], final_thickness: float,
                        lens_key: int, bsdf: torch.Tensor, seg: torch.Tensor,
                        apod: torch.Tensor | None, px: torch.Tensor, py: torch.Tensor,
                        seed: int, plan_meta: list[int]) -> torch.Tensor:
    """Optic.trace's fused generation + trace of a lens with BSDF surfaces
    (ort_trace_pupil_scatter): the rays [8, n] (x y z L M N i opd). Ray r draws as ray
    r + ray_offset of the stream keyed by `seed`. Forward only: a backward raises."""
    n, seg_len, ppr, ray_offset, cap = plan_meta[:5]
    from . import raytrace

    dl = _scatter_lens(lens, lens_meta, final_thickness, lens_key, bsdf, seed, cap)
    rays = torch.empty((8, n), dtype=torch.float64, device=dl.device)
    raytrace.trace_pupil_on(dl, seg, px.detach().contiguous(), py.detach().contiguous(),
                            list(rays.unbind(0)), n, seg_len, bool(ppr),
                            ray_offset=ray_offset, apod=apod)
    return rays


@trace_pupil_scatter.register_kernel("cpu")
def _trace_pupil_scatter_cpu(lens, lens_meta, final_thickness, lens_key, bsdf, seg, apod, px,
                             py, seed, plan_meta):
    """The CPU dispatch key: the host build (ort_host_trace_pupil_scatter)."""
    return trace_pupil_scatter._init_fn(lens, lens_meta, final_thickness, lens_key, bsdf, seg,
                                        apod, px, py, seed, plan_meta)


@trace_pupil_scatter.register_fake
def _(lens, lens_meta, final_thickness, lens_key, bsdf, seg, apod, px, py, seed, plan_meta):
    return px.new_empty((8, plan_meta[0]), dtype=torch.float64)


@torch.library.custom_op("ort::trace_sequential_scatter", mutates_args=(), device_types="cuda")
def trace_sequential_scatter(lens: list[torch.Tensor], lens_meta: list[int],
                             final_thickness: float, lens_key: int, bsdf: torch.Tensor,
                             rays_in: torch.Tensor, seed: int,
                             plan_meta: list[int]) -> torch.Tensor:
    """SurfaceGroup.trace of resident rays [8, n] through a lens with BSDF surfaces
    (ort_trace_sequential_scatter): the traced rays [8, n]. Forward only."""
    start_surface, ray_offset, cap = plan_meta[:3]
    dl = _scatter_lens(lens, lens_meta, final_thickness, lens_key, bsdf, seed, cap)
    from . import raytrace

    rin = rays_in.detach().to(torch.float64).contiguous()
    rout = torch.empty_like(rin)
    raytrace.trace_rays_on(dl, list(rin.unbind(0)), list(rout.unbind(0)), start_surface,
                           ray_offset=ray_offset)
    return rout


@trace_sequential_scatter.register_kernel("cpu")
def _trace_sequential_scatter_cpu(lens, lens_meta, final_thickness, lens_key, bsdf, rays_in,
                                  seed, plan_meta):
    """The CPU dispatch key: the host build (ort_host_trace_sequential_scatter)."""
    return trace_sequential_scatter._init_fn(lens, lens_meta, final_thickness, lens_key, bsdf,
                                             rays_in, seed, plan_meta)


@trace_sequential_scatter.register_fake
def _(lens, lens_meta, final_thickness, lens_key, bsdf, rays_in, seed, plan_meta):
    return rays_in.new_empty(rays_in.shape, dtype=torch.float64)


@torch.library.custom_op("ort::bsdf_scatter", mutates_args=(), device_types="cuda")
def bsdf_scatter(dirs: torch.Tensor, normals: torch.Tensor, kind: int, sigma: float, seed: int,
                 plan_meta: list[int]) -> torch.Tensor:
    """BaseBSDF.scatter on tensors (ort_bsdf_scatter): dirs [3, n] (L M N) and normals
    [3, n] -> the scattered directions [3, n]. kind: _abi.BSDF_LAMBERTIAN / BSDF_GAUSSIAN;
    plan_meta = [surface_index, ray_offset, max_attempts]. Forward only."""
    from . import scatter as sc

    f = sc.LambertianBSDF() if kind == _abi.BSDF_LAMBERTIAN else sc.GaussianBSDF(sigma)
    if kind not in (_abi.BSDF_LAMBERTIAN, _abi.BSDF_GAUSSIAN):
        raise ValueError("bsdf_scatter: kind must be BSDF_LAMBERTIAN or BSDF_GAUSSIAN")
    surface_index, ray_offset, cap = plan_meta[:3]
    d, nrm = dirs.detach(), normals.detach()
    outs = sc.bsdf_scatter(d[0], d[1], d[2], nrm[0], nrm[1], nrm[2], f,
                           seed=int(seed) & 0xFFFFFFFFFFFFFFFF, surface_index=surface_index,
                           ray_offset=ray_offset, max_attempts=cap)
    return torch.stack(outs)


@bsdf_scatter.register_kernel("cpu")
def _bsdf_scatter_cpu(dirs, normals, kind, sigma, seed, plan_meta):
    """The CPU dispatch key: the host build (ort_host_bsdf_scatter)."""
    return bsdf_scatter._init_fn(dirs, normals, kind, sigma, seed, plan_meta)


@bsdf_scatter.register_fake
def _(dirs, normals, kind, sigma, seed, plan_meta):
    return dirs.new_empty(dirs.shape, dtype=torch.float64)


def _scatter_backward(ctx, *grads):
    raise RuntimeError("the ort::*_scatter ops are forward only: a trace through BSDF "
                       "surfaces has no derivative")


trace_pupil_scatter.register_autograd(_scatter_backward)
trace_sequential_scatter.register_autograd(_scatter_backward)
bsdf_scatter.register_autograd(_scatter_backward)


# --------------------------------------------------------------------------------------
# ort::trace_ensemble -- V variants of one lens in one launch (ort_trace_ensemble,
# tolerancing.py): the stacked tables in, the per-(variant, pair) rms rows and, on request,
# the rays out. Device only: the host build traces one lens per call.
# --------------------------------------------------------------------------------------
ENSEMBLE_META = ("n_surfaces", "n_lambda", "n_mat", "final_mat", "geometry_mask",
                 "interaction_mask", "frame_flags", "form_flags", "n_variants", "pairs",
                 "cs_stride")


@torch.library.custom_op("ort::trace_ensemble", mutates_args=(), device_types="cuda")
def trace_ensemble(lens: list[torch.Tensor], lens_meta: list[int], final_thickness: torch.Tensor,
                   seg: torch.Tensor, apod: torch.Tensor | None, px: torch.Tensor,
                   py: torch.Tensor, want_rays: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """lens: the nine tables of tolerancing.EnsembleTable.tensors (surfaces [V][S], cs_ops
    [V][cs_stride], coef, zern, n_tab and alpha_tab [V][n_lambda][n_mat], optics
    [V][n_lambda][S], materials, wavelengths); lens_meta: ENSEMBLE_META; final_thickness [V];
    seg: [V][P] SEGMENT records as bytes; px, py: the shared pupil points. Returns stats
    [V, P, 4] (count, mean x, mean y, rms: the C row without its constant NaN column) and the
    rays [8, V * P * n_pupil] (x y z L M N i opd; [8, 0] without want_rays). Forward only."""
    from . import tolerancing

    if len(lens_meta) != len(ENSEMBLE_META) or len(lens) != 9:
        raise ValueError("trace_ensemble: lens holds nine tables, lens_meta ENSEMBLE_META")
    V, P = lens_meta[8], lens_meta[9]
    if seg.numel() != V * P * _abi.SEGMENT.itemsize or final_thickness.numel() != V:
        raise ValueError("trace_ensemble: seg holds [V][P] segments, final_thickness [V]")
    stats, rays, status = tolerancing.trace_ensemble(
        [t.detach().contiguous() for t in lens], [int(v) for v in lens_meta],
        final_thickness.detach().to(torch.float64).contiguous(), seg.contiguous(),
        apod, px.detach().contiguous(), py.detach().contiguous(), bool(want_rays))
    if apod is not None:  # only an apodization record can raise a status bit here
        _calls.raise_status(int(status.item()))
    if rays is None:
        rays = px.new_empty((8, 0), dtype=torch.float64)
    return stats[..., :4].contiguous(), rays


@trace_ensemble.register_fake
def _(lens, lens_meta, final_thickness, seg, apod, px, py, want_rays):
    V, P = lens_meta[8], lens_meta[9]
    n = V * P * px.numel() if want_rays else 0
    return (px.new_empty((V, P, 4), dtype=torch.float64),
            px.new_empty((8, n), dtype=torch.float64))


def _ensemble_backward(ctx, *grads):
    raise RuntimeError("ort::trace_ensemble is forward only: autograd through the lens-ensemble "
                       "trace is not implemented")


trace_ensemble.register_autograd(_ensemble_backward)
