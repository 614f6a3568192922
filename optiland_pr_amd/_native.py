"""ctypes bindings of the C ABIs: include/optiland_rt.h (liboptiland_rt.so, the HIP trace
core) and include/optiland_host.h (liboptiland_host.so, its host build: the CPU dispatch key
of the torch custom ops).

There is no fallback between them: a trace of device tensors needs liboptiland_rt.so and a
GPU, a trace of host tensors needs liboptiland_host.so; a missing library raises.
"""

from __future__ import annotations

import ctypes as C
import os

from . import _abi
from .build import HOST_LIB_PATH, LIB_PATH


class ort_lens(C.Structure):
    _fields_ = [
        ("surfaces", C.c_void_p),
        ("cs_ops", C.c_void_p),
        ("coef", C.c_void_p),
        ("zern", C.c_void_p),
        ("n_tab", C.c_void_p),
        ("alpha_tab", C.c_void_p),
        ("optics", C.c_void_p),
        ("n_surfaces", C.c_int32),
        ("n_lambda", C.c_int32),
        ("n_mat", C.c_int32),
        ("final_mat", C.c_int32),
        ("geometry_mask", C.c_uint32),
        ("interaction_mask", C.c_uint32),
        ("final_thickness", C.c_double),
        ("materials", C.c_void_p),
        ("wavelengths", C.c_void_p),
        ("frame_flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class ort_rays(C.Structure):
    _fields_ = [(a, C.c_void_p) for a in _abi.RAY_FIELDS]


class ort_batch(C.Structure):
    _fields_ = [
        ("n_rays", C.c_int64),
        ("seg_len", C.c_int64),
        ("group_len", C.c_int64),
        ("n_seg", C.c_int32),
        ("pupil_per_ray", C.c_int32),
        ("seg", C.c_void_p),
        ("w", C.c_void_p),
        ("apod", C.c_void_p),
    ]


class ort_vjp_params(C.Structure):  # field 7 ("grad_init") was "reserved" before v14
    _fields_ = [
        ("n_param", C.c_int32),
        ("mode", C.c_int32),
        ("zern_param", C.c_void_p),
        ("surf_tangent", C.c_void_p),
        ("final_tangent", C.c_void_p),
        ("n_zern", C.c_int32),
        ("grad_init", C.c_int32),
        ("workspace", C.c_void_p),
        ("workspace_size", C.c_int64),
        ("slot_need", C.c_void_p),
        ("tape", C.c_void_p),
        ("primal", ort_rays),
        ("n_mono", C.c_int32),  # v18
        ("reserved", C.c_int32),
        ("rms_stats", C.c_void_p),
        ("rms_grad", C.c_void_p),
    ]


ADAM_MAX_TENSORS = 16  # include/optiland_rt.h ORT_ADAM_MAX_TENSORS


class ort_adam_params(C.Structure):  # v19
    _fields_ = [
        ("n_tensors", C.c_int32),
        ("reserved", C.c_int32),
        ("param", C.c_void_p * ADAM_MAX_TENSORS),
        ("grad", C.c_void_p * ADAM_MAX_TENSORS),
        ("exp_avg", C.c_void_p * ADAM_MAX_TENSORS),
        ("exp_avg_sq", C.c_void_p * ADAM_MAX_TENSORS),
        ("row0", C.c_int64 * ADAM_MAX_TENSORS),
        ("count", C.c_int64 * ADAM_MAX_TENSORS),
        ("step", C.c_void_p * ADAM_MAX_TENSORS),
        ("lr", C.c_double),
        ("beta1", C.c_double),
        ("beta2", C.c_double),
        ("eps", C.c_double),
        ("weight_decay", C.c_double),
    ]


class ort_pupil(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("positive_only", C.c_int32),
        ("n", C.c_int64),
        ("n_points", C.c_int64),
        ("n_rows", C.c_int32),
        ("reserved", C.c_int32),
        ("row_start", C.c_void_p),
        ("row_col", C.c_void_p),
        ("rng_chunk", C.c_void_p),
        ("rng_lane", C.c_void_p),
    ]


class ort_options(C.Structure):
    _fields_ = [
        ("newton_mode", C.c_int32),
        ("start_surface", C.c_int32),
        ("sched", C.c_void_p),
        ("conv_base", C.c_int32),
        ("flags", C.c_int32),
        ("run_if", C.c_void_p),
        ("tape", C.c_void_p),
        ("verify_stats", C.c_void_p),
        ("verify_prev_flag", C.c_void_p),
        ("verify_flag", C.c_void_p),
        ("sched_out", C.c_void_p),
        ("rms_part", C.c_void_p),  # v18
    ]


class ort_polarization(C.Structure):  # added within v21 (ort_trace_*_polarized)
    _fields_ = [
        ("mode", C.c_int32),
        ("reserved", C.c_int32),
        ("ex_re", C.c_double),
        ("ex_im", C.c_double),
        ("ey_re", C.c_double),
        ("ey_im", C.c_double),
        ("coatings", C.c_void_p),
        ("p_out", C.c_void_p),
    ]


class ort_spot_layout(C.Structure):
    _fields_ = [
        ("n_pupil", C.c_int64),
        ("n_fields", C.c_int32),
        ("n_wl", C.c_int32),
        ("ref_wl", C.c_int32),
        ("n_local_ops", C.c_int32),
        ("local_ops", C.c_void_p),
    ]


class ort_wavefront_ref(C.Structure):
    _fields_ = [(f, C.c_double) for f in ("xc", "yc", "zc", "xc2", "yc2", "zc2", "r2",
                                          "n_image", "opd_ref", "ux", "uy", "epd", "wl_mm")]
    _fields_ += [("tilt", C.c_int32), ("reserved", C.c_int32)]


EXPORTS = ("ort_abi_version", "ort_trace_sequential", "ort_trace_pupil", "ort_trace_pupil_vjp",
           "ort_trace_sequential_vjp",
           "ort_vjp_workspace_size", "ort_vjp_tape_size", "ort_generate_pupil", "ort_newton_fixup",
           "ort_surface_sag_normal", "ort_surface_distance", "ort_generate_rays",
           "ort_material_nk", "ort_spot_workspace_size", "ort_spot_stats", "ort_trace_spot", "ort_spot_partials",
           "ort_rms_spot_workspace_size", "ort_rms_spot", "ort_rms_spot_vjp",
           "ort_wavefront_workspace_size", "ort_wavefront_opd", "ort_patch_zernike",
           "ort_patch_zernike_ptrs", "ort_newton_finish", "ort_adam_patch_zernike",
           "ort_rms_finish", "ort_newton_finish_rms", "ort_huygens_workspace_size",
           "ort_huygens_psf", "ort_irradiance_workspace_size", "ort_irradiance_bin",
           "ort_irradiance_bin_vjp", "ort_trace_pupil_polarized",
           "ort_trace_sequential_polarized")

_lib = None


class NativeLibraryError(RuntimeError):
    pass


def load(path: str | None = None):
    """Load liboptiland_rt.so (raises NativeLibraryError when it is not built)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # ORT_LIB_PATH: load an alternative build (A/B timing of kernel variants)
    p = path or os.environ.get("ORT_LIB_PATH") or LIB_PATH
    if not os.path.exists(p):
        raise NativeLibraryError(
            f"{p} is missing: build the HIP extension first "
            "(python -m optiland_pr_amd.build or __graft_entry__.build())")
    lib = C.CDLL(p)
    lib.ort_abi_version.restype = C.c_int
    lib.ort_abi_version.argtypes = []
    P = C.POINTER
    lib.ort_trace_sequential.restype = C.c_int
    lib.ort_trace_sequential.argtypes = [P(ort_lens), P(ort_rays), P(ort_rays), P(ort_batch),
                                         P(ort_options), C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    lib.ort_trace_pupil.restype = C.c_int
    lib.ort_trace_pupil.argtypes = [P(ort_lens), C.c_void_p, C.c_void_p, P(ort_rays),
                                    P(ort_batch), P(ort_options), C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
    lib.ort_trace_pupil_vjp.restype = C.c_int
    lib.ort_trace_pupil_vjp.argtypes = [P(ort_lens), C.c_void_p, C.c_void_p, P(ort_batch),
                                        P(ort_options), P(ort_vjp_params), P(ort_rays),
                                        C.c_void_p, C.c_void_p]
    lib.ort_trace_sequential_vjp.restype = C.c_int
    lib.ort_trace_sequential_vjp.argtypes = [P(ort_lens), P(ort_rays), P(ort_batch),
                                             P(ort_options), P(ort_vjp_params), P(ort_rays),
                                             C.c_void_p, C.c_void_p, C.c_void_p, P(ort_rays),
                                             C.c_void_p]
    lib.ort_vjp_tape_size.restype = C.c_int64
    lib.ort_vjp_tape_size.argtypes = [P(ort_lens), P(ort_batch)]
    lib.ort_vjp_workspace_size.restype = C.c_int64
    lib.ort_vjp_workspace_size.argtypes = [P(ort_lens), P(ort_batch), P(ort_vjp_params)]
    lib.ort_patch_zernike.restype = C.c_int
    lib.ort_patch_zernike.argtypes = [P(ort_lens), C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_void_p]
    lib.ort_rms_finish.restype = C.c_int
    lib.ort_rms_finish.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ort_adam_patch_zernike.restype = C.c_int
    lib.ort_adam_patch_zernike.argtypes = [P(ort_lens), P(ort_adam_params), C.c_void_p]
    lib.ort_patch_zernike_ptrs.restype = C.c_int
    lib.ort_patch_zernike_ptrs.argtypes = [P(ort_lens), C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_void_p]
    lib.ort_newton_finish.restype = C.c_int
    lib.ort_newton_finish.argtypes = [P(ort_lens), C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]
    lib.ort_newton_finish_rms.restype = C.c_int
    lib.ort_newton_finish_rms.argtypes = [P(ort_lens), C.c_int64, C.c_void_p, C.c_int32,
                                          C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ort_surface_sag_normal.restype = C.c_int
    lib.ort_surface_sag_normal.argtypes = [P(ort_lens), C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ort_surface_distance.restype = C.c_int
    lib.ort_surface_distance.argtypes = [P(ort_lens), C.c_int32, P(ort_rays), C.c_int64,
                                         P(ort_options), C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    lib.ort_newton_fixup.restype = C.c_int
    lib.ort_newton_fixup.argtypes = [P(ort_lens), C.c_int64, C.c_void_p, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]
    lib.ort_generate_pupil.restype = C.c_int
    lib.ort_generate_pupil.argtypes = [P(ort_pupil), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ort_material_nk.restype = C.c_int
    lib.ort_material_nk.argtypes = [P(ort_lens), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
    lib.ort_generate_rays.restype = C.c_int
    lib.ort_generate_rays.argtypes = [C.c_void_p, C.c_void_p, P(ort_rays), P(ort_batch),
                                      C.c_void_p]
    lib.ort_spot_workspace_size.restype = C.c_int64
    lib.ort_spot_workspace_size.argtypes = [P(ort_spot_layout)]
    lib.ort_spot_stats.restype = C.c_int
    lib.ort_spot_stats.argtypes = [P(ort_rays), P(ort_spot_layout), C.c_void_p, C.c_int64,
                                   C.c_void_p, C.c_void_p]
    lib.ort_trace_spot.restype = C.c_int
    lib.ort_trace_spot.argtypes = [P(ort_lens), C.c_void_p, C.c_void_p, P(ort_rays),
                                   P(ort_batch), P(ort_options), C.c_void_p,
                                   P(ort_spot_layout), C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_void_p]
    lib.ort_spot_partials.restype = C.c_int
    lib.ort_spot_partials.argtypes = [P(ort_rays), P(ort_spot_layout), C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.ort_rms_spot_workspace_size.restype = C.c_int64
    lib.ort_rms_spot_workspace_size.argtypes = [C.c_int64]
    lib.ort_rms_spot.restype = C.c_int
    lib.ort_rms_spot.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                 C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ort_rms_spot_vjp.restype = C.c_int
    lib.ort_rms_spot_vjp.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ort_wavefront_workspace_size.restype = C.c_int64
    lib.ort_wavefront_workspace_size.argtypes = [C.c_int64]
    lib.ort_wavefront_opd.restype = C.c_int
    lib.ort_wavefront_opd.argtypes = [P(ort_rays), C.c_void_p, C.c_void_p, C.c_int64,
                                      P(ort_wavefront_ref), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_void_p]
    lib.ort_huygens_workspace_size.restype = C.c_int64
    lib.ort_huygens_workspace_size.argtypes = [C.c_int64, C.c_int64]
    lib.ort_huygens_psf.restype = C.c_int
    lib.ort_huygens_psf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.c_void_p]
    lib.ort_irradiance_workspace_size.restype = C.c_int64
    lib.ort_irradiance_workspace_size.argtypes = [C.c_int64, C.c_int64]
    lib.ort_irradiance_bin.restype = C.c_int
    lib.ort_irradiance_bin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                       C.c_double, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.c_void_p]
    lib.ort_irradiance_bin_vjp.restype = C.c_int
    lib.ort_irradiance_bin_vjp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                           C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
    lib.ort_trace_pupil_polarized.restype = C.c_int
    lib.ort_trace_pupil_polarized.argtypes = [P(ort_lens), C.c_void_p, C.c_void_p, P(ort_rays),
                                              P(ort_batch), P(ort_options), C.c_void_p,
                                              C.c_void_p, C.c_void_p, P(ort_polarization),
                                              C.c_void_p]
    lib.ort_trace_sequential_polarized.restype = C.c_int
    lib.ort_trace_sequential_polarized.argtypes = [P(ort_lens), P(ort_rays), P(ort_rays),
                                                   P(ort_batch), P(ort_options), C.c_void_p,
                                                   C.c_void_p, C.c_void_p, P(ort_polarization),
                                                   C.c_void_p]
    v = lib.ort_abi_version()
    if v != _abi.ABI_VERSION:
        raise NativeLibraryError(f"ABI version mismatch: library {v}, host {_abi.ABI_VERSION}")
    if path is None:
        _lib = lib
    return lib


HOST_EXPORTS = ("ort_host_abi_version", "ort_host_trace_sequential",
                "ort_host_trace_sequential_vjp", "ort_host_trace_pupil", "ort_host_trace_pupil_vjp",
                "ort_host_rms_spot", "ort_host_rms_spot_vjp", "ort_host_set_threads",
                "ort_host_huygens_psf", "ort_host_irradiance_bin",
                "ort_host_irradiance_bin_vjp", "ort_host_trace_pupil_polarized",
                "ort_host_trace_sequential_polarized", "ort_host_generate_rays")
HOST_ABI_VERSION = 3  # include/optiland_host.h ORT_HOST_ABI_VERSION

_host = None


def load_host(path: str | None = None):
    """Load liboptiland_host.so (raises NativeLibraryError when it is not built)."""
    global _host
    if _host is not None and path is None:
        return _host
    p = path or os.environ.get("ORT_HOST_LIB_PATH") or HOST_LIB_PATH
    if not os.path.exists(p):
        raise NativeLibraryError(
            f"{p} is missing: build the native libraries first "
            "(python -m optiland_pr_amd.build or __graft_entry__.build())")
    lib = C.CDLL(p)
    P = C.POINTER
    lib.ort_host_abi_version.restype = C.c_int
    lib.ort_host_abi_version.argtypes = []
    lib.ort_host_trace_sequential.restype = C.c_int
    lib.ort_host_trace_sequential.argtypes = [P(ort_lens), P(ort_rays), P(ort_rays),
                                              P(ort_batch), P(ort_options), C.c_void_p,
                                              C.c_void_p, C.c_void_p]
    lib.ort_host_trace_sequential_vjp.restype = C.c_int
    lib.ort_host_trace_sequential_vjp.argtypes = [P(ort_lens), P(ort_rays), P(ort_batch),
                                                  P(ort_options), P(ort_vjp_params),
                                                  P(ort_rays), C.c_void_p, C.c_void_p,
                                                  C.c_void_p, P(ort_rays)]
    lib.ort_host_trace_pupil.restype = C.c_int
    lib.ort_host_trace_pupil.argtypes = [P(ort_lens), C.c_void_p, C.c_void_p, P(ort_rays),
                                         P(ort_batch), P(ort_options), C.c_void_p, C.c_void_p]
    lib.ort_host_trace_pupil_vjp.restype = C.c_int
    lib.ort_host_trace_pupil_vjp.argtypes = [P(ort_lens), C.c_void_p, C.c_void_p, P(ort_batch),
                                             P(ort_options), P(ort_vjp_params), P(ort_rays),
                                             C.c_void_p]
    lib.ort_host_rms_spot.restype = C.c_int
    lib.ort_host_rms_spot.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.ort_host_rms_spot_vjp.restype = C.c_int
    lib.ort_host_rms_spot_vjp.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ort_host_set_threads.restype = None
    lib.ort_host_set_threads.argtypes = [C.c_int32]
    lib.ort_host_huygens_psf.restype = C.c_int
    lib.ort_host_huygens_psf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int64, C.c_double, C.c_double,
                                         C.c_void_p]
    lib.ort_host_irradiance_bin.restype = C.c_int
    lib.ort_host_irradiance_bin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                            C.c_int32, C.c_double, C.c_void_p]
    lib.ort_host_irradiance_bin_vjp.restype = C.c_int
    lib.ort_host_irradiance_bin_vjp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p]
    lib.ort_host_trace_pupil_polarized.restype = C.c_int
    lib.ort_host_trace_pupil_polarized.argtypes = [P(ort_lens), C.c_void_p, C.c_void_p,
                                                   P(ort_rays), P(ort_batch), P(ort_options),
                                                   C.c_void_p, C.c_void_p, C.c_void_p,
                                                   P(ort_polarization)]
    lib.ort_host_trace_sequential_polarized.restype = C.c_int
    lib.ort_host_trace_sequential_polarized.argtypes = [P(ort_lens), P(ort_rays), P(ort_rays),
                                                        P(ort_batch), P(ort_options), C.c_void_p,
                                                        C.c_void_p, C.c_void_p,
                                                        P(ort_polarization)]
    lib.ort_host_generate_rays.restype = C.c_int
    lib.ort_host_generate_rays.argtypes = [C.c_void_p, C.c_void_p, P(ort_rays), P(ort_batch)]
    v = lib.ort_host_abi_version()
    if v != HOST_ABI_VERSION:
        raise NativeLibraryError(f"host ABI version mismatch: library {v}, host {HOST_ABI_VERSION}")
    if path is None:
        _host = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        names = {-1: "ORT_ERR_ARG", -2: "ORT_ERR_SURFACES", -3: "ORT_ERR_LAUNCH"}
        raise RuntimeError(f"{what} failed: {names.get(rc, rc)}")
