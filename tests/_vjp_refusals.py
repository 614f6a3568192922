"""The argument-refusal table of the VJP entry points, shared by the host library's test
(tests/test_host_vjp_refusals.py: ort_host_trace_sequential_vjp / ort_host_trace_pupil_vjp)
and the device library's (tests/test_gpu_vjp_refusals.py: ort_trace_sequential_vjp /
ort_trace_pupil_vjp). The expected return codes are read off the two libraries' sources
(csrc/ort_host.cpp, csrc/ort_api.hip): every refusal is ORT_ERR_ARG, returned before
anything is traced (the gradient buffer keeps its bytes).

A call is built in backend-neutral form -- a Call holds the ctypes structs and the arrays
they point to, allocated through `alloc(np_array) -> (keepalive, address)` (numpy memory on
the host, a device tensor on the GPU) -- a row of the table mutates it, and the test hands
it to its library.
"""

import ctypes as C

import numpy as np

from optiland_pr_amd import _abi, _native
from optiland_pr_amd.ops import mono_slot_count

OK, ERR_ARG = 0, -1  # include/optiland_rt.h: ORT_OK, ORT_ERR_ARG
N_RAYS = 64
SENTINEL = 7.0  # the gradient buffer's fill before every call

# the golden lenses the table needs (each lowered once per test module)
LENSES = {
    "tma_fringe": "the Newton (Zernike) lens of the base call",
    "cooke": "closed-form: no Zernike surface",
    "paraxial_lens": "thin-lens interaction model",
    "grid_lens": "grid-sag surface",
}


def lowered(name):
    """(LensTable, segments [1]) of a golden lens at its primary wavelength, field (0, 1)."""
    from tests._cases import build_lens, native_case

    wl = build_lens(name).primary_wavelength
    _, table, segs = native_case(name, {"wavelengths": [wl], "fields": [(0.0, 1.0)]})
    return table, segs


class Call:
    """One VJP call: form "seq" (resident rays) or "pupil" (generated rays)."""

    def __init__(self, form, mode, lens_c, table, segs, alloc):
        self.form, self.mode, self.alloc, self.table = form, mode, alloc, table
        self.keep = []
        n, S = N_RAYS, table.n_surfaces
        self.lens = lens_c
        gen = np.random.default_rng(5)
        r = np.sqrt(gen.uniform(0.0, 1.0, n))
        th = gen.uniform(0.0, 2.0 * np.pi, n)
        self.px, self.py = self.dev(r * np.cos(th)), self.dev(r * np.sin(th))
        # resident rays: a collimated +z bundle of unit intensity from the plane z = 0
        zeros, ones = self.dev(np.zeros(n)), self.dev(np.ones(n))
        self.rays_in = _native.ort_rays(self.px, self.py, zeros, zeros, zeros, ones, ones, zeros)
        if form == "pupil":
            self.batch = _native.ort_batch(n, n, n, 1, 0, self.dev(segs))
        else:
            self.batch = _native.ort_batch(n, n, n, 0, 0, None)
        self.opt = _native.ort_options(_abi.NEWTON_SCHEDULE, 0, None)
        # two parameters: the first Zernike term of the lens (when it has a Zernike surface:
        # the lowered table of a lens without one still holds a dummy term row, and a
        # zern_param on such a lens is a refusal of its own, zern_param_without_zernike) and
        # the radius of surface 1
        self.n_param = 2
        zp = None
        if np.any(table.surfaces["geometry"] == _abi.GEOM_ZERNIKE):
            zp = np.full(len(table.zern), -1, np.int32)
            zp[0] = 0
        st = np.zeros((self.n_param, S, 3))
        st[1, 1, 0] = 1.0
        self.params = _native.ort_vjp_params(
            self.n_param, int(mode), None if zp is None else self.dev(zp), self.dev(st), None,
            0 if zp is None else len(zp), 0, None, 0, None)
        if mode == _abi.VJP_ADJOINT:
            self.params.n_mono = mono_slot_count(table, zp)
        cot = gen.standard_normal((8, n))
        self.cot = _native.ort_rays(*(self.dev(c) for c in cot))
        self.grad_keep, self.grad = alloc(np.full(self.n_param, SENTINEL))
        self.rec_cot = self.rec = None
        self.gin = None
        # NULL-able struct arguments
        self.null = set()

    def dev(self, arr):
        keep, addr = self.alloc(np.ascontiguousarray(arr))
        self.keep.append(keep)
        return addr

    def ref(self, name):
        return None if name in self.null else C.byref(getattr(self, name))


# ---- the rows: (id, lens, forms, modes, mutate, device) -> ORT_ERR_ARG -------------------
# device: None -- the device library refuses the same calls; False -- it accepts them (a
# host-only refusal); a tuple -- the modes in which it refuses them
A, U = _abi.VJP_ADJOINT, _abi.VJP_UNROLLED
BOTH, SEQ, PUPIL = ("seq", "pupil"), ("seq",), ("pupil",)


def _null(name):
    return lambda c: c.null.add(name)


def _set(obj, field, value):
    return lambda c: setattr(getattr(c, obj), field, value(c) if callable(value) else value)


def _some(c):
    return c.dev(np.ones(8))


def _zern_param_on_closed(c):
    c.params.zern_param = c.dev(np.zeros(1, np.int32))
    c.params.n_zern = 1


def _rec_cot_without_rec(c):
    c.rec_cot = c.dev(np.zeros(8 * N_RAYS))


def _grad_null(c):
    c.grad = None


def _n_mono_without_zern(c):
    c.params.zern_param = None
    c.params.n_zern = 0
    c.params.n_mono = 6


def _rms_both(c):
    c.params.rms_stats = c.dev(np.ones(5))
    c.params.rms_grad = c.dev(np.ones(1))


def _grad_in(c):
    c.gin = _native.ort_rays(*([c.dev(np.zeros(N_RAYS))] + [None] * 7))


REFUSED = [
    ("null_batch", "tma_fringe", BOTH, (A, U), _null("batch"), None),
    ("null_cotangent", "tma_fringe", BOTH, (A, U), _null("cot"), None),
    ("null_params", "tma_fringe", BOTH, (A, U), _null("params"), None),
    ("null_opt", "tma_fringe", BOTH, (A, U), _null("opt"), None),
    ("negative_n_param", "tma_fringe", BOTH, (A, U), _set("params", "n_param", -1), None),
    ("grad_null", "tma_fringe", BOTH, (A, U), _grad_null, None),
    ("rec_cotangent_without_rec", "tma_fringe", SEQ, (A, U), _rec_cot_without_rec, None),
    ("zern_param_without_zernike", "cooke", BOTH, (A, U), _zern_param_on_closed, None),
    ("interaction_lens_adjoint", "paraxial_lens", BOTH, (A,), lambda c: None, None),
    ("grid_sag_lens", "grid_lens", BOTH, (A, U), lambda c: None, None),
    ("negative_n_mono", "tma_fringe", BOTH, (A,), _set("params", "n_mono", -1), None),
    ("n_mono_without_zern_param", "tma_fringe", BOTH, (A,), _n_mono_without_zern, None),
    ("rms_stats_without_rms_grad", "tma_fringe", BOTH, (A,),
     _set("params", "rms_stats", _some), None),
    ("rms_in_unrolled", "tma_fringe", BOTH, (U,), _rms_both, None),
    ("grad_in_in_unrolled", "tma_fringe", SEQ, (U,), _grad_in, None),
    ("unknown_mode", "tma_fringe", BOTH, (7,), lambda c: None, None),
    # the host library takes no tape; the device's adjoint refuses this one by its own check
    # (a tape needs generated rays and the primal's final state), its forward mode reads none
    ("params_tape", "tma_fringe", BOTH, (A, U), _set("params", "tape", _some), (A,)),
    # host only: the device library takes a tape in the options and a start surface
    ("opt_tape", "tma_fringe", BOTH, (A, U), _set("opt", "tape", _some), False),
    ("pupil_start_surface", "tma_fringe", PUPIL, (A, U), _set("opt", "start_surface", 1), False),
]


def rows(device):
    """(id, lens, form, mode, mutate) of every refused call of a library."""
    out = []
    for name, lens, forms, modes, mutate, dev in REFUSED:
        if device and dev is False:
            continue
        if device and dev is not None:
            modes = dev
        for form in forms:
            for mode in modes:
                out.append((f"{name}-{form}-mode{mode}", lens, form, mode, mutate))
    return out


# ---- accepted ---------------------------------------------------------------------------
# The unmutated base call, where the library must take it: (lens, mode). These pin that a
# row above is refused for its own reason and not because its base call already was
# (paraxial_lens: the forward mode differentiates interaction-model lenses).
BASE_ACCEPTED = [("tma_fringe", A), ("tma_fringe", U), ("cooke", A), ("cooke", U),
                 ("paraxial_lens", U)]


# accepted without tracing
def empty_batch_grad_init(c):
    c.batch.n_rays = 0
    c.params.grad_init = 1


def no_param_no_grad_in(c):
    c.params.n_param = 0
