"""Shared by tests/test_vjp_sums_cpu.py and tests/test_gpu_vjp_sums.py: the ray sums of the
gradient kernels (ort_trace_pupil_vjp / ort_trace_sequential_vjp, both modes; adj_kernel's
emit / mono_put / mono_chunk / group8_sum and block epilogue, adj_slot_reduce_kernel,
adj_grad_kernel, vjp_kernel / vjp_reduce_kernel<P> (their block sums: ort_reduce.h
block_sum_lead / block_sum_at); on the host adj_chunks / vjp_chunks)
against an exact sum, at the lane, wave, block and partial-column edges. The maths of the
per-ray sweep (ort_sweep.h) is pinned elsewhere (adjoint against unrolled, the reference's
autograd goldens, the oracle's finite differences); here only the summation is.

Method. J^T c is linear in the cotangent c and a sum of per-ray terms: for a fixed lens,
fixed Newton schedule and fixed tangent tables ray r adds t_r[p] to parameter p, and t_r
depends only on the ray's own pupil point and cotangent row.
  1. t_r comes from launches of ONE ray (n = 1: lane 0 is the only active lane, one block, one
     partial column -- nothing is left of the reduction), for the R = 257 rays of a seeded
     base set, on the device and on the host.
  2. Scaling a ray's cotangents by +-2^e scales every operation of its sweep, hence its term,
     exactly. A large batch is copies of the base set (pupil_per_ray, the pupil points and
     cotangent rows repeated), copy c scaled by s_c = +-2^e, e in [-6, 6], seeded (s_0 = 1:
     the sizes up to 257 are plain prefixes).
  3. The exact gradient of the batch is sum_c s_c sum_r t_r[p], every product exact, summed
     in fractions.Fraction. It never sees the kernels' partition into waves, blocks, slots.

Bound. |grad[p] - exact[p]| <= T A[p], A[p] = sum_c sum_r |s_c t_r[p]| (the absolute mass:
cancelling sums do not turn correct arithmetic into a failure). T is not derived: a slot
may take several partly cancelling emits per ray, which the batch sums emit by emit and the
n = 1 launch per ray, and a Zernike coefficient is a fixed linear map of monomial slot sums
(integer weights up to a few hundred, ort_args.h mono_weight) -- neither visible from
outside. HOST_DEV is the host build's largest |grad - exact| / A over every row and size
below against its own n = 1 terms, measure(); T = 16 HOST_DEV (one order for the device's
different tree), under the cap 1e-12: the longest chain any term passes through is under a
hundred additions of 1.1e-16 on the device, so more than 1e-12 of the absolute mass is a lost
or doubled term, not rounding. The cap is a condition, asserted at import.

Parameters. "slots": one parameter per slot -- radius, conic and vertex z of every traced
surface (surf_tangent one-hot), every Zernike term (zern_param), the image-space thickness
(final_tangent one-hot) -- so grad[p] is one slot's ray sum (or the term matrices' map of the
monomial slot sums), followed by the lens's ordinary parameters as tests/test_gpu_adjoint.py
names them (ops.tangent_tables: a thickness in the middle of the lens fans out over the
later vertices -- adj_grad_kernel's contraction). A surf_tangent table selects the P = 4
kernels (ort_api.hip vjp_run). "zern": the Zernike terms and the final thickness only, no
surf_tangent: the P = 2 kernels (adj2 / adj2r at 3 waves per SIMD).
"""

import contextlib
import functools
import os
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

from optiland_pr_amd import _abi

# measured: 1.28e-15, the tma_fringe rows at n = 2 (the term matrices' map of two rays'
# monomial sums); every other row and size stays below 2.9e-16:
#   python -c "from tests import _vjp_sums as V; print(V.measure())"
# (the MI355X's own largest value, measure("device"), is 1.05e-15 at the same place, 1.8e-16
# elsewhere: inside HOST_DEV itself)
HOST_DEV = 1.3e-15
CAP = 1e-12

R = 257                                   # the base set
SMALL = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257)  # prefixes of the base set
MID = (65536, 65537)                      # 256 | 257 partial columns: the strided loop's 2nd pass
LARGE = (458752, 458753, 524289)          # 1792 | 1793: the unrolled body's first run; 2049: + tail
MAX_COPIES = -(-LARGE[-1] // R) + 1
FIELDS = _abi.RAY_FIELDS
ADJ, UNR = _abi.VJP_ADJOINT, _abi.VJP_UNROLLED

# row -> lens, parameter set, mode, entry point, ORT_VJP_TANGENTS (unrolled), largest sizes
ROWS = {
    "cooke": dict(lens="cooke", pset="slots", mode=ADJ, large=True),           # adj4, KM = 0
    "rt_asph": dict(lens="rt_asph", pset="slots", mode=ADJ),                   # adj4, Newton
    "tma_fringe": dict(lens="tma_fringe", pset="zern", mode=ADJ, large=True),  # adj2, monomials
    "tma_fringe_slots": dict(lens="tma_fringe", pset="slots", mode=ADJ),       # adj4, monomials
    "tma_fringe25": dict(lens="tma_fringe25", pset="zern", mode=ADJ),          # adj2, per-term emit
    "tma_standard_t1": dict(lens="tma_standard", pset="slots", mode=UNR, tangents=1),
    "tma_standard_t2": dict(lens="tma_standard", pset="slots", mode=UNR, tangents=2),
    "tma_standard_t4": dict(lens="tma_standard", pset="slots", mode=UNR, tangents=4, large=True),
    "cooke_resident": dict(lens="cooke", pset="slots", mode=ADJ, resident=True),       # adj4r
    "tma_fringe_resident": dict(lens="tma_fringe", pset="zern", mode=ADJ, resident=True),  # adj2r
    # clipped rays. The lens's apertures clip 0.9% of the disc of radius 1.0 at this field
    # (r_max = 4.5 lies outside the beam; the central obscuration r_min = 0.4 of surface 5
    # shadows the pupil patch around (0, -0.667), radius 0.094; 200,000 points on the host),
    # so no seed brings 257 uniform points to the 5% the test requires of its input: 48 of
    # the 257 points, chosen by the seed, are moved into the disc of radius 0.13 around that
    # patch, uniform in it, the others stay uniform in the disc of radius 1.0.
    "cooke_aperture": dict(lens="cooke_aperture", pset="slots", mode=ADJ, radius=1.0,
                           patch=(0.0, -0.667, 0.13), patch_rays=48, sizes=(R,)),
}
HOST_ROWS = tuple(r for r in ROWS if r not in ("tma_standard_t1", "tma_standard_t2"))  # the host
# build has one forward-mode chunk width (4)
CLIP_SEED = 5  # cooke_aperture's base set: 5% to 60% of its rays clipped (asserted)


def sizes_of(row):
    spec = ROWS[row]
    if "sizes" in spec:
        return spec["sizes"]
    return SMALL + MID + (LARGE if spec.get("large") else ())


# -- the lenses ------------------------------------------------------------------------
@contextlib.contextmanager
def _zm_max_deg(deg):
    import optiland_pr_amd.geometries as geometries

    old = geometries.ZM_MAX_DEG
    geometries.ZM_MAX_DEG = deg
    try:
        yield
    finally:
        geometries.ZM_MAX_DEG = old


@functools.lru_cache(maxsize=None)
def lowered(name):
    """(LensTable, segments [1]) of the lens at field (0, 1), primary wavelength.
    tma_fringe25: 25 fringe coefficients per mirror lowered with a Cartesian block above
    degree 6, which takes the per-term slots (tests/test_cpu_vjp.py
    test_block_above_degree_six_takes_per_term_slots)."""
    from optiland_pr_amd import ops, samples
    from optiland_pr_amd.lowering import lower_apodization, lower_surface_group, segment_params
    from tests._cases import build_lens

    if name == "tma_fringe25":
        coeffs = tuple(1e-5 * ((-1) ** k) / (1 + k) for k in range(25))
        lens = samples.ThreeMirrorAnastigmat("fringe", coeffs)
        with _zm_max_deg(10):
            table = lower_surface_group(lens.surface_group, [lens.primary_wavelength])
        deg = table.surfaces["zm_deg"][table.surfaces["geometry"] == _abi.GEOM_ZERNIKE]
        assert np.all(deg > 6) and ops.mono_slot_count(table, np.zeros(1, np.int32)) == 0
    else:
        lens = build_lens(name)
        table = lower_surface_group(lens.surface_group, [lens.primary_wavelength])
    table.apod = lower_apodization(lens)
    assert table.apod is None
    return table, np.stack([segment_params(lens, 0.0, 1.0, 0)])


class _Scalar:
    @staticmethod
    def numel():
        return 1


@functools.lru_cache(maxsize=None)
def tables(row):
    """SimpleNamespace(zp, st, ft, need, n_param, n_slots): the tangent tables of the row's
    parameter set as host arrays (None: no such table) and ops.slot_need of them; parameters
    [0, n_slots) are one slot each."""
    from optiland_pr_amd import ops
    from tests.test_gpu_adjoint import CASES

    spec = ROWS[row]
    table, _ = lowered(spec["lens"])
    S, nz = table.n_surfaces, len(table.zern)
    zern = bool(np.any(table.surfaces["geometry"] == _abi.GEOM_ZERNIKE))
    zp = st = None
    off = 0
    if spec["pset"] == "slots":
        off = 3 * S
    if zern:
        zp = np.arange(off, off + nz, dtype=np.int32)
        off += nz
    n_slots = off + 1  # + the final thickness
    extra = []
    if spec["pset"] == "slots":
        base = "tma_fringe" if spec["lens"] == "tma_fringe25" else spec["lens"]
        # (CASES counts the object surface; the tables count traced surfaces)
        extra = [(k, si - 1) for k, si in next(c[1] for c in CASES if c[0] == base)
                 if k != "zernike"]
        assert any(k == "thickness" and si < S - 2 for k, si in extra), extra
        if spec["mode"] == UNR:  # a ragged last chunk at every chunk width: 4 .. 4, 2, 1
            while (n_slots + len(extra)) % 4 != 3:
                extra.append(("vertex", len(extra) % S))
    n_param = n_slots + len(extra)
    ft = np.zeros(n_param)
    ft[n_slots - 1] = 1.0
    if spec["pset"] == "slots":
        st = np.zeros((n_param, S, 3))
        st[np.arange(3 * S), np.arange(3 * S) // 3, np.arange(3 * S) % 3] = 1.0
        _, ex, _, _ = ops.tangent_tables(table, extra, [_Scalar] * len(extra))
        st[n_slots:] = ex
    need = ops.slot_need(table, zp, st, ft) if spec["mode"] == ADJ else None
    return SimpleNamespace(zp=zp, st=st, ft=ft, need=need, n_param=n_param, n_slots=n_slots)


# -- inputs ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base(row):
    """The base set: R seeded pupil points uniform in the disc of radius 0.9 (every ray
    reaches the image), standard-normal cotangents on all eight outputs."""
    radius = ROWS[row].get("radius", 0.9)
    gen = np.random.default_rng(CLIP_SEED if "radius" in ROWS[row] else 20240)
    rho = radius * np.sqrt(gen.random(R))
    phi = 2.0 * np.pi * gen.random(R)
    cot = gen.standard_normal((8, R))
    px, py = rho * np.cos(phi), rho * np.sin(phi)
    if "patch" in ROWS[row]:
        (cx, cy, pr), k = ROWS[row]["patch"], ROWS[row]["patch_rays"]
        at = gen.choice(R, k, replace=False)
        px[at] = cx + pr * rho[at] / radius * np.cos(phi[at])
        py[at] = cy + pr * rho[at] / radius * np.sin(phi[at])
    return SimpleNamespace(px=px, py=py, cot=cot)


@functools.lru_cache(maxsize=None)
def scales():
    gen = np.random.default_rng(77)
    s = np.ldexp(gen.choice([-1.0, 1.0], MAX_COPIES), gen.integers(-6, 7, MAX_COPIES))
    s[0] = 1.0
    return s


def batch(row, n):
    """(base ray [n], cot [8][n], scale [n]) of the n-ray batch: copies of the base set, copy
    c scaled by s_c."""
    idx = np.arange(n) % R
    s = scales()[np.arange(n) // R]
    return idx, np.ascontiguousarray(base(row).cot[:, idx] * s), s


# -- the exact reference -------------------------------------------------------------------
def _fr(a):
    out = np.empty(a.shape, dtype=object)
    out.ravel()[:] = [Fraction(float(v)) for v in a.ravel()]
    return out


class Exact:
    """Exact sums of per-ray terms [R][n_param] over batches of any size."""

    def __init__(self, terms):
        assert terms.shape[0] == R and np.all(np.isfinite(terms))
        t = _fr(terms)
        zero = np.full((1, terms.shape[1]), Fraction(0), dtype=object)
        self.pre = np.concatenate([zero, np.cumsum(t, axis=0)])         # prefix sums
        self.pre_abs = np.concatenate([zero, np.cumsum(abs(t), axis=0)])
        s = [Fraction(float(v)) for v in scales()]
        self.s = s
        self.cs = np.concatenate([[Fraction(0)], np.cumsum(np.array(s, dtype=object))])
        self.cs_abs = np.concatenate([[Fraction(0)],
                                      np.cumsum(np.array([abs(v) for v in s], dtype=object))])

    def sum(self, n):
        """(exact [n_param], A [n_param]) of the n-ray batch, as Fractions"""
        q, rem = divmod(n, R)
        return (self.cs[q] * self.pre[R] + self.s[q] * self.pre[rem],
                self.cs_abs[q] * self.pre_abs[R] + abs(self.s[q]) * self.pre_abs[rem])


WORST = {}  # label -> the largest |grad - exact| / A seen


def deviation(grad, exact, mass):
    """max_p |grad[p] - exact[p]| / A[p] (0 / 0 = 0, x / 0 = inf)"""
    assert np.all(np.isfinite(grad)), grad
    worst = 0.0
    for g, e, a in zip(grad, exact, mass):
        err = abs(Fraction(float(g)) - e)
        worst = max(worst, float(err / a) if a else (0.0 if err == 0 else np.inf))
    return worst


def check_sum(label, grad, exact, tol):
    """Assertion 1: every parameter within tol A[p] of the exact sum."""
    ex, mass = exact
    dev = deviation(grad, ex, mass)
    WORST[label] = max(WORST.get(label, 0.0), dev)
    if dev > tol:
        bad = [(p, float(grad[p]), float(ex[p]), float(mass[p])) for p in range(len(grad))
               if abs(Fraction(float(grad[p])) - ex[p]) > Fraction(tol) * mass[p]]
        raise AssertionError(f"{label}: |grad - exact| / A = {dev:.3e} > {tol:.3e}; "
                             f"(p, grad, exact, A) = {bad[:4]}")


def report():
    return "\n".join(f"  {k}: {v:.3e}" for k, v in sorted(WORST.items()))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64),
                          np.asarray(b, dtype=np.float64).view(np.int64))


def same_values(a, b):
    """Finite and equal: the same bits but for the sign of a zero (a parameter no ray
    reaches sums to +0 or -0 with the signs of its rays' cotangents)."""
    return bool(np.all(np.isfinite(a)) and np.array_equal(a, b))


# -- the two builds ------------------------------------------------------------------------
class Backend:
    """One build of the gradient code: "host" (liboptiland_host.so on CPU tensors) or
    "device" (the HIP library). Lenses, schedules, generated rays and n = 1 terms are made
    once and kept."""

    def __init__(self, kind):
        import torch

        from optiland_pr_amd import _native

        self.kind, self.torch = kind, torch
        self.dev = torch.device("cpu" if kind == "host" else "cuda")
        self.lib = _native.load_host() if kind == "host" else _native.load()
        self._lens, self._sched, self._terms, self._gin, self._rays = {}, {}, {}, {}, {}

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def lens(self, name):
        if name not in self._lens:
            from optiland_pr_amd.host import HostLens
            from optiland_pr_amd.raytrace import DeviceLens

            table, seg = lowered(name)
            dl = HostLens(table) if self.kind == "host" else DeviceLens(table, device=self.dev)
            seg_t = self.up(np.frombuffer(seg.tobytes(), dtype=np.uint8).copy())
            self._lens[name] = (dl, seg_t)
        return self._lens[name]

    def trace(self, row):
        """The base set traced once: (outputs [8][R] host array, schedule tensor or None)."""
        if row in self._sched:
            return self._sched[row]
        from optiland_pr_amd import host, ops
        from optiland_pr_amd.raytrace import RealRays, trace_pupil

        dl, seg = self.lens(ROWS[row]["lens"])
        b = base(row)
        px, py = self.up(b.px), self.up(b.py)
        if self.kind == "host":
            outs, updates = host.trace_pupil(dl, seg, px, py, R, R, True)
            sched = updates if dl.newton else None
        else:
            out = RealRays.empty(R, dl.table.wavelengths[0], device=self.dev)
            trace_pupil(dl, seg, px, py, out, R, R, R, pupil_per_ray=True)
            outs = [getattr(out, a) for a in FIELDS]
            sched = ops._schedule_tensor(dl) if dl.newton else None
        res = (np.stack([t.cpu().numpy() for t in outs]), sched)
        self._sched[row] = res
        return res

    def rays(self, row):
        """The rays ort_generate_rays makes for the base set: [8][R] host array."""
        if row not in self._rays:
            import ctypes as C

            from optiland_pr_amd import _calls
            from optiland_pr_amd.raytrace import _stream_handle

            _, seg = self.lens(ROWS[row]["lens"])
            b = base(row)
            px, py = self.up(b.px), self.up(b.py)
            out = [self.torch.empty(R, dtype=self.torch.float64, device=self.dev)
                   for _ in range(8)]
            bt = _calls.pupil_batch(R, R, R, seg, True, None)
            oc = _calls.rays_struct(out)
            if self.kind == "host":
                rc = self.lib.ort_host_generate_rays(_calls.addr(px), _calls.addr(py),
                                                     C.byref(oc), C.byref(bt))
            else:
                rc = self.lib.ort_generate_rays(_calls.addr(px), _calls.addr(py), C.byref(oc),
                                                C.byref(bt), _stream_handle())
            assert rc == 0, rc
            self._rays[row] = np.stack([t.cpu().numpy() for t in out])
        return self._rays[row]

    def vjp(self, row, px, py, cot, rays_in=None, grad0=None, want_in=False):
        """One VJP call of the row's entry point over the given rays (host arrays; px, py per
        ray, or rays_in [8][n] for the resident entry): the gradient [n_param] as a host array
        (grad0: accumulated onto it, else overwritten / started from zero), and the input-ray
        cotangents [8][n] when want_in."""
        spec, tb = ROWS[row], tables(row)
        dl, seg = self.lens(spec["lens"])
        _, sched = self.trace(row)
        n = cot.shape[1]
        torch = self.torch
        cot_t = [self.up(c) for c in cot]
        grad = self.up(np.zeros(tb.n_param) if grad0 is None else grad0).clone()
        old = os.environ.get("ORT_VJP_TANGENTS")
        if "tangents" in spec:
            os.environ["ORT_VJP_TANGENTS"] = str(spec["tangents"])
        try:
            if spec.get("resident"):
                from optiland_pr_amd import ops

                rin = [self.up(c) for c in rays_in]
                gin = ([torch.zeros(n, dtype=torch.float64, device=self.dev) for _ in range(8)]
                       if want_in else None)
                ops._seq_vjp(dl, rin, None, False, 0, sched, tb.zp, tb.st, tb.ft, tb.n_param,
                             cot_t, None, None, grad, gin, spec["mode"], tb.need)
                g = grad.cpu().numpy()
                return (g, np.stack([t.cpu().numpy() for t in gin])) if want_in else g
            self._pupil_vjp(row, dl, seg, self.up(px), self.up(py), n, sched, tb, cot_t, grad,
                            spec["mode"], overwrite=grad0 is None)
        finally:
            if old is None:
                os.environ.pop("ORT_VJP_TANGENTS", None)
            else:
                os.environ["ORT_VJP_TANGENTS"] = old
        return grad.cpu().numpy()

    def _pupil_vjp(self, row, dl, seg, px, py, n, sched, tb, cot, grad, mode, overwrite):
        tabs = [None if a is None else dl.resident(("sums_tangent", ROWS[row]["pset"], i), a)
                for i, a in enumerate((tb.zp, tb.st, tb.ft, tb.need))]
        if self.kind == "device":
            from optiland_pr_amd import autodiff

            autodiff.vjp(dl, seg, px, py, n, n, sched, tabs, tb.n_param, cot, grad,
                         pupil_per_ray=True, mode=mode, tape=None, overwrite=overwrite)
            return
        import ctypes as C

        from optiland_pr_amd import _calls, _native

        # (host.trace_pupil_vjp always overwrites: the same call with grad_init as asked)
        bt = _calls.pupil_batch(n, n, n, seg, True, None)
        opt = _native.ort_options(_abi.NEWTON_SCHEDULE, 0, _calls.addr(sched))
        params = _calls.vjp_params(dl.table, tb.n_param, mode, tabs[:3], tabs[3], overwrite)
        rc = self.lib.ort_host_trace_pupil_vjp(
            C.byref(dl.c), _calls.addr(px), _calls.addr(py), C.byref(bt), C.byref(opt),
            C.byref(params), C.byref(_calls.rays_struct(cot)), _calls.addr(grad))
        _native.check(rc, "ort_host_trace_pupil_vjp")

    def run_rays(self, row, idx, cot, grad0=None, want_in=False):
        """The row's VJP over the base rays idx [n] with the cotangents cot [8][n]."""
        b = base(row)
        rin = None
        if ROWS[row].get("resident"):
            rin = np.ascontiguousarray(self.rays(row)[:, idx])
        return self.vjp(row, np.ascontiguousarray(b.px[idx]), np.ascontiguousarray(b.py[idx]),
                        cot, rin, grad0, want_in)

    def run(self, row, n, grad0=None, want_in=False):
        """The row's VJP over the n-ray batch."""
        idx, cot, _ = batch(row, n)
        return self.run_rays(row, idx, cot, grad0, want_in)

    def terms(self, row):
        """t_r[p] [R][n_param] of the base set from R launches of one ray each (and, for the
        resident entry, the input-ray cotangents [8][R] of the same launches)."""
        if row not in self._terms:
            b = base(row)
            resident = bool(ROWS[row].get("resident"))
            rays = self.rays(row) if resident else None
            out, gin = [], []
            for r in range(R):
                sl = slice(r, r + 1)
                res = self.vjp(row, b.px[sl], b.py[sl], np.ascontiguousarray(b.cot[:, sl]),
                               None if rays is None else np.ascontiguousarray(rays[:, sl]),
                               want_in=resident)
                if resident:
                    out.append(res[0])
                    gin.append(res[1][:, 0])
                else:
                    out.append(res)
            self._terms[row] = np.stack(out)
            if resident:
                self._gin[row] = np.stack(gin, axis=1)
        return self._terms[row]

    def gin_terms(self, row):
        self.terms(row)
        return self._gin[row]

    @functools.lru_cache(maxsize=None)
    def exact(self, row):
        return Exact(self.terms(row))


@functools.lru_cache(maxsize=None)
def backend(kind):
    return Backend(kind)


def clipped(be, row):
    """bool [R]: the base rays an aperture clipped (intensity 0 at the image)"""
    outs, _ = be.trace(row)
    return outs[FIELDS.index("i")] == 0.0


def padded(row, m, n, pad_from=None):
    """(base ray [n], cot [8][n]) of n rays: the first m of the base set, then rows with zero
    cotangents on every output (their rays: the base set's next ones, or drawn in turn from
    the rays pad_from flags)."""
    idx = np.arange(n) % R
    if pad_from is not None:
        pool = np.flatnonzero(pad_from)
        idx[m:] = pool[np.arange(n - m) % len(pool)]
    cot = np.ascontiguousarray(base(row).cot[:, idx])
    cot[:, m:] = 0.0
    return idx, cot


def padding_pair(be, row, m, n, pad_from=None):
    """The gradients of the m-ray batch and of the same rays padded to n"""
    idx, cot = padded(row, m, n, pad_from)
    return (be.run_rays(row, idx[:m], np.ascontiguousarray(cot[:, :m])),
            be.run_rays(row, idx, cot))


def seeded_grad(row, like):
    """Seeded values to prefill a gradient with, of the size of `like`'s entries"""
    gen = np.random.default_rng(31)
    return gen.standard_normal(like.shape) * np.maximum(np.abs(like), 1e-3)


PADDING = ((1, 256), (63, 256), (65, 256), (200, 256), (1, 257), (63, 257), (65, 257),
           (200, 257), (257, 512))


# -- the assertions both test files make, on either build ------------------------------------
def assert_sum(be, row, n):
    """Assertion 1 at one size."""
    check_sum(f"{be.kind} {row}", be.run(row, n), be.exact(row).sum(n), TOL)


def assert_padding(be, row, m, n, pad_from=None):
    """Zero-cotangent rows add nothing: the same bits (at most 256 partial columns, so the
    addition trees coincide and the added terms are zeros)."""
    a, b = padding_pair(be, row, m, n, pad_from)
    assert same_bits(a, b), f"{be.kind} {row}: {m} rays vs padded to {n}: {a - b}"


def assert_deterministic(be, row, n):
    a, b = be.run(row, n), be.run(row, n)
    assert np.all(np.isfinite(a)) and same_bits(a, b), f"{be.kind} {row} n={n}: {a - b}"


def assert_accumulates(be, row, n=R):
    """grad_init = 0: the call returns fl(g0 + g) of the overwriting call's g, exactly."""
    g = be.run(row, n)
    g0 = seeded_grad(row, g)
    got = be.run(row, n, grad0=g0)
    assert same_bits(got, g0 + g), f"{be.kind} {row}: {got - (g0 + g)}"


def assert_resident_cotangents(be, row, n):
    """The input-ray cotangents of a batch are those of the n = 1 launches, scaled: bit for
    bit (elementwise, no sum)."""
    idx, _, s = batch(row, n)
    _, gin = be.run(row, n, want_in=True)
    assert same_bits(gin, be.gin_terms(row)[:, idx] * s), f"{be.kind} {row} n={n}"


def assert_clipped_input(be, row="cooke_aperture"):
    """The clipped row's condition on its input, and its clipped rays' terms."""
    c = clipped(be, row)
    assert 0.05 <= c.mean() <= 0.60, c.mean()
    assert np.all(np.isfinite(be.terms(row)[c]))
    return c


def measure(kind="host", rows=None, sizes=None):
    """The largest |grad - exact| / A of `kind`'s batched gradients against its own n = 1
    terms over every row and size (python -c "from tests import _vjp_sums as V;
    print(V.measure())"); the per-row values are left in WORST."""
    be = backend(kind)
    worst = 0.0
    for row in (rows or (HOST_ROWS if kind == "host" else tuple(ROWS))):
        ex = be.exact(row)
        for n in (sizes or sizes_of(row)):
            if n not in sizes_of(row):
                continue
            dev = deviation(be.run(row, n), *ex.sum(n))
            WORST[f"{kind} {row}"] = max(WORST.get(f"{kind} {row}", 0.0), dev)
            worst = max(worst, dev)
    return worst


TOL = 16 * HOST_DEV
assert TOL <= CAP  # a condition, not a measurement
