"""The analysis reductions on the MI355X, each C entry point on data the test controls:
ort_spot_stats, ort_spot_partials, ort_rms_spot, ort_rms_spot_vjp, ort_rms_finish and
ort_wavefront_opd at the chunk, tile and row edges of their kernels, for a centred point set
and a far, tight one (where the sums cancel), against the extended-precision references and
the bounds of tests/_reductions.py (derived there; relative tolerance 0, every bound from the
test's own arrays). tests/test_reductions_cpu.py shows on the CPU that the kernels' order of
additions meets the same bounds.
"""

import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _reductions as R

pytestmark = pytest.mark.gpu

KINDS = R.POINT_SETS


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("needs the MI355X")
    from optiland_pr_amd import _native
    import optiland_pr_amd.ops  # noqa: F401  (registers torch.ops.ort)

    R.WORST.clear()
    yield SimpleNamespace(torch=torch, lib=_native.load(), native=_native,
                          dev=torch.device("cuda"))
    print("\nlargest error / bound on the device:\n" + R.report())


def up(g, a):
    return g.torch.tensor(np.ascontiguousarray(a), dtype=g.torch.float64, device=g.dev)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream(g):
    return C.c_void_p(g.torch.cuda.current_stream().cuda_stream)


class Rays:
    """Device arrays behind an ort_rays (the fields a kernel does not read stay NULL)."""

    def __init__(self, g, **arrays):
        self.t = {k: up(g, v) for k, v in arrays.items()}
        self.c = g.native.ort_rays()
        for k, t in self.t.items():
            setattr(self.c, k, t.data_ptr() or None)

    def c_struct(self):
        return self.c


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def assert_bit_exact(got, exp, what):
    """Equal bit for bit where exp is a number (the sign of zero included), NaN where it is
    NaN (a NaN's sign and payload are not the operation's result)."""
    nan = np.isnan(exp)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
    assert same_bits(got[~nan], exp[~nan]), what


# -- ort_spot_stats ---------------------------------------------------------------------
def spot_stats(g, p, sl=slice(None)):
    from optiland_pr_amd.analysis import SpotStatistics

    surface = None
    if p.ops is not None:
        surface = SimpleNamespace(geometry=SimpleNamespace(cs=R.image_cs()))
    n = p.x[:, sl].shape[1]
    st = SpotStatistics(R.N_FIELDS, R.N_WL, n, R.REF_WL, surface, g.dev)
    rays = Rays(g, x=p.x[:, sl], y=p.y[:, sl], z=p.z[:, sl], i=p.i[:, sl])
    return st, rays


def spot_ref(p, k=None, gsum=None, sl=slice(None)):
    n = p.xl[:, sl].shape[1]
    return R.spot_reference(p.xl[:, sl], p.yl[:, sl], p.i[:, sl], R.N_FIELDS, R.N_WL, R.REF_WL,
                            R.chain(n) if k is None else k, gsum)


def expect_variant(variant, out):
    """What each variant must do to the rows [6][5] (field 0: pairs 0-2, field 1: 3-5)."""
    f0, f1 = out[:3], out[3:]
    if variant == "ref_masked":    # every radius of the field NaN, the other field untouched
        assert f0[R.REF_WL, 0] == 0 and np.all(np.isnan(f0[:, 3:]))
        assert np.all(np.isfinite(f0[[0, 2], 1:3])) and np.all(np.isfinite(f1))
    elif variant == "nan_tail":    # only that pair goes NaN (its x is NaN, its y is not)
        assert np.all(np.isnan(out[2, [1, 3, 4]])) and np.isfinite(out[2, 2])
        assert np.all(np.isfinite(np.delete(out, 2, axis=0)))
    elif variant == "nan_ref":     # the field's radii NaN, the other pairs' centroids finite
        assert np.all(np.isnan(f0[:, 3:])) and np.all(np.isfinite(f0[[0, 2], 1:3]))
        assert np.all(np.isnan(f0[R.REF_WL, 2:])) and np.all(np.isfinite(f1))
    elif variant == "inf":         # inf - inf in the ref pair, inf radii in the others
        assert np.all(np.isfinite(f0)) and f1[R.REF_WL, 2] == np.inf
        assert np.all(np.isnan(f1[R.REF_WL, 3:])) and np.all(f1[[0, 2], 3:] == np.inf)
    else:
        assert np.all(np.isfinite(out))


SPOT_CASES = [(n, "plain") for n in R.SPOT_SIZES] + \
    [(n, v) for n in R.SPOT_VARIANT_SIZES for v in R.SPOT_VARIANTS]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,variant", SPOT_CASES)
def test_spot_stats(gpu, kind, n, variant):
    p = R.spot_problem(kind, n, variant)
    st, rays = spot_stats(gpu, p)
    out = st.run(rays).cpu().numpy()
    R.check_spot_rows(f"ort_spot_stats {kind}", out, spot_ref(p))
    if n >= 257:
        expect_variant(variant, out)
    if n == 0:  # one empty chunk: no point, NaN statistics
        assert np.all(out[:, 0] == 0) and np.all(np.isnan(out[:, 1:]))
    if n == 131073:
        again = st.run(rays).cpu().numpy()
        assert same_bits(out, again)


# -- ort_spot_partials ------------------------------------------------------------------
def partials(g, st, rays, phase, sums1):
    out = g.torch.empty((R.N_FIELDS * R.N_WL, 3), dtype=g.torch.float64, device=g.dev)
    rc = g.lib.ort_spot_partials(C.byref(rays.c_struct()), C.byref(st._lay), phase, ptr(sums1),
                                 C.c_void_p(st._ws.data_ptr()), st._size, ptr(out), stream(g))
    g.native.check(rc, "ort_spot_partials")
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", R.PARTIAL_SIZES)
def test_spot_partials_two_ranks(gpu, kind, n):
    """Two simulated ranks' slices: phase 1 rows, phase 2 rows about the centroid of the
    combined sums (not this rank's own), and the rows combined as distributed.py combines
    them against the statistics of the unsplit data."""
    from optiland_pr_amd.distributed import combine_spot_partials, finalize_spot

    p = R.spot_problem(kind, n)
    ranks = (slice(0, n // 2), slice(n // 2, n))
    dev = [spot_stats(gpu, p, sl) for sl in ranks]
    parts1 = [partials(gpu, st, rays, 1, None) for st, rays in dev]
    for sl, rows in zip(ranks, parts1, strict=True):
        R.check_partial_rows(f"ort_spot_partials {kind}", 1, rows.cpu().numpy(),
                             spot_ref(p, sl=sl))
    s1 = combine_spot_partials(gpu.torch.stack(parts1))
    gsum = s1.cpu().numpy()
    parts2 = [partials(gpu, st, rays, 2, s1) for st, rays in dev]
    for sl, own, rows in zip(ranks, parts1, parts2, strict=True):
        if n > 1:
            assert not gpu.torch.equal(own, s1)  # a centroid this rank's rows do not hold
        rows = rows.cpu().numpy()
        R.check_partial_rows(f"ort_spot_partials {kind}", 2, rows,
                             spot_ref(p, gsum=gsum, sl=sl))
        if sl.stop == sl.start:  # an empty slice: sum 0, max radius 0, flag 0 (header)
            assert np.all(rows == 0.0)
    s1, s2 = combine_spot_partials(gpu.torch.stack(parts1), gpu.torch.stack(parts2))
    out, _ = finalize_spot(s1, s2, R.N_FIELDS, R.N_WL, R.REF_WL)
    k = max(R.chain(sl.stop - sl.start) for sl in ranks) + len(ranks) - 1
    R.check_spot_rows(f"ort_spot_partials combined {kind}", out.cpu().numpy(), spot_ref(p, k=k))
    if n == 65537:
        st, rays = dev[1]
        assert gpu.torch.equal(partials(gpu, st, rays, 2, s1), parts2[1])


@pytest.mark.parametrize("kind", KINDS)
def test_spot_partials_nan_flag(gpu, kind):
    """A NaN point that counts: phase 2 reports it in the flag, the max is of the rest."""
    p = R.spot_problem(kind, 257, "nan_tail")
    st, rays = spot_stats(gpu, p)
    s1 = partials(gpu, st, rays, 1, None)
    rows = partials(gpu, st, rays, 2, s1).cpu().numpy()
    R.check_partial_rows(f"ort_spot_partials {kind}", 2, rows,
                         spot_ref(p, gsum=s1.cpu().numpy()))
    assert rows[2, 2] == 1.0 and math.isnan(rows[2, 0])
    assert np.all(np.delete(rows, 2, axis=0)[:, 2] == 0)


# -- ort_rms_spot and its vjp -----------------------------------------------------------
def rms_ref(p):
    return R.spot_reference(p.x[None], p.y[None], None, 1, 1, 0, R.chain(p.n, R.RMS_MAX_CHUNKS))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,nan", [(n, False) for n in (0, *R.RMS_SIZES)]
                         + [(257, True), (65537, True)])
def test_rms_spot_and_vjp(gpu, kind, n, nan):
    torch = gpu.torch
    p = R.rms_problem(kind, n, nan)
    x, y = up(gpu, p.x), up(gpu, p.y)
    rms, stats_dev = torch.ops.ort.rms_spot(x, y)
    stats = stats_dev.cpu().numpy()
    assert same_bits(rms.cpu().numpy(), stats[3])
    R.check_spot_rows(f"ort_rms_spot {kind}", stats[None], rms_ref(p))
    if nan or n == 0:  # n = 0: count 0, NaN statistics; the NaN point's x is NaN, its y not
        assert stats[0] == n and np.all(np.isnan(stats[[1, 3, 4]]))
        assert np.isnan(stats[2]) == (n == 0)
    g = torch.tensor(0.37, dtype=torch.float64, device=gpu.dev)  # read on the device
    gx, gy = torch.ops.ort.rms_spot_vjp(x, y, stats_dev, g)
    rx, ry, bx, by = R.vjp_reference(p.x, p.y, stats, 0.37)
    R.check_array(f"ort_rms_spot_vjp {kind}", gx.cpu().numpy(), rx, bx)
    R.check_array(f"ort_rms_spot_vjp {kind}", gy.cpu().numpy(), ry, by)
    if n == 262145:
        rms2, stats2 = torch.ops.ort.rms_spot(x, y)
        gx2, gy2 = torch.ops.ort.rms_spot_vjp(x, y, stats_dev, g)
        assert same_bits(stats, stats2.cpu().numpy()) and torch.equal(rms, rms2)
        assert torch.equal(gx, gx2) and torch.equal(gy, gy2)


# -- ort_rms_finish ---------------------------------------------------------------------
def rms_finish(g, rows):
    stats = g.torch.empty(5, dtype=g.torch.float64, device=g.dev)
    rms = g.torch.empty((), dtype=g.torch.float64, device=g.dev)
    rc = g.lib.ort_rms_finish(ptr(rows), rows.shape[0], ptr(stats), ptr(rms), stream(g))
    g.native.check(rc, "ort_rms_finish")
    return stats.cpu().numpy(), rms.cpu().numpy()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("variant", R.FINISH_VARIANTS)
@pytest.mark.parametrize("n_rows", R.FINISH_ROWS)
def test_rms_finish(gpu, kind, n_rows, variant):
    p = R.finish_problem(kind, n_rows, variant)
    rows = up(gpu, p.rows)
    stats, rms = rms_finish(gpu, rows)
    assert same_bits(rms, stats[3])
    R.check_finish(f"ort_rms_finish {kind}", stats, R.finish_reference(p.rows))
    if n_rows == 4353:
        assert same_bits(rms_finish(gpu, rows)[0][:4], stats[:4])


@pytest.fixture(scope="module")
def newton_lens(gpu):
    from optiland_pr_amd.raytrace import lens_for
    from tests._cases import build_lens

    lens = build_lens("rt_asph")  # (alive as long as its lowered form is in use)
    yield lens_for(lens, [0.5876])


def newton_finish_rms(g, dl, rows):
    """The smallest legal ort_newton_finish_rms call: one round that did not run (flags[0] =
    0, settled), so the first workgroup checks no statistics and the second finishes the rms."""
    torch = g.torch
    ngs = dl.table.n_surfaces  # one group
    words = torch.zeros(2 * 2 + 1 + 2 * ngs, dtype=torch.int32, device=g.dev)
    flags, statuses, status_out = words[0:2], words[2:4], words[4:5]
    sched, copy = words[5:5 + ngs], words[5 + ngs:]
    nstats = torch.full((2, ngs * 24), 255, dtype=torch.uint8, device=g.dev)
    stats = torch.empty(5, dtype=torch.float64, device=g.dev)
    rms = torch.empty((), dtype=torch.float64, device=g.dev)
    rc = g.lib.ort_newton_finish_rms(C.byref(dl.c), 1, ptr(nstats), 1, 0, ptr(sched), ptr(flags),
                                     ptr(statuses), ptr(status_out), ptr(copy), ptr(rows),
                                     rows.shape[0], ptr(stats), ptr(rms), stream(g))
    g.native.check(rc, "ort_newton_finish_rms")
    return stats.cpu().numpy(), rms.cpu().numpy()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_rows", (1, 255, 256, 257, 4096, 4097))
def test_rms_finish_same_bits_from_both_entry_points(gpu, newton_lens, kind, n_rows):
    """ort_rms_finish and the second workgroup of ort_newton_finish_rms run the same
    rms_finish_block<256, 16>: the same rows give the same bits (4096 rows: the last size
    held in registers, 4097: the first that re-reads a row)."""
    rows = up(gpu, R.finish_problem(kind, n_rows, "plain").rows)
    stats, rms = rms_finish(gpu, rows)
    stats_n, rms_n = newton_finish_rms(gpu, newton_lens, rows)
    assert same_bits(stats_n[:4].view(np.uint64), stats[:4].view(np.uint64))
    assert same_bits(rms_n.view(np.uint64), rms.view(np.uint64))
    assert math.isnan(stats[4]) and math.isnan(stats_n[4])


def test_rms_finish_argument_errors(gpu):
    buf = gpu.torch.zeros(8, dtype=gpu.torch.float64, device=gpu.dev)
    assert gpu.lib.ort_rms_finish(ptr(buf), 0, ptr(buf), ptr(buf), stream(gpu)) == -1
    assert gpu.lib.ort_rms_finish(None, 2, ptr(buf), ptr(buf), stream(gpu)) == -1


# -- ort_wavefront_opd ------------------------------------------------------------------
def wavefront(g, p, tilt, with_pupil):
    torch = g.torch
    rays = Rays(g, **p.rays)
    px, py = up(g, p.px), up(g, p.py)
    ref = g.native.ort_wavefront_ref()
    for f in R.WF_FIELDS:
        setattr(ref, f, p.ref[f])
    ref.tilt = tilt
    size = int(g.lib.ort_wavefront_workspace_size(p.n))
    ws = torch.empty(size // 8, dtype=torch.float64, device=g.dev)
    out = [torch.full((p.n,), 7.0, dtype=torch.float64, device=g.dev)
           for _ in range(4 if with_pupil else 1)]
    pupil = out[1:] if with_pupil else [None, None, None]
    sums = torch.empty(11, dtype=torch.float64, device=g.dev)
    rc = g.lib.ort_wavefront_opd(C.byref(rays.c_struct()), ptr(px), ptr(py), p.n, C.byref(ref),
                                 ptr(out[0]), *(ptr(t) for t in pupil), ptr(ws), size, ptr(sums),
                                 stream(g))
    g.native.check(rc, "ort_wavefront_opd")
    return [t.cpu().numpy() for t in out], sums.cpu().numpy()


@pytest.mark.parametrize("with_pupil", [True, False])
@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("tilt", [0, 1])
@pytest.mark.parametrize("n", R.WAVEFRONT_SIZES)
def test_wavefront_opd(gpu, n, tilt, nan, with_pupil):
    p = R.wavefront_problem(n, nan)
    out, sums = wavefront(gpu, p, tilt, with_pupil)
    *per_ray, terms = R.wavefront_terms(p.rays, p.px, p.py, p.ref, tilt)
    names = ("opd_wv", "pupil_x", "pupil_y", "pupil_z")
    for got, exp, name in zip(out, per_ray, names, strict=False):
        assert_bit_exact(got, exp, name)
    ref, bound = R.wavefront_reference(terms)
    for j in range(11):
        R.check("ort_wavefront_opd sums", sums[j], ref[j], bound[j])
    if nan and n > 1:  # a NaN intensity and a NaN ray that counts: only the count is a number
        assert math.isfinite(sums[0]) and np.all(np.isnan(sums[1:]))
    elif not nan:
        assert np.all(np.isfinite(sums))
    if n == 65537 and with_pupil:
        out2, sums2 = wavefront(gpu, p, tilt, with_pupil)
        assert same_bits(sums, sums2)
        assert all(same_bits(a, b) for a, b in zip(out, out2, strict=True))
