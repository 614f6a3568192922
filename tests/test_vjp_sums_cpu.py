"""No GPU: the host build's gradient sums (ort_host_trace_pupil_vjp /
ort_host_trace_sequential_vjp: adj_chunks / vjp_chunks, the chunk and slot sums, the slot
contraction) against the exact sums of tests/_vjp_sums.py, and that helper validated before
a device sees it: the per-ray terms come from launches of one ray, a batch is scaled copies
of the base set, and the host's batched gradients meet the bound T A[p] that
tests/test_gpu_vjp_sums.py holds the device to. The value measured here is the HOST_DEV that T
is sixteen times of.

Sizes: the prefixes of the base set and 65,536 | 65,537 rays (256 | 257 chunks); the larger
sizes of the device's tests are measured by _vjp_sums.measure() and not run here.
"""

import numpy as np
import pytest

from tests import _vjp_sums as V

CPU_SIZES = V.SMALL + V.MID
SUMS = [(row, n) for row in V.HOST_ROWS for n in V.sizes_of(row) if n in CPU_SIZES]
EXACT_ROWS = ("cooke", "tma_fringe", "tma_fringe25", "tma_standard_t4", "cooke_resident",
              "tma_fringe_resident")


@pytest.fixture(scope="module")
def be():
    V.WORST.clear()
    yield V.backend("host")
    print("\nlargest |grad - exact| / A on the host:\n" + V.report())


def test_parameter_sets():
    """Each row's tables select the kernel family it is there for, and the forward-mode rows
    end on a ragged chunk at every chunk width."""
    for row, spec in V.ROWS.items():
        tb = V.tables(row)
        assert (tb.st is not None) == (spec["pset"] == "slots")  # surf_tangent: P = 4
        assert tb.ft[tb.n_slots - 1] == 1.0 and np.count_nonzero(tb.ft) == 1
        if spec["pset"] == "slots":
            S = V.lowered(spec["lens"])[0].n_surfaces
            assert np.array_equal(tb.st[:3 * S].reshape(3 * S, 3 * S), np.eye(3 * S))
            assert np.any(np.count_nonzero(tb.st[tb.n_slots:, :, 2], axis=1) > 1)  # a thickness
        if tb.zp is not None:
            assert np.array_equal(np.sort(tb.zp), np.arange(tb.zp[0], tb.zp[0] + len(tb.zp)))
        if spec["mode"] == V.UNR:
            assert tb.n_param % 4 == 3
    assert V.TOL == 16 * V.HOST_DEV <= V.CAP


def test_scaled_copies_are_exact(be):
    """Scaling a ray's cotangents by +-2^e scales its term exactly (what the reference of
    every larger batch rests on): one-ray launches with scaled cotangents, both modes."""
    for row in ("cooke", "tma_fringe", "tma_standard_t4", "cooke_aperture"):
        t = be.terms(row)
        b = V.base(row)
        for r, s in ((0, -0.015625), (100, 64.0), (256, -2.0)):
            sl = slice(r, r + 1)
            g = be.run_rays(row, np.arange(r, r + 1), np.ascontiguousarray(b.cot[:, sl] * s))
            assert V.same_values(g, t[r] * s), (row, r, s)


@pytest.mark.parametrize("row,n", SUMS, ids=[f"{r}-{n}" for r, n in SUMS])
def test_sum_against_exact(be, row, n):
    V.assert_sum(be, row, n)


def test_measured_host_dev(be):
    """HOST_DEV of tests/_vjp_sums.py is what the host build measures here (its largest
    value falls on a size this file runs)."""
    worst = V.measure("host", sizes=CPU_SIZES)
    print(f"\nhost |grad - exact| / A: {worst:.3e} (HOST_DEV {V.HOST_DEV:.3e})")
    assert 0.9 * V.HOST_DEV <= worst <= V.HOST_DEV


@pytest.mark.parametrize("row", EXACT_ROWS)
@pytest.mark.parametrize("m,n", V.PADDING)
def test_padding_adds_nothing(be, row, m, n):
    V.assert_padding(be, row, m, n)


@pytest.mark.parametrize("row", ("tma_fringe", "tma_standard_t4"))
@pytest.mark.parametrize("n", (V.R, 65537))
def test_same_launch_same_bits(be, row, n):
    V.assert_deterministic(be, row, n)


@pytest.mark.parametrize("row", ("cooke", "tma_fringe", "tma_standard_t4"))
def test_accumulating_call_adds_once(be, row):
    V.assert_accumulates(be, row)


@pytest.mark.parametrize("row", ("cooke_resident", "tma_fringe_resident"))
@pytest.mark.parametrize("n", (V.R, 65537))
def test_resident_input_cotangents(be, row, n):
    V.assert_resident_cotangents(be, row, n)


def test_clipped_rays(be):
    """cooke_aperture: 5% to 60% of the base rays are clipped, their terms are finite (the
    sum itself: test_sum_against_exact[cooke_aperture-257]), and zero-cotangent rows placed
    on clipped rays add nothing."""
    c = V.assert_clipped_input(be)
    for m, n in V.PADDING:
        V.assert_padding(be, "cooke_aperture", m, n, pad_from=c)
