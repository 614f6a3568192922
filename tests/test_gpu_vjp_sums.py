"""The gradient kernels' ray sums on the MI355X against exact sums (tests/_vjp_sums.py: the
method, the rows, the bound): adj_kernel's per-slot wave sums, monomial chunks and block
epilogue, adj_slot_reduce_kernel's strided, 8-way unrolled and tail loops, adj_grad_kernel's
contraction in both store modes, vjp_kernel / vjp_reduce_kernel<1 | 2 | 4>, for generated and
resident rays -- at 1 to 257 rays (one lane, a wave and a block and their neighbours, a block
whose trailing waves are idle) and at 256 | 257, 1792 | 1793 and 2049 partial columns.

  * every row, size and parameter within T A[p] of the exact sum of the device's own
    one-ray terms;
  * the anchor: at 257 rays the host build's gradient meets the same bound against the
    device's one-ray terms, and the device's against the host's (the one-ray launches tied
    to code without any lane machinery);
  * exact: zero-cotangent padding, run-to-run bits, the accumulating call, the resident
    entry's input-ray cotangents, clipped rays.
tests/test_vjp_sums_cpu.py makes the same checks of the host build and measures T.
"""

import numpy as np
import pytest

from tests import _vjp_sums as V

pytestmark = pytest.mark.gpu

SUMS = [(row, n) for row in V.ROWS for n in V.sizes_of(row)]
EXACT_ROWS = ("cooke", "rt_asph", "tma_fringe", "tma_fringe_slots", "tma_fringe25",
              "tma_standard_t1", "tma_standard_t2", "tma_standard_t4", "cooke_resident",
              "tma_fringe_resident")


@pytest.fixture(scope="module")
def be():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("needs the MI355X")
    V.WORST.clear()
    yield V.backend("device")
    print("\nlargest |grad - exact| / A on the device (T = "
          f"{V.TOL:.2e}):\n" + V.report())


@pytest.fixture(scope="module")
def host():
    return V.backend("host")


def test_scaled_copies_are_exact(be):
    """Scaling a ray's cotangents by +-2^e scales its term exactly: one-ray launches with
    scaled cotangents, every kernel family."""
    for row in V.ROWS:
        t = be.terms(row)
        b = V.base(row)
        for r, s in ((0, -0.015625), (100, 64.0), (256, -2.0)):
            g = be.run_rays(row, np.arange(r, r + 1),
                            np.ascontiguousarray(b.cot[:, r:r + 1] * s))
            assert V.same_values(g, t[r] * s), (row, r, s)


@pytest.mark.parametrize("row,n", SUMS, ids=[f"{r}-{n}" for r, n in SUMS])
def test_sum_against_exact(be, row, n):
    V.assert_sum(be, row, n)


@pytest.mark.parametrize("row", V.HOST_ROWS)
def test_host_anchor(be, host, row):
    """257 rays: host gradient vs the device's one-ray terms, device gradient vs the host's."""
    sd, sh = be.trace(row)[1], host.trace(row)[1]
    assert (sd is None) == (sh is None)
    if sd is not None:  # one Newton schedule for both builds
        assert np.array_equal(sd.cpu().numpy().ravel(), sh.numpy().ravel())
    V.check_sum(f"host vs device terms {row}", host.run(row, V.R), be.exact(row).sum(V.R), V.TOL)
    V.check_sum(f"device vs host terms {row}", be.run(row, V.R), host.exact(row).sum(V.R), V.TOL)


@pytest.mark.parametrize("row", EXACT_ROWS)
@pytest.mark.parametrize("m,n", V.PADDING)
def test_padding_adds_nothing(be, row, m, n):
    V.assert_padding(be, row, m, n)


@pytest.mark.parametrize("row", ("cooke", "tma_fringe", "tma_standard_t4"))
@pytest.mark.parametrize("n", (V.R, 458753))
def test_same_launch_same_bits(be, row, n):
    V.assert_deterministic(be, row, n)


@pytest.mark.parametrize("row", ("cooke", "tma_fringe", "tma_fringe_slots", "tma_standard_t1",
                                 "tma_standard_t2", "tma_standard_t4"))
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
