"""The plain closed-form kernel's sphere branches (ort_fastpath.h), restated operation for
operation with an exact fma (fractions.Fraction, rounded once), as
test_seed_sequences_cpu.py does for the (2 / R) h seed. No GPU.

normal_conic_rcp<true>, k == 0: the norm's root sqrt(X), X = dfdx^2 + dfdy^2 + 1, starts
from g = sqrt(1 - q) in v_rsq(X)'s place (sqrt_seeded_h). Checked: the bound on
|g sqrt(X) - 1| written at the function (2^-50), the root (== RN(sqrt(X))), the refined
1 / mag (within 2^-52) and the three normal components (== the IEEE quotients), with the
seed as it is and moved by +-2^-47. v_rsq of the first root is (1 + e0) / sqrt(x) rounded,
e0 = +-2^-20.

shared_div_unit: 1 / a of a unit direction's a = L^2 + M^2 + N^2 from 2 - a and one Newton
step, over |1 - a| <= 2^-27 and at the edge of its flag.
"""
import math
from fractions import Fraction

import numpy as np

from tests._fast_sequences import fma, numerators, quot, quot_pos, sqrt_h, sqrt_seeded_h

SEED_BOUND = Fraction(1, 2**50)  # the bound at normal_conic_rcp's sphere branch
Q_TARGETS = [0.0, 2.0**-60, 0.25, 0.9, 1 - 2.0**-10, 1 - 2.0**-40, 1 - 2.0**-52]
RADII = [22.01359, -435.76044, 1.0, -3.0, 2.0**150, -(2.0**150), 2.0**-150, -(2.0**-150),
         2.0**140 * 1.37, -(2.0**-140) * 1.91]
DIRS = [(1.0, 0.0), (0.0, -1.0), (0.6, -0.8)]


def _w_of(x, y, R):
    """fl(1 - q) of normal_conic_rcp for a sphere (one_plus_k = 1), with the host's r_sq,
    inv_r2."""
    r_sq = float(np.float64(R) * np.float64(R))
    inv_r2 = float(np.float64(1.0) / np.float64(r_sq))
    r2 = x * x + y * y
    a = 1.0 * r2
    q0 = a * inv_r2
    q = fma(fma(-r_sq, q0, a), inv_r2, q0)
    return 1.0 - q, q


def _ieee_div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _within(v, bound):
    """|sqrt(v) - 1| < bound for a positive Fraction v, without forming the root."""
    return (1 - bound) ** 2 < v < (1 + bound) ** 2


def _check_sphere_normal(x, y, R, e0):
    """One hit (x, y) on a sphere of radius R; -> (w, q) or None when 1 - q <= 0."""
    w, q = _w_of(x, y, R)
    if not w > 0.0:
        return None
    g, h = sqrt_h(w, e0)
    assert g == float(np.sqrt(np.float64(w))), (x, y, R)
    denom = R * g
    y0 = float(np.float64(2.0) / np.float64(R)) * h
    e = fma(-denom, y0, 1.0)
    yd = fma(y0, e, y0)
    dfdx, dfdy = quot(x, denom, yd), quot(y, denom, yd)
    assert dfdx == _ieee_div(x, denom) and dfdy == _ieee_div(y, denom), (x, y, R)
    X = dfdx * dfdx + dfdy * dfdy + 1.0
    assert math.isfinite(X) and X >= 1.0
    # the seed: |g sqrt(X) - 1| under the bound written at the function
    assert _within(Fraction(g) ** 2 * Fraction(X), SEED_BOUND), (x, y, R, w)
    mag_exp = float(np.sqrt(np.float64(X)))
    for p in (0.0, 2.0**-47, -(2.0**-47)):
        seed = g * (1.0 + p)
        mag, hm = sqrt_seeded_h(X, seed)
        assert mag == mag_exp, (x, y, R, p)
        s0 = 2.0 * hm
        e = fma(-mag, s0, 1.0)
        ym = fma(s0, e, s0)
        assert abs(Fraction(mag) * Fraction(ym) - 1) <= Fraction(1, 2**52), (x, y, R, p)
        assert quot_pos(dfdx, mag, ym) == _ieee_div(dfdx, mag), (x, y, R, p)
        assert quot_pos(dfdy, mag, ym) == _ieee_div(dfdy, mag), (x, y, R, p)
        assert quot(-1.0, mag, ym) == _ieee_div(-1.0, mag), (x, y, R, p)
    return w, q


def _hit(R, qt, cx, cy):
    """(x, y) along (cx, cy) with r^2 / R^2 ~ qt, moved inward until 1 - q > 0."""
    r = abs(R) * math.sqrt(qt)
    x, y = r * cx, r * cy
    for _ in range(64):
        if _w_of(x, y, R)[0] > 0.0:
            break
        x, y = float(np.nextafter(x, 0.0)), float(np.nextafter(y, 0.0))
    return x, y


def test_sphere_norm_seed_targets():
    ws = []
    for R in RADII:
        for qt in Q_TARGETS:
            for i, (cx, cy) in enumerate(DIRS):
                x, y = _hit(R, qt, cx, cy)
                out = _check_sphere_normal(x, y, R, 2.0**-20 if i % 2 else -(2.0**-20))
                assert out is not None, (R, qt)
                ws.append(out[0])
    # q = 0: g = 1, X = 1; and the low end of fl(1 - q) > 0
    assert max(ws) == 1.0 and min(ws) <= 2.0**-51


def test_sphere_norm_seed_random():
    rng = np.random.default_rng(11)
    n = 200
    qs = rng.uniform(0.0, 1.0, n)
    qs[: n // 4] = 1.0 - np.ldexp(rng.uniform(1.0, 2.0, n // 4), rng.integers(-50, -2, n // 4))
    radii = np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-150, 150, n)) * rng.choice([-1.0, 1.0], n)
    th = rng.uniform(0.0, 2 * np.pi, n)
    done = 0
    for qt, R, t, e0 in zip(qs, radii, th, rng.choice([-(2.0**-20), 2.0**-20], n)):
        x, y = _hit(float(R), float(qt), math.cos(t), math.sin(t))
        done += _check_sphere_normal(x, y, float(R), float(e0)) is not None
    assert done == n


def test_vertex_hit_is_exact():
    for R in RADII:
        w, q = _check_sphere_normal(0.0, 0.0, R, 2.0**-20)
        assert (w, q) == (1.0, 0.0)


# ---- shared_div_unit ----------------------------------------------------------------------

def _unit_flag(a):  # ORT_CHK(bad, !(fabs(1.0 - a) <= 0x1p-27))
    return not abs(1.0 - a) <= 2.0**-27


def _unit_rcp(a):
    y0 = 2.0 - a
    e = fma(-a, y0, 1.0)
    return y0, fma(y0, e, y0)


def test_unit_reciprocal():
    rng = np.random.default_rng(12)
    lo, hi = 1.0 - 2.0**-27, 1.0 + 2.0**-27
    vals = [1.0, lo, hi, float(np.nextafter(lo, 2.0)), float(np.nextafter(hi, 0.0)),
            float(np.nextafter(1.0, 0.0)), float(np.nextafter(1.0, 2.0)), 1.0 - 2.0**-40,
            1.0 + 2.0**-40, 1.0 - 2.0**-28, 1.0 + 2.0**-28]
    vals += [float(v) for v in 1.0 + rng.uniform(-1.0, 1.0, 150) * 2.0**-27]
    vals += [float(v) for v in 1.0 + rng.uniform(-1.0, 1.0, 50) * 2.0**-50]
    for a in vals:
        assert not _unit_flag(a), a
        y0, y = _unit_rcp(a)
        # the seed: (1 - (1 - a)^2) / a and the rounding of 2 - a
        assert abs(Fraction(a) * Fraction(y0) - 1) < Fraction(1, 2**52), a
        assert abs(Fraction(a) * Fraction(y) - 1) <= Fraction(1, 2**52), a
        for n in numerators(rng, 6):
            n = float(n)
            assert quot_pos(n, a, y) == _ieee_div(n, a), (a, n)


def test_unit_flag_edges():
    lo, hi = 1.0 - 2.0**-27, 1.0 + 2.0**-27
    assert not _unit_flag(lo) and not _unit_flag(hi)
    assert _unit_flag(float(np.nextafter(lo, 0.0))) and _unit_flag(float(np.nextafter(hi, 2.0)))
    for a in (float("nan"), float("inf"), 0.0, -1.0, 2.0, 2.0**300, 2.0**-1074):
        assert _unit_flag(a), a
