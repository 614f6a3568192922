"""The gfx950 fp64 sequences of csrc/ort_core.h (sqrt_seeded_h, quot, quot_pos) restated
operation for operation in Python with an exact fma (fractions.Fraction, rounded once), and
a model of v_rsq. Shared by test_seed_sequences_cpu.py, test_sphere_norm_seed_cpu.py and
test_one_root_cpu.py. No GPU.
"""
import math
from fractions import Fraction

import numpy as np


def rn(v):
    """A Fraction rounded to the nearest double, ties to even (int / int is exact)."""
    return v.numerator / v.denominator


def fma(a, b, c):
    return rn(Fraction(a) * Fraction(b) + Fraction(c))


def quot(a, b, y):  # ort_core.h quot
    q0 = a * y
    r = fma(-b, q0, a)
    return fma(r, y, q0)


def quot_pos(a, b, y):  # ort_core.h quot_pos
    q0 = a * y
    rn_ = fma(b, q0, -a)
    return fma(-rn_, y, q0)


def numerators(rng, n):
    return np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-300, 300, n)) * rng.choice([-1.0, 1.0], n)


def rsq_model(x, e0):
    """(1 + e0) / sqrt(x) rounded: sqrt to 120 bits past the quotient's."""
    f = Fraction(x)
    k = 200
    s = Fraction(math.isqrt(f.numerator * f.denominator << (2 * k)), f.denominator << k)
    return rn((1 + Fraction(e0)) / s)


def sqrt_seeded_h(x, y):
    """ort_core.h sqrt_seeded_h: the Goldschmidt sequence from the seed y -> (g, h)."""
    g = x * y
    h = y * 0.5
    r = fma(-h, g, 0.5)
    g = fma(g, r, g)
    h = fma(h, r, h)
    d = fma(-g, g, x)
    g = fma(d, h, g)
    d = fma(-g, g, x)
    g = fma(d, h, g)
    return g, h


def sqrt_h(x, e0):
    """ort_fastpath.h sqrt_h (the sequence seeded by the v_rsq model): -> (g, h)."""
    return sqrt_seeded_h(x, rsq_model(x, e0))
