// ort_sampled_otf.h -- one term of SampledMTF's overlap sum, shared by the HIP kernel
// (ort_k_sampled_otf.hip) and the host build (ort_host.cpp): the contribution of pupil point
// (x, y, I, opd) to the OTF at the shear (sx, sy), all in normalised pupil units,
//   mtf/sampled.py:170-196
//     P1 = sqrt(I) exp(i 2 pi opd), P2* = sqrt(I) exp(-i 2 pi W(x - sx, y - sy)),
//     P2* = 0 where r > 1, otf = sum P1 P2*
// with W the Zernike fit's polynomial (zernike/base.py:42-102) and the two exponentials
// folded into one sincos of a range-reduced argument:
//   xs = x - sx;  ys = y - sy;  r = sqrt(xs^2 + ys^2)       (each operation rounded, see below)
//   r > 1            -> term = 0                                   (mtf/sampled.py:190-193)
//   W  = sum_j c_j norm_j R_nj^|mj|(r) {cos | sin}(|mj| phi),  phi = atan2(ys, xs), term order
//   t  = opd - W                                                                (waves)
//   term = I (cos, sin)(2 pi (t - rint(t)))
//
// The mask has to agree with NumPy's bit for bit (a point that flips changes the sum by I,
// not by a rounding), so shear_radius forms r exactly as NumPy does: two rounded products, a
// rounded sum, a correctly rounded square root, never contracted; the comparison is r > 1.0,
// not r^2 > 1 (sqrt(1 + 2^-52) rounds to 1).
//
// W is evaluated as sagnorm_zernike (ort_core.h) evaluates a surface's term sum: cos phi, sin
// phi from polar_unit (r = 0 gives phi = 0, as arctan2(0, 0)), cos / sin(|m| phi) and r^|m| by
// the angle-addition recurrence, the radial polynomial by Horner in r^2 over the term's a_k.
// The term loop is written again here rather than factored out of sagnorm_zernike: that loop
// carries the surface's coefficient seeds, the normal's chain rule and dual numbers, and the
// trace kernels' instructions must stay what they are. Only the values are shared: the
// ort_zernike_term records and radial weights the Python side builds with
// geometries._zernike_structure (c is not read: the coefficients come per batch entry).
// The tables are wave-uniform and read through PZ / PD (the constant address space on the
// device: scalar loads); nothing is indexed per lane, so nothing goes to scratch.
//
// W and the phase do not keep NumPy's rounding (cos(m atan2) and libm powers cannot be
// bit-matched anyway), so the device build contracts a * b + c there; the error bound of
// DESIGN.md "Zernike fits and SampledMTF" covers both builds and the folding. No guards
// beyond the reference's: a masked point contributes exactly 0 whatever its data; an unmasked
// point with I = 0 and a finite opd contributes exactly 0; NaN data at an unmasked point gives
// NaN.
#pragma once

#include <math.h>

#include "ort_core.h"  // polar_unit, ort_zernike_term, ORT_SAMPLED_OTF_CHUNK

namespace ort {

// r of the sheared point, NumPy's operations: sqrt(xs * xs + ys * ys), nothing fused
ORT_INLINE double shear_radius(double xs, double ys) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double xx = xs * xs;
  const double yy = ys * ys;
  return ::sqrt(xx + yy);
}

// W(xs, ys) = sum_j coef[j] norm_j R_j(r) az_j(phi) in term order from 0.0
template <class PZ, class PD>
ORT_INLINE double zernike_poly(double xs, double ys, double r, PZ terms, PD radial, PD coef,
                               int n_terms) {
#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
  double c1, s1;
  polar_unit(xs, ys, r, c1, s1);
  const double r2 = r * r;
  double total = 0.0;
  for (int j = 0; j < n_terms; ++j) {
    const ort_zernike_term t = terms[j];
    const int am = t.m >= 0 ? t.m : -t.m;
    double cm = 1.0, sm = 0.0, pm = 1.0;  // cos(am phi), sin(am phi), r^am
#pragma unroll 1
    for (int q = 0; q < am; ++q) {
      const double cn = cm * c1 - sm * s1;
      sm = sm * c1 + cm * s1;
      cm = cn;
      pm = pm * r;
    }
    const PD a = radial + t.rad_off;
    double P = a[0];
#pragma unroll 1
    for (int k = 1; k < t.n_rad; ++k) P = P * r2 + a[k];
    const double az = t.m >= 0 ? cm : sm;  // base.py:242-258
    total = total + coef[j] * t.norm * (P * pm) * az;
  }
  return total;
}

template <class PZ, class PD>
ORT_INLINE void sampled_otf_term(double x, double y, double inten, double opd, double sx,
                                 double sy, PZ terms, PD radial, PD coef, int n_terms,
                                 double& re, double& im) {
  const double xs = x - sx, ys = y - sy;
  const double r = shear_radius(xs, ys);
  if (r > 1.0) {
    re = 0.0;
    im = 0.0;
    return;
  }
  const double t = opd - zernike_poly(xs, ys, r, terms, radial, coef, n_terms);  // waves
  const double phase = 6.283185307179586476925 * (t - ::rint(t));
  double s, c;
  ::sincos(phase, &s, &c);
  re = inten * c;
  im = inten * s;
}

// chunks of ORT_SAMPLED_OTF_CHUNK pupil points (an empty pupil: one empty chunk)
ORT_INLINE int64_t sampled_otf_chunks(int64_t n_pupil) {
  return n_pupil > 0 ? (n_pupil + ORT_SAMPLED_OTF_CHUNK - 1) / ORT_SAMPLED_OTF_CHUNK : 1;
}

}  // namespace ort
