// ort_huygens.h -- one term of the Huygens-Fresnel diffraction sum, shared by the HIP
// kernel (ort_k_huygens.hip) and the host build (ort_host.cpp): the complex contribution of
// pupil point Q_j = (u, v, w) to image point P = (x, y, z),
//   psf/huygens_fresnel_strategies.py:124-166
//     wave = exp(i k R) / R, Q_obliq = (1 + cos theta) / 2, pupil_phase = exp(-i k opd_j),
//     sum += amp_j pupil_phase wave Q_obliq
// with the two exponentials folded into one sincos of a range-reduced argument:
//   dx, dy, dz = P - Q_j;  R = sqrt(dx^2 + dy^2 + dz^2)
//   cos theta  = (dx u + dy v + dz w) / (Rp R)             (the pupil normal is Q_j / Rp)
//   A          = amp_j (1 + cos theta) / (2 R)
//   phase      = 2 pi frac((R - opd_j) / lambda),  frac(t) = t - rint(t)  (in cycles)
//   term       = A (cos phase, sin phase)
// k R is ~1e6 rad: the reduction happens in cycles, in fp64, before the trigonometric call
// (fp32 anywhere in the phase is wrong). No guards beyond the reference's: R = 0 or a
// non-finite coordinate gives inf / NaN as the reference does; amp_j = 0 with finite
// coordinates contributes exactly 0.
//
// The callers pass 1 / lambda and 1 / Rp (formed once per call). This unit does not keep
// NumPy's rounding (exp cannot be bit-matched anyway), so the device build contracts
// a * b + c here; the error bound of DESIGN.md "Huygens-Fresnel PSF" covers both builds.
#pragma once

#include <math.h>

#include "../../include/optiland_rt.h"  // ORT_HUYGENS_CHUNK

#ifndef ORT_HD
#define ORT_HD __host__ __device__
#endif

namespace ort {

ORT_HD inline __attribute__((always_inline)) void huygens_term(
    double x, double y, double z, double u, double v, double w, double amp, double opd,
    double inv_wl, double inv_rp, double& re, double& im) {
#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
  const double dx = x - u, dy = y - v, dz = z - w;
  const double R = ::sqrt(dx * dx + dy * dy + dz * dz);
  const double inv_r = 1.0 / R;
  const double cos_t = (dx * u + dy * v + dz * w) * inv_rp * inv_r;
  const double A = amp * 0.5 * (1.0 + cos_t) * inv_r;
  const double t = (R - opd) * inv_wl;  // cycles
  const double phase = 6.283185307179586476925 * (t - ::rint(t));
  double s, c;
  ::sincos(phase, &s, &c);
  re = A * c;
  im = A * s;
}

// One image point against pupil points [j0, j1): the partial sum of one chunk, in index
// order from zero.
ORT_HD inline __attribute__((always_inline)) void huygens_chunk(
    double x, double y, double z, const double* px, const double* py, const double* pz,
    const double* amp, const double* opd, long long j0, long long j1, double inv_wl,
    double inv_rp, double& re, double& im) {
  double sr = 0.0, si = 0.0;
  for (long long j = j0; j < j1; ++j) {
    double tr, ti;
    huygens_term(x, y, z, px[j], py[j], pz[j], amp[j], opd[j], inv_wl, inv_rp, tr, ti);
    sr += tr;
    si += ti;
  }
  re = sr;
  im = si;
}

}  // namespace ort
