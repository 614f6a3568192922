// ort_dft.h -- the terms of the pupil-to-image transform of FFTPSF / MMDFTPSF / FFTMTF,
// shared by the HIP kernels (ort_k_dft.hip) and the host build (ort_host.cpp):
//   psf/mmdft.py:164-184, 230-290   G = L g R with the twiddle matrices L, R
//   psf/fft.py:169-234              fftshift(fft2(padded pupil)): the same |G|^2 with
//                                   pad = image size = grid size
//   g[j,k]   = amp[j,k] exp(-2 pi i opd[j,k])                                 (dft_pupil)
//   W(a, b)  = exp(-2 pi i a b / pad), a = v - m/2 (or u - m/2), b = j - n/2 (or k - n/2),
//              integer divisions                                               (dft_twiddle)
//   out[v,u] = |sum_j W(v - m/2, j - n/2) sum_k g[j,k] W(u - m/2, k - n/2)|^2
// Every phase is reduced in cycles, in fp64, before the sincos: frac(t) = t - rint(t) (exact),
// as ort_huygens.h does. The product a b is an exact integer; when pad is an integer it is
// first reduced mod pad (exact as well), so such a twiddle's only roundings are the division,
// the multiplication by 2 pi and the sincos. amp == 0 with a finite opd gives exactly 0;
// a non-finite input gives NaN.
//
// The sums run from zero in index order: per row j over k (stage A, T = g R), then per output
// over j (stage B, |R^T T|^2); dft_mac is one step of either. This unit keeps no NumPy
// rounding (exp cannot be bit-matched), so the device build contracts a * b + c here as
// ort_huygens.h does; the bound of DESIGN.md "FFT / MMDFT PSF and MTF" covers both builds.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/optiland_rt.h"  // ORT_DFT_TILE_M, ORT_DFT_TILE_K

#ifndef ORT_HD
#define ORT_HD __host__ __device__
#endif

namespace ort {

constexpr double kDftTwoPi = 6.283185307179586476925;

// pad as an integer modulus when it is one (0 otherwise: no reduction of a b)
ORT_HD inline int64_t dft_int_pad(double pad) {
  return (pad >= 1.0 && pad <= 2147483648.0 && pad == ::rint(pad)) ? (int64_t)pad : 0;
}

ORT_HD inline __attribute__((always_inline)) void dft_pupil(double amp, double opd, double& re,
                                                            double& im) {
  const double phase = -kDftTwoPi * (opd - ::rint(opd));
  double s, c;
  ::sincos(phase, &s, &c);
  re = amp * c;
  im = amp * s;
}

ORT_HD inline __attribute__((always_inline)) void dft_twiddle(int64_t a, int64_t b, double pad,
                                                              int64_t ipad, double& re,
                                                              double& im) {
  int64_t p = a * b;
  if (ipad > 0) p %= ipad;
  const double t = (double)p / pad;  // cycles
  const double phase = -kDftTwoPi * (t - ::rint(t));
  double s, c;
  ::sincos(phase, &s, &c);
  re = c;
  im = s;
}

// (sr, si) += (ar, ai) (br, bi)
ORT_HD inline __attribute__((always_inline)) void dft_mac(double ar, double ai, double br,
                                                          double bi, double& sr, double& si) {
#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
  sr = sr + (ar * br - ai * bi);
  si = si + (ar * bi + ai * br);
}

}  // namespace ort
