// ort_irradiance.h -- the per-ray pieces of IncoherentIrradiance's binning
// (analysis/irradiance.py:243-330), shared by the HIP kernels (ort_k_irradiance.hip) and the
// host build (ort_host.cpp): which pixel(s) a ray lands in, what it contributes, how a
// contribution becomes a 64-bit fixed-point integer and how a pixel's integer sum becomes
// W/mm^2. Everything here is +, -, *, /, comparisons, rint and exact scaling by powers of
// two, compiled without contraction on both sides, so host and device agree to the bit.
//
// ORT_BIN_HISTOGRAM (numpy.histogram2d(x, y, bins=[x_edges, y_edges], weights=power) after
//   the reference's power > 0 filter): the pixel along one axis is
//   searchsorted(edges, v, side='right') - 1, a value equal to the last edge goes to the
//   last bin, values outside [e[0], e[nb]] and NaN are dropped. Output index ix * ny + iy.
// ORT_BIN_BILINEAR (backend/torch_backend.py:548-599 get_bilinear_weights, then four
//   index_put(accumulate=True)): cells between pixel centres c[j] = (e[j] + e[j+1]) / 2,
//   ix = clamp(searchsorted(c, x, right=True) - 1, 0, nc - 2), wx = (x - c[ix]) /
//   (c[ix+1] - c[ix] + 1e-9), the four weights in the reference's order w00, w01, w10, w11
//   on pixels (ix, iy), (ix, iy+1), (ix+1, iy), (ix+1, iy+1). Output index iy * nx + ix.
//
// The index along an axis starts from a multiply-and-floor guess and is then corrected
// against the stored points (one step either way; a binary search when the guess is further
// off), so it is exact for any strictly increasing edge array.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/optiland_rt.h"

#ifndef ORT_HD
#define ORT_HD __host__ __device__
#endif

namespace ort {

struct IrrEdges {  // the points of an axis are its edges
  const double* e;
  ORT_HD double operator()(int64_t j) const { return e[j]; }
};

struct IrrCentres {  // the points of an axis are its pixel centres
  const double* e;
  ORT_HD double operator()(int64_t j) const { return (e[j] + e[j + 1]) / 2.0; }
};

// searchsorted(points, v, side='right') - 1 over nn >= 2 strictly increasing points: the
// last j with points[j] <= v; -1 below the first point, nn - 1 from the last point on and
// for NaN (which sorts past the end).
template <class P>
ORT_HD inline int64_t irr_index(const P& pt, int64_t nn, double v) {
  const double first = pt(0), last = pt(nn - 1);
  if (!(v >= first)) return v != v ? nn - 1 : -1;
  if (v >= last) return nn - 1;
  // first <= v < last: the answer is in [0, nn - 2]
  const double t = (v - first) * ((double)(nn - 1) / (last - first));
  int64_t k = t < (double)(nn - 2) ? (int64_t)t : nn - 2;
  if (v < pt(k)) {  // (k > 0 here: v >= pt(0))
    --k;
    if (!(v < pt(k))) return k;
  } else if (v >= pt(k + 1)) {  // (k + 1 < nn - 1 here: v < pt(nn - 1))
    ++k;
    if (!(v >= pt(k + 1))) return k;
  } else {
    return k;
  }
  int64_t lo = 0, hi = nn;  // first index with pt > v
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (pt(mid) > v) hi = mid; else lo = mid + 1;
  }
  return lo - 1;
}

// histogram bin along one axis of nb bins, -1: dropped
ORT_HD inline int64_t irr_bin(const double* e, int64_t nb, double v) {
  if (!(v >= e[0] && v <= e[nb])) return -1;
  const int64_t k = irr_index(IrrEdges{e}, nb + 1, v);
  return k == nb ? nb - 1 : k;
}

// bilinear cell along one axis of nb >= 2 pixels: the index of the lower centre, the weight
// of the upper one and the weight's derivative with respect to v
ORT_HD inline int64_t irr_cell(const double* e, int64_t nb, double v, double& w, double& dw) {
  const IrrCentres c{e};
  int64_t k = irr_index(c, nb, v);
  k = k < 0 ? 0 : (k > nb - 2 ? nb - 2 : k);
  const double c0 = c(k), c1 = c(k + 1);
  const double den = c1 - c0 + 1e-9;
  w = (v - c0) / den;
  dw = 1.0 / den;
  return k;
}

struct IrrGrid {
  const double* x_edges;
  const double* y_edges;
  int64_t nx, ny;
  int32_t mode;
};

// The contributions of one ray: pixel indices and values; returns how many (0, 1 or 4).
ORT_HD inline int irr_contributions(const IrrGrid& g, double x, double y, double p,
                                    int64_t pix[4], double c[4]) {
  if (g.mode == ORT_BIN_HISTOGRAM) {
    if (!(p > 0.0)) return 0;
    const int64_t ix = irr_bin(g.x_edges, g.nx, x);
    if (ix < 0) return 0;
    const int64_t iy = irr_bin(g.y_edges, g.ny, y);
    if (iy < 0) return 0;
    pix[0] = ix * g.ny + iy;
    c[0] = p;
    return 1;
  }
  double wx, wy, dwx, dwy;
  const int64_t ix = irr_cell(g.x_edges, g.nx, x, wx, dwx);
  const int64_t iy = irr_cell(g.y_edges, g.ny, y, wy, dwy);
  const double ux = 1.0 - wx, uy = 1.0 - wy;
  pix[0] = iy * g.nx + ix;
  pix[1] = pix[0] + g.nx;
  pix[2] = pix[0] + 1;
  pix[3] = pix[1] + 1;
  c[0] = ux * uy * p;
  c[1] = ux * wy * p;
  c[2] = wx * uy * p;
  c[3] = wx * wy * p;
  return 4;
}

ORT_HD inline bool irr_finite(double c) { return c - c == 0.0; }

// |c| as an integer that orders as the value does (finite c)
ORT_HD inline uint64_t irr_abs_bits(double c) {
  union { double d; uint64_t u; } v;
  v.d = c;
  return v.u & 0x7fffffffffffffffULL;
}

// ORT_IRRADIANCE_EXPONENT (optiland_rt.h): E = 62 - ec - L with cmax = m 2^ec, 0.5 <= m < 1,
// and L = log2_n = the least L with 2^L >= n; E = 0 when there is no positive cmax.
ORT_HD inline int irr_exponent(uint64_t cmax_bits, int log2_n) {
  if (cmax_bits == 0) return 0;
  union { double d; uint64_t u; } v;
  v.u = cmax_bits;
  int ec;
  (void)::frexp(v.d, &ec);
  return 62 - ec - log2_n;
}

inline int irr_log2_ceil(int64_t n) {
  int L = 0;
  while (L < 62 && ((int64_t)1 << L) < n) ++L;
  return L;
}

// a finite contribution |c| <= cmax in units of 2^-E, rounded to nearest (ties to even) once
ORT_HD inline int64_t irr_quantise(double c, int E) { return (int64_t)::rint(::ldexp(c, E)); }

// the pixel area the sums are divided by: the caller's, or (pixel_area <= 0) the first pixel's
ORT_HD inline double irr_area(const IrrGrid& g, double pixel_area) {
  if (pixel_area > 0.0) return pixel_area;
  return (g.x_edges[1] - g.x_edges[0]) * (g.y_edges[1] - g.y_edges[0]);
}

// a pixel's integer sum as irradiance: one rounding to fp64, exact scaling, / area
ORT_HD inline double irr_finish(int64_t sum, uint32_t flag, int E, double area) {
  if (flag) return NAN;
  return ::ldexp((double)sum, -E) / area;
}

// ORT_BIN_BILINEAR's backward for one ray: G is the upstream gradient image [ny][nx]. The
// clamped indices are piecewise constant (zero derivative, as in torch).
ORT_HD inline void irr_vjp(const IrrGrid& g, const double* G, double x, double y, double p,
                           double area, double& gx, double& gy, double& gp) {
  double wx, wy, dwx, dwy;
  const int64_t ix = irr_cell(g.x_edges, g.nx, x, wx, dwx);
  const int64_t iy = irr_cell(g.y_edges, g.ny, y, wy, dwy);
  const double* q = G + iy * g.nx + ix;
  const double g00 = q[0], g01 = q[g.nx], g10 = q[1], g11 = q[g.nx + 1];
  const double ux = 1.0 - wx, uy = 1.0 - wy;
  gp = (ux * uy * g00 + ux * wy * g01 + wx * uy * g10 + wx * wy * g11) / area;
  gx = p * dwx * ((g10 - g00) * uy + (g11 - g01) * wy) / area;
  gy = p * dwy * ((g01 - g00) * ux + (g11 - g10) * wx) / area;
}

}  // namespace ort
