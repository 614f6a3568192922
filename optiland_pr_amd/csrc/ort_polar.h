// ort_polar.h -- the per-ray polarization code shared by trace_kernel<F_POL>
// (ort_k_trace_pol.hip) and the host build (ort_host.cpp): the 3x3 complex polarization
// matrix of rays/polarized_rays.py, the Fresnel Jones diagonal of jones.py:90-117 and the
// intensity of PolarizedRays.update_intensity. Plain ORT_HD functions under
// -ffp-contract=off, so the host runs the kernel's operations.
//
// Reference files are cited as path:line under optiland/.
#pragma once

#include "ort_core.h"

namespace ort {

struct Cplx {
  double re, im;
};
ORT_INLINE Cplx cmul(const Cplx& a, const Cplx& b) {
  return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
ORT_INLINE Cplx cdiv(const Cplx& a, const Cplx& b) {
  const double d = b.re * b.re + b.im * b.im;
  return {(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}

// P[r][c] = re[3 r + c] + i im[3 r + c], the ray's initial direction k (the frame E0 is
// built in) and its initial intensity
struct PolState {
  double re[9], im[9];
  double kx, ky, kz, i0;
};

ORT_INLINE void pol_init(PolState& p, double L, double M, double N, double i0) {
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    p.re[e] = (e % 4 == 0) ? 1.0 : 0.0;
    p.im[e] = 0.0;
  }
  p.kx = L;
  p.ky = M;
  p.kz = N;
  p.i0 = i0;
}

// np.cross(a, b)
ORT_INLINE void cross3(double ax, double ay, double az, double bx, double by, double bz,
                       double& cx, double& cy, double& cz) {
  cx = ay * bz - az * by;
  cy = az * bx - ax * bz;
  cz = ax * by - ay * bx;
}

// jones.py:90-117 with cos(aoi) = d, sin^2(aoi) = 1 - d^2 (d = |n . k0| clipped to 1,
// coatings.py:82-84: arccos / cos / sin are not evaluated), n = n2 / n1 real
ORT_INLINE void jones_fresnel(double d, double n1, double n2, bool reflect, Cplx& js, Cplx& jp,
                              Cplx& jk) {
  if (d > 1.0) d = 1.0;
  const double n = n2 / n1;
  const double nsq = n * n;
  const double rad = nsq - (1.0 - d * d);
  Cplx root;  // the complex square root of a real radicand (NaN stays NaN)
  if (rad < 0.0) {
    root.re = 0.0;
    root.im = sqrt(-rad);
  } else {
    root.re = sqrt(rad);
    root.im = 0.0;
  }
  const Cplx ds = {d + root.re, root.im};
  const Cplx dp = {nsq * d + root.re, root.im};
  if (reflect) {
    js = cdiv({d - root.re, -root.im}, ds);
    const Cplx p = cdiv({nsq * d - root.re, -root.im}, dp);
    jp = {-p.re, -p.im};
    jk = {-1.0, 0.0};
  } else {
    js = cdiv({2.0 * d, 0.0}, ds);
    jp = cdiv({2.0 * n * d, 0.0}, dp);
    jk = {1.0, 0.0};
  }
}

// PolarizedRays.update (polarized_rays.py:110-151): k0 -> k1 at one surface with the Jones
// diagonal (js, jp, jk), as three rank-one terms
//   P <- s (js s^T P) + p1 (jp p0^T P) + k1 (jk k0^T P)
ORT_INLINE void pol_update(PolState& P, double k0x, double k0y, double k0z, double k1x,
                           double k1y, double k1z, const Cplx& js, const Cplx& jp,
                           const Cplx& jk) {
  double sx, sy, sz;
  cross3(k0x, k0y, k0z, k1x, k1y, k1z, sx, sy, sz);
  double mag = sqrt(sx * sx + sy * sy + sz * sz);
  if (mag == 0.0) {  // k0 parallel to k1 (:127-132)
    cross3(k0x, k0y, k0z, 1.0, 0.0, 0.0, sx, sy, sz);
    mag = sqrt(sx * sx + sy * sy + sz * sz);
  }
  sx = sx / mag;
  sy = sy / mag;
  sz = sz / mag;
  double p0x, p0y, p0z, p1x, p1y, p1z;
  cross3(k0x, k0y, k0z, sx, sy, sz, p0x, p0y, p0z);
  cross3(k1x, k1y, k1z, sx, sy, sz, p1x, p1y, p1z);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double r0 = P.re[c], r1 = P.re[3 + c], r2 = P.re[6 + c];
    const double i0 = P.im[c], i1 = P.im[3 + c], i2 = P.im[6 + c];
    // the brackets: a real 3-vector times the complex rows of P, then the Jones factor
    const Cplx a = cmul(js, {sx * r0 + sy * r1 + sz * r2, sx * i0 + sy * i1 + sz * i2});
    const Cplx b = cmul(jp, {p0x * r0 + p0y * r1 + p0z * r2, p0x * i0 + p0y * i1 + p0z * i2});
    const Cplx k = cmul(jk, {k0x * r0 + k0y * r1 + k0z * r2, k0x * i0 + k0y * i1 + k0z * i2});
    P.re[c] = sx * a.re + p1x * b.re + k1x * k.re;
    P.im[c] = sx * a.im + p1x * b.im + k1x * k.im;
    P.re[3 + c] = sy * a.re + p1y * b.re + k1y * k.re;
    P.im[3 + c] = sy * a.im + p1y * b.im + k1y * k.im;
    P.re[6 + c] = sz * a.re + p1z * b.re + k1z * k.re;
    P.im[6 + c] = sz * a.im + p1z * b.im + k1z * k.im;
  }
}

// One surface's coating after the refraction / reflection (interactions/base.py:112-128):
// none -> rays.update(), SIMPLE -> the intensity only (P untouched: coating.interact runs
// instead of rays.update), FRESNEL -> rays.update(jones). (nx, ny, nz): the surface normal
// as the geometry gave it; n1, n2: the coating's own materials at the ray's wavelength.
ORT_INLINE void pol_surface(PolState& P, const ort_coating& c, bool reflect, double nx,
                            double ny, double nz, double k0x, double k0y, double k0z,
                            double k1x, double k1y, double k1z, double n1, double n2,
                            double& inten) {
  if (c.kind == ORT_COAT_SIMPLE) {
    inten = inten * (reflect ? c.reflectance : c.transmittance);
    return;
  }
  Cplx js = {1.0, 0.0}, jp = {1.0, 0.0}, jk = {1.0, 0.0};
  if (c.kind == ORT_COAT_FRESNEL) {
    const double d = fabs(nx * k0x + ny * k0y + nz * k0z);  // coatings.py:82
    jones_fresnel(d, n1, n2, reflect, js, jp, jk);
  }
  pol_update(P, k0x, k0y, k0z, k1x, k1y, k1z, js, jp, jk);
}

// sum |P E|^2 for E = ex s + ey p (polarized_rays.py:56-78, :153-182)
ORT_INLINE double pol_power(const PolState& P, const Cplx& ex, const Cplx& ey, double sx,
                            double sy, double sz, double px, double py, double pz) {
  const Cplx e0 = {ex.re * sx + ey.re * px, ex.im * sx + ey.im * px};
  const Cplx e1 = {ex.re * sy + ey.re * py, ex.im * sy + ey.im * py};
  const Cplx e2 = {ex.re * sz + ey.re * pz, ex.im * sz + ey.im * pz};
  double sum = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const Cplx a = cmul({P.re[3 * r], P.im[3 * r]}, e0);
    const Cplx b = cmul({P.re[3 * r + 1], P.im[3 * r + 1]}, e1);
    const Cplx c = cmul({P.re[3 * r + 2], P.im[3 * r + 2]}, e2);
    const double re = a.re + b.re + c.re, im = a.im + b.im + c.im;
    sum = sum + (re * re + im * im);
  }
  return sum;
}

// PolarizedRays.update_intensity (polarized_rays.py:68-108): the stored intensity for
// `mode`, given the traced intensity (IGNORE / MATRICES keep it)
ORT_INLINE double pol_intensity(const PolState& P, int mode, const Cplx& ex, const Cplx& ey,
                                double traced) {
  if (mode != ORT_POL_POLARIZED && mode != ORT_POL_UNPOLARIZED) return traced;
  double px, py, pz, sx, sy, sz;
  cross3(P.kx, P.ky, P.kz, 1.0, 0.0, 0.0, px, py, pz);
  const double norm = sqrt(px * px + py * py + pz * pz);
  px = px / norm;
  py = py / norm;
  pz = pz / norm;
  cross3(px, py, pz, P.kx, P.ky, P.kz, sx, sy, sz);
  if (mode == ORT_POL_POLARIZED) return pol_power(P, ex, ey, sx, sy, sz, px, py, pz);
  const Cplx one = {1.0, 0.0}, zero = {0.0, 0.0};
  const double ix = pol_power(P, one, zero, sx, sy, sz, px, py, pz);
  const double iy = pol_power(P, zero, one, sx, sy, sz, px, py, pz);
  return (ix + iy) * P.i0 / 2.0;
}

}  // namespace ort
