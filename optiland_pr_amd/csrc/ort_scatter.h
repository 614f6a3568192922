// ort_scatter.h -- BSDF surface scattering (scatter.py:23-111) with a counter-based random
// stream, shared by trace_kernel<F_SCAT> (ort_k_trace_scat.hip), ort_bsdf_scatter and the
// host build (ort_host.cpp). Plain ORT_HD functions under -ffp-contract=off, so the host
// runs the kernel's operations.
//
// The reference draws from Numba's global generator inside `while True`; here every
// (ray, surface, attempt) owns one Philox4x32-10 block, so a ray draws the same numbers
// whatever the launch shape, the batch split (ort_scatter.ray_offset) or a verify round's
// re-trace:
//   key      (seed & 0xffffffff, seed >> 32)
//   counter  (ray & 0xffffffff, ray >> 32, surface_index, attempt)
//   u1 = (((o0 >> 5) << 26 | (o1 >> 6)) + 1) 2^-53, u2 likewise from o2, o3: in (0, 1],
//   exact in fp64.
//
// Reference files are cited as path:line under optiland/.
#pragma once

#include "ort_core.h"

namespace ort {

struct Philox {
  uint32_t o[4];
};

// Philox4x32-10 (Salmon et al., SC'11), the standard multipliers and key increments
ORT_INLINE Philox philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                             uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return {{c0, c1, c2, c3}};
}

// 53 bits of two output words as a double in (0, 1]
ORT_INLINE double philox_uniform(uint32_t hi, uint32_t lo) {
  const uint64_t m = (((uint64_t)(hi >> 5)) << 26) | (uint64_t)(lo >> 6);
  return (double)(m + 1) * 0x1p-53;
}

// the two uniforms of (seed, ray, surface, attempt)
ORT_INLINE void bsdf_uniforms(uint64_t seed, uint64_t ray, uint32_t surface, uint32_t attempt,
                              double& u1, double& u2) {
  const Philox p = philox4x32((uint32_t)ray, (uint32_t)(ray >> 32), surface, attempt,
                              (uint32_t)seed, (uint32_t)(seed >> 32));
  u1 = philox_uniform(p.o[0], p.o[1]);
  u2 = philox_uniform(p.o[2], p.o[3]);
}

// scatter.py:66-111 for one ray, in the surface's local frame: (L, M, N) the direction after
// the refraction / reflection, (nx, ny, nz) the geometry's raw normal (not the copy
// real_rays.py:511-547 aligns to the ray). The reference's own choices are kept:
//   the auxiliary vector is (1, 0, 0) unless the RAY's L >= 0.999 (scatter.py:89), so a
//   normal along it gives a = 0 / 0 = NaN;
//   a NaN radicand is not < 0, so a NaN ray leaves at attempt 0 with a NaN direction.
// The tangent frame and the ray's components in it do not depend on the draw and are formed
// once. Returns false when max_attempts draws all fell outside the unit disk (the direction
// is then NaN; the caller raises ORT_STATUS_SCATTER_ATTEMPTS).
ORT_INLINE bool bsdf_scatter(const ort_bsdf& f, uint64_t seed, uint64_t ray, uint32_t surface,
                             int32_t max_attempts, double nx, double ny, double nz, double& L,
                             double& M, double& N) {
  const double vx = L < 0.999 ? 1.0 : 0.0, vy = L < 0.999 ? 0.0 : 1.0, vz = 0.0;
  // a = cross(n, v) / |cross(n, v)|, b = cross(n, a)
  double ax = ny * vz - nz * vy;
  double ay = nz * vx - nx * vz;
  double az = nx * vy - ny * vx;
  const double an = sqrt(ax * ax + ay * ay + az * az);
  ax = ax / an;
  ay = ay / an;
  az = az / an;
  const double bx = ny * az - nz * ay;
  const double by = nz * ax - nx * az;
  const double bz = nx * ay - ny * ax;
  const double ra = L * ax + M * ay + N * az;
  const double rb = L * bx + M * by + N * bz;
  const double two_pi = 2.0 * 3.141592653589793;
  for (int32_t attempt = 0; attempt < max_attempts; ++attempt) {
    double u1, u2;
    bsdf_uniforms(seed, ray, surface, (uint32_t)attempt, u1, u2);
    const double theta = two_pi * u2;
    double px, py;
    if (f.kind == ORT_BSDF_GAUSSIAN) {  // scatter.py:38-54 (Box-Muller)
      const double rr = sqrt(-2.0 * ::log(u1));
      px = f.sigma * (rr * ::cos(theta));
      py = f.sigma * (rr * ::sin(theta));
    } else {  // scatter.py:23-35 (uniform on the unit disk)
      const double rr = sqrt(u1);
      px = rr * ::cos(theta);
      py = rr * ::sin(theta);
    }
    const double sx = ra + px;
    const double sy = rb + py;
    const double radicand = 1.0 - sx * sx - sy * sy;
    if (radicand < 0.0) continue;  // the wrong hemisphere: draw again
    const double sz = sqrt(radicand);
    L = sx * ax + sy * bx + sz * nx;
    M = sx * ay + sy * by + sz * ny;
    N = sx * az + sy * bz + sz * nz;
    return true;
  }
  L = M = N = __builtin_nan("");
  return false;
}

}  // namespace ort
