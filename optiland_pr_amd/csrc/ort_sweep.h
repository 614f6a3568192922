// ort_sweep.h -- the two derivative sweeps of the trace, shared by the HIP kernels and the
// host build:
//
//   adj_ray  the reverse-mode (adjoint) VJP of one ray (ort_trace_*_vjp, ORT_VJP_ADJOINT);
//   vjp_ray  the forward-mode (dual number) VJP of one ray (ORT_VJP_UNROLLED).
//
// Plain per-ray C++ (ORT_HD: __host__ __device__ under hipcc, plain functions under g++).
// Their argument blocks (KArgs, AArgs, JArgs), the frame changes, table lookups and slot
// helpers they use, and the front end that fills the blocks from the C ABI structs are in
// ort_args.h; only the units that differentiate include this file (ort_adjoint.h, which
// the ort_k_adj*.hip and ort_k_vjp*.hip units and ort_api.hip include, and ort_host.cpp).
//
// The GPU kernels (ort_adjoint.h adj_kernel and vjp_kernel) run the sweeps one
// ray per lane; the host library (ort_host.cpp: the CPU dispatch key of the torch custom
// ops) runs them one ray per loop iteration. What differs between the two is behind a small
// "lane" policy object: where a per-ray contribution to a parameter slot goes (a wave sum
// into partial[slot][wave] on the device, a per-chunk accumulator on the host), where the
// adjoint tape lives (HBM rows [S][11][n_rays] on the device, a per-ray scratch array on
// the host) and how a wave-uniform loop bound is formed. The arithmetic is the same source,
// so the host gradients follow the GPU's operation for operation (the reductions over rays
// run in a different fixed order).
//
// Reference files are cited as path:line under optiland/.
#pragma once

#include "ort_args.h"

namespace ortk {

// =====================================================================================
// Reverse-mode (adjoint) VJP of one ray.
//
// The forward-mode VJP (vjp_ray) re-traces the lens once per chunk of P parameter
// tangents, so its cost grows with the number of parameters. The adjoint computes the
// same vector-Jacobian product in one sweep whatever the parameter count:
//
//   forward   the primal trace in double (same code, same values as ort_trace_pupil),
//             taping each traced surface's incoming global ray (x, y, z, L, M, N), its
//             intersection distance t and (Newton surfaces) the iterates before the
//             last kHist updates;
//   reverse   from the image back to the first surface, the adjoint of every step of
//             Surface.trace (standard_surface.py:186-233): globalize, refract / reflect
//             with the aligned normal, the normal at the hit point, OPD and absorption,
//             propagation, the intersection distance, localize.
//
// Closed-form intersections (plane, conic) are differentiated through their implicit
// equations (the derivative of the closed form, up to rounding). Newton intersections
// are differentiated like torch autograd does it, through the unrolled updates
// t' = t - f(t) / f'(t) (newton_raphson.py:137-166) -- not through the converged root:
// the last update starts ~sqrt(tol) from the root, so the two differ at the 1e-5 level.
// The reverse sweep replays the last kHist updates from taped iterates and then the
// conic initial guess; with more updates the earliest are dropped (their share is
// scaled by products of converged residuals). The standard / noll Zernike normal omits
// the normalisation constant, so its Newton slope is not the sag's derivative and the
// iteration converges linearly: on those surfaces (ORT_SURF_SLOPE_INEXACT) the sweep is
// exact while U <= kHist (every iterate taped), and the host takes the forward-mode VJP
// for a longer schedule (autodiff.vjp_mode).
//
// Local derivatives of the surface at the hit point (normal and sag w.r.t. x, y and,
// with P = 4, the radius and conic) come from one forward-mode evaluation with dual
// numbers seeded on those inputs; the Zernike coefficients from one transposed pass
// over the terms (ort::zernike_coef_adjoint). Each per-ray contribution to a parameter
// "slot" (radius / conic / vertex z of each surface, each Zernike term, the image-space
// propagation distance) goes to lane.emit(slot, v, first); the per-parameter gradient is
// the sum over rays of its slots weighted by the tangent tables (slot_weight).
// =====================================================================================

// adjoint of a coordinate-system op: rotations transpose (sin -> -sin), translations
// are constant offsets (identity on the adjoint)
ORT_INLINE void adj_cs_op(ort::Ray& b, const ort_cs_op& op) {
  if (op.kind == ORT_CS_TRANSLATE) return;
  ort_cs_op t = op;
  t.p[1] = -op.p[1];
  ort::apply_cs_op(b, t);
}

// Distance along the ray to surface s in its local frame, as the primal computes it
// (ort_trace_pupil with ORT_NEWTON_SCHEDULE: exactly sched[group][si] Newton updates),
// keeping the iterates before the last kHist updates: hist[m] = t_{U-1-m}.
template <uint32_t KM>
ORT_INLINE double replay_distance(const KArgs& a, const ort_surface& s, int si,
                                  const ort::Ray& r, int64_t group, double (&hist)[kHist]) {
#pragma unroll
  for (int h = 0; h < kHist; ++h) hist[h] = 0.0;
  if (s.geometry == ORT_GEOM_PLANE) return ort::distance_plane(r);
  double t = ort::distance_conic(r, s.radius, s.conic, (s.flags & ORT_SURF_RADIUS_INF) != 0);
  if (s.geometry == ORT_GEOM_STANDARD) return t;
  if constexpr (KM != 0) {
    const int U = a.sched ? a.sched[group * a.n_surf + si] : s.max_iter;
    bool rerr = false;
    for (int it = 0; it < U; ++it) {
#pragma unroll
      for (int h = kHist - 1; h > 0; --h) hist[h] = hist[h - 1];
      hist[0] = t;
      double nx, ny, nz;
      const double f = ort::newton_eval<KM>(s, s.radius, s.conic, cst(a.coef), cst(a.zern),
                                            kNoSeed, r, t, ort::kSlope, rerr, nx, ny, nz);
      t = ort::newton_step_any(r, t, f, nx, ny, nz);
    }
  }
  return t;
}

// One evaluation's Zernike coefficient adjoint in the monomial basis of a degree-N block
// (see AArgs.n_mono): at the normalised point (xn, yn) the sag's weight ws adds ws m_k to
// S_k (SAG; without it -- the hit point, where the sag has no adjoint -- the S slots are
// left alone) and the slopes' weights (ax, ay) -- the adjoint of the block gradient
// (Gx, Gy) the Cartesian normal is formed from -- add ax dm_k/dxn + ay dm_k/dyn to D_k;
// handed to the lane value by value (mono_put(base, i, v): slot base + i, i counting from
// 0), then mono_flush(base, n)
template <int N, bool SAG, class Lane>
ORT_INLINE void zmono_adjoint(Lane& ln, int slot0, double xn, double yn, double ws, double ax,
                              double ay) {
  constexpr int K = (N + 1) * (N + 2) / 2;
  double xp[N + 1], yp[N + 1];
  xp[0] = yp[0] = 1.0;
#pragma unroll
  for (int p = 1; p <= N; ++p) {
    xp[p] = xp[p - 1] * xn;
    yp[p] = yp[p - 1] * yn;
  }
  const int base = SAG ? slot0 : slot0 + K;
  int i = 0;
  if constexpr (SAG) {
#pragma unroll
    for (int p = 0; p <= N; ++p) {
#pragma unroll
      for (int q = 0; q <= N - p; ++q) ln.mono_put(base, i++, ws * (xp[p] * yp[q]));
    }
  }
#pragma unroll
  for (int p = 0; p <= N; ++p) {
#pragma unroll
    for (int q = 0; q <= N - p; ++q) {
      double d = 0.0;
      if (p > 0) d = ax * ((double)p * (xp[p - 1] * yp[q]));
      if (q > 0) d = d + ay * ((double)q * (xp[p] * yp[q - 1]));
      ln.mono_put(base, i++, d);
    }
  }
  ln.mono_flush(base, i);
}

template <bool SAG, class Lane>
ORT_INLINE void zmono_adjoint_deg(Lane& ln, int deg, int slot0, double xn, double yn, double ws,
                                  double ax, double ay) {
  switch (deg) {
    case 0: zmono_adjoint<0, SAG>(ln, slot0, xn, yn, ws, ax, ay); break;
    case 1: zmono_adjoint<1, SAG>(ln, slot0, xn, yn, ws, ax, ay); break;
    case 2: zmono_adjoint<2, SAG>(ln, slot0, xn, yn, ws, ax, ay); break;
    case 3: zmono_adjoint<3, SAG>(ln, slot0, xn, yn, ws, ax, ay); break;
    case 4: zmono_adjoint<4, SAG>(ln, slot0, xn, yn, ws, ax, ay); break;
    case 5: zmono_adjoint<5, SAG>(ln, slot0, xn, yn, ws, ax, ay); break;
    case 6: zmono_adjoint<6, SAG>(ln, slot0, xn, yn, ws, ax, ay); break;
    default:  // unreachable (mono_slots gives such a surface no monomial slots): never
              // another degree's layout -- a NaN in the surface's first slot instead
      ln.mono_put(slot0, 0, __builtin_nan(""));
      ln.mono_flush(slot0, 1);
      break;
  }
}

// The lane policy (Lane) adj_ray is written against:
//   void   emit(int slot, double v, bool first)  add the ray's v to parameter slot `slot`
//                                                 (first: the slot's first contribution
//                                                 from this ray / wave)
//   double* tape_at(int64_t row)                  this ray's entry of tape row `row`
//   int64_t tape_stride()                         distance between two tape rows
//   int    uniform_max(int v)                     max over the rays sharing control flow
//   void   mono_put(int slot0, int i, double v), mono_flush(int slot0, int n)
//                                                 one evaluation's monomial-basis values,
//                                                 v to slot slot0 + i (zmono_adjoint)
// RES = false: rays generated from pupil samples (ort_trace_pupil_vjp);
// RES = true: resident input rays a.in (ort_trace_sequential_vjp, SurfaceGroup.trace under
// autograd), optionally with per-ray wavelengths (a.w), and the cotangents of the input
// rays written to j.gin. The forward then runs with i = 1, so intensity(r) is the factor
// d i_out / d i_in (0 when clipped, exp(att) otherwise; i_in times it is the primal's
// intensity, operation for operation).
template <uint32_t KM, int P, bool RES, class Lane>
ORT_INLINE void adj_ray(const KArgs& a, const AArgs& j, Lane& ln, int64_t rid, bool active) {
  using D = ort::Dual<P>;
  const int64_t r_ld = active ? rid : 0;
  const int64_t NR = a.n_rays;
  const int64_t TS = ln.tape_stride();
  const int64_t sidx = (RES && !a.seg) ? 0 : r_ld / a.seg_len;
  int lam = 0;
  double wl = 0.0, i_in = 1.0;
  ort::Ray r;
  if constexpr (RES) {
    if (a.seg) lam = a.seg[sidx].lambda_idx;
    if (a.w) wl = a.w[r_ld];
    r.x = a.in.x[r_ld];
    r.y = a.in.y[r_ld];
    r.z = a.in.z[r_ld];
    r.L = a.in.L[r_ld];
    r.M = a.in.M[r_ld];
    r.N = a.in.N[r_ld];
    i_in = a.in.i[r_ld];
    r.i = 1.0;
    r.opd = a.in.opd[r_ld];
    r.att = 0.0;
  } else {
    const ort_segment sg = a.seg[sidx];
    lam = sg.lambda_idx;
    const int64_t p = a.pupil_per_ray ? r_ld : (r_ld - sidx * a.seg_len);
    r = ort::generate_ray(sg, a.px[p], a.py[p], a.apod);
  }
  const int64_t group = r_ld / a.group_len;
  // optical constants of surface si at this ray's wavelength (table row, or per ray)
  auto optics_of = [&](const ort_surface& s, int si) -> ort_surface_optics {
    if constexpr (RES) {
      if (a.w) return optics_ray(a, s, wl);
    }
    return optics_row(a, lam, si);
  };

  // sag and normal of surface s at local (x, y) as duals (sag only for Newton kinds)
  auto sagnorm = [&](const ort_surface& s, double x, double y, D& nx, D& ny, D& nz) -> D {
    D X(x), Y(y);
    X.d[0] = 1.0;
    Y.d[1] = 1.0;
    if (s.geometry == ORT_GEOM_PLANE) {
      nx = D(0.0);
      ny = D(0.0);
      nz = D(1.0);
      return D(0.0);
    }
    if (s.geometry == ORT_GEOM_STANDARD) {
      if (s.flags & ORT_SURF_RADIUS_INF) {  // standard.py with R = inf: (0, 0, -1)
        nx = D(0.0);
        ny = D(0.0);
        nz = D(-1.0);
      } else if constexpr (P == 4) {
        D Rd(s.radius), Kd(s.conic);
        Rd.d[2] = 1.0;
        Kd.d[3] = 1.0;
        ort::normal_conic(X, Y, Rd, Kd, nx, ny, nz);
      } else {
        ort::normal_conic(X, Y, s.radius, s.conic, nx, ny, nz);
      }
      return D(0.0);
    }
    bool rerr = false;
    if constexpr (P == 2 && (KM & ort::KM_ZERN) != 0) {
      // Zernike: the plain-double second-order model (ort::zernike_jet) instead of the
      // dual-number evaluation -- the same derivatives, a fraction of the registers
      if (KM == ort::KM_ZERN || s.geometry == ORT_GEOM_ZERNIKE) {
        ort::SurfJet J;
        ort::zernike_jet(x, y, s.radius, s.conic, s.norm_radius, cst(a.zern), s.coef_off,
                         s.n_coef, cst(a.coef), J, s.zm_off, s.zm_deg);
        ort::jet_normal(J, nx, ny, nz);
        D z(J.z);
        z.d[0] = J.zx;
        z.d[1] = J.zy;
        return z;
      }
    }
    if constexpr (KM == 0) {
      nx = ny = nz = D(__builtin_nan(""));
      return D(__builtin_nan(""));
    } else if constexpr (P == 4) {
      D Rd(s.radius), Kd(s.conic);
      Rd.d[2] = 1.0;
      Kd.d[3] = 1.0;
      return ort::newton_sagnorm<KM>(s, Rd, Kd, cst(a.coef), cst(a.zern), kNoSeed, X, Y, true,
                                     rerr, nx, ny, nz);
    } else {
      return ort::newton_sagnorm<KM>(s, s.radius, s.conic, cst(a.coef), cst(a.zern), kNoSeed,
                                     X, Y, true, rerr, nx, ny, nz);
    }
  };

  // monomial-basis coefficient slots (AArgs.n_mono): the current surface's first slot
  // (mono_base, -1: per-term slots), walking back from the end of the slot table
  int mono_base = -1;
  int mono_end = 3 * a.n_surf + j.n_zern + 1 + (j.mono_on ? j.n_mono : 0);

  // Zernike coefficients at local (x, y): w_sag * d sag / d c plus the slopes' share of
  // the normal's adjoint bn (n = (dzdx, dzdy, -1) / q, q = -1 / nz)
  auto zern_adj = [&](const ort_surface& s, bool on, bool first, double x, double y,
                      double w_sag, double bnx, double bny, double bnz, double nxv,
                      double nyv, double nzv) {
    if constexpr ((KM & ort::KM_ZERN) != 0) {
      if (s.geometry == ORT_GEOM_ZERNIKE && j.zparam) {
        const double bn = bnx * nxv + bny * nyv + bnz * nzv;
        const double bdx = -nzv * (bnx - nxv * bn);
        const double bdy = -nzv * (bny - nyv * bn);
        if (mono_base >= 0) {
          // the Cartesian normal's slopes (sagnorm_zernike): their adjoints (bdx, bdy)
          // pulled back to the block gradient (Gx, Gy) (derivative-only quotients: rdiv)
          const double inv_rn = ort::rrcp(s.norm_radius);
          const double xn = x * inv_rn, yn = y * inv_rn;
          // sagnorm_zernike's slopes: Gx / Rn, Gy / Rn off the disc rho^2 < kZernChainRho2
          // (their adjoint: (bdx, bdy) / Rn), the reference's chain on it
          const double rho2n = xn * xn + yn * yn;
          double ax, ay;
          if (rho2n >= ort::kZernChainRho2) {
            ax = bdx * inv_rn;
            ay = bdy * inv_rn;
          } else {
            const double eps = 1e-14;
            const double rho = sqrt(rho2n);
            const double ire = ort::rrcp(rho + eps), iq = ort::rrcp(rho * rho + eps);
            const double drx = xn * inv_rn * ire, dry = yn * inv_rn * ire;
            const double qy = -(yn)*iq, qx = xn * iq;
            double cx = 0.0, cy = 0.0;  // xn / rho, yn / rho (Fr's factors)
            if (rho > 0.0) {
              const double ir = ort::rrcp(rho);
              cx = xn * ir;
              cy = yn * ir;
            }
            const double fr = bdx * drx + bdy * dry;        // adjoint of Fr
            const double g2 = (bdx * qy + bdy * qx) * inv_rn;  // adjoint of G2
            ax = fr * cx - g2 * yn;
            ay = fr * cy + g2 * xn;
          }
          const double wx = on ? ax : 0.0, wy = on ? ay : 0.0;
          if (first)  // the hit point: the normal only (w_sag == 0)
            zmono_adjoint_deg<false>(ln, s.zm_deg, mono_base, xn, yn, 0.0, wx, wy);
          else
            zmono_adjoint_deg<true>(ln, s.zm_deg, mono_base, xn, yn, on ? w_sag : 0.0, wx, wy);
          return;
        }
        const int base = 3 * a.n_surf;
        ort::zernike_coef_adjoint(x, y, s.norm_radius, cst(a.zern), s.coef_off, s.n_coef,
                                  cst(a.coef), w_sag, bdx, bdy,
                                  [&](int term, double g) {
                                    ln.emit(base + term, on ? g : 0.0, first);
                                  });
      }
    }
  };

  // distance of the closed forms through their implicit equations: plane / flat conic
  // F = -z (plane.py:61-77), conic x^2 + y^2 + (1 + k) z^2 - 2 R z = 0
  // (standard.py:89-140); tb = adjoint of t, at the point q + t D
  auto closed_adj = [&](const ort_surface& s, const ort::Ray& q, double t, double tb,
                        ort::Ray& b, double& bR, double& bk) {
    const double x = q.x + t * q.L, y = q.y + t * q.M, z = q.z + t * q.N;
    double Gx = 0.0, Gy = 0.0, Gz = -1.0, GR = 0.0, Gk = 0.0;
    if (s.geometry != ORT_GEOM_PLANE && !(s.flags & ORT_SURF_RADIUS_INF)) {
      Gx = 2.0 * x;
      Gy = 2.0 * y;
      Gz = 2.0 * (1.0 + s.conic) * z - 2.0 * s.radius;
      GR = -2.0 * z;
      Gk = z * z;
    }
    const double lm = ort::rdiv(-tb, Gx * q.L + Gy * q.M + Gz * q.N);
    b.x += lm * Gx;
    b.y += lm * Gy;
    b.z += lm * Gz;
    b.L += lm * t * Gx;
    b.M += lm * t * Gy;
    b.N += lm * t * Gz;
    bR += lm * GR;
    bk += lm * Gk;
  };

  // ---- forward: the primal trace, taping (incoming ray, t, Newton iterates) per surface;
  // skipped when the primal launch wrote the tape itself (F_TAPE, tape_ready): the final
  // state is then that launch's output (the same values, operation for operation)
  double gi = 0.0;  // RES: d (recorded intensities) / d i_in, contracted with rec_cot
  bool replay = true;
  if constexpr (!RES) replay = !j.tape_ready;
  if (replay) {
    int64_t trow = tape_row0(a.surf, a.start_surface);
    for (int si = a.start_surface; si < a.n_surf; ++si) {
      const ort_surface s = cst(a.surf)[si];
      const ort_surface_optics o = optics_of(s, si);
      double* tp = ln.tape_at(trow);
      trow += tape_rows(s);
      if (active) {
        tp[0] = r.x;
        tp[TS] = r.y;
        tp[2 * TS] = r.z;
        tp[3 * TS] = r.L;
        tp[4 * TS] = r.M;
        tp[5 * TS] = r.N;
      }
      localize(a, s, r);
      double hist[kHist];
      const double t = replay_distance<KM>(a, s, si, r, group, hist);
      if (active) {
        tp[6 * TS] = t;
        if (s.geometry != ORT_GEOM_PLANE && s.geometry != ORT_GEOM_STANDARD) {
#pragma unroll
          for (int h = 0; h < kHist; ++h) tp[(7 + h) * TS] = hist[h];
        }
      }
      ort::finish_surface<KM>(r, s, s.radius, s.conic, cst(a.coef), cst(a.zern), kNoSeed, t,
                              o.n_pre, o.u, o.alpha_pre);
      globalize(a, s, r);
      if constexpr (RES) {
        if (j.rec_cot && (s.flags & ORT_SURF_RECORD) && active)
          gi += j.rec_cot[((int64_t)s.rec_slot * 8 + 6) * NR + rid] * ort::intensity(r);
      }
    }
  } else {
    r.L = j.primal.L[r_ld];
    r.M = j.primal.M[r_ld];
    r.N = j.primal.N[r_ld];
    r.i = j.primal.i[r_ld];  // the stored intensity: i exp(att), apodization included
    r.att = 0.0;
  }
  double alpha_f = 0.0;
  if (a.final_mat >= 0) {
    if (RES && a.w)
      alpha_f = ort::absorption_alpha(ort::material_k(cst(a.mats)[a.final_mat], a.coef, wl), wl);
    else
      alpha_f = tab(a.alpha_tab, a.n_lambda, a.n_mat, lam, a.final_mat);
    if (replay) ort::propagate(r, a.final_thickness, alpha_f);
  }

  // ---- output cotangents (intensity = i exp(att): d/d att = intensity)
  ort::Ray b;
  b.x = b.y = b.z = b.L = b.M = b.N = 0.0;
  b.i = b.opd = b.att = 0.0;
  double bopd = 0.0, batt = 0.0;
  if (active) {
    if (j.cot.x) b.x = j.cot.x[rid];
    if (j.cot.y) b.y = j.cot.y[rid];
    if (j.cot.z) b.z = j.cot.z[rid];
    if (j.cot.L) b.L = j.cot.L[rid];
    if (j.cot.M) b.M = j.cot.M[rid];
    if (j.cot.N) b.N = j.cot.N[rid];
    if (j.cot.opd) bopd = j.cot.opd[rid];
    if (j.cot.i) batt = j.cot.i[rid] * (RES ? i_in * ort::intensity(r) : ort::intensity(r));
    if (j.rms_stats) {
      // d rms / d (x, y) = (x - mx, y - my) / (n rms) times the upstream gradient: the
      // ort_rms_spot_vjp kernel's operations, on the final point (the primal's outputs, or
      // the replayed state after the image-space propagate: the same values)
      const double px = replay ? r.x : j.primal.x[r_ld];
      const double py = replay ? r.y : j.primal.y[r_ld];
      const double w = cst(j.rms_grad)[0] / (cst(j.rms_stats)[0] * cst(j.rms_stats)[3]);
      b.x = b.x + (px - cst(j.rms_stats)[1]) * w;
      b.y = b.y + (py - cst(j.rms_stats)[2]) * w;
    }
  }
  const double factor_f = ort::intensity(r);  // RES: d i_out / d i_in
  // image-space propagate (real_ray_tracer.py:84-89): x = x' + d L, ...
  if (a.final_mat >= 0) {
    double bd = b.x * r.L + b.y * r.M + b.z * r.N;
    if (alpha_f > 0.0) bd += batt * (-alpha_f * 1e3);
    ln.emit(3 * a.n_surf + j.n_zern, bd, true);
    const double d = a.final_thickness;
    b.L += d * b.x;
    b.M += d * b.y;
    b.N += d * b.z;
  }

  // ---- reverse over the surfaces
  int64_t trow_end = tape_row0(a.surf, a.n_surf);  // (this surface's rows end here)
  for (int si = a.n_surf - 1; si >= a.start_surface; --si) {
    const ort_surface s = cst(a.surf)[si];
    const ort_surface_optics o = optics_of(s, si);
    trow_end -= tape_rows(s);
    const int64_t trow = trow_end;
    if constexpr ((KM & ort::KM_ZERN) != 0) {
      mono_base = -1;  // this surface's monomial slots (uniform), walking back from the end
      if (j.mono_on) {
        const int ms = mono_slots(s);
        if (ms > 0) {
          mono_end -= ms;
          mono_base = mono_end;
        }
      }
    }
    // cotangent of this surface's record (the state after its globalize): the adjoint of
    // the state there gains it; its intensity row through att (d I / d att = I, the
    // primal's recorded value)
    if (j.rec_cot && (s.flags & ORT_SURF_RECORD) && active) {
      const double* rc = j.rec_cot + (int64_t)s.rec_slot * 8 * NR + rid;
      b.x += rc[0];
      b.y += rc[NR];
      b.z += rc[2 * NR];
      b.L += rc[3 * NR];
      b.M += rc[4 * NR];
      b.N += rc[5 * NR];
      bopd += rc[7 * NR];
      const double ci = rc[6 * NR];
      if (ci != 0.0) batt += ci * j.rec[((int64_t)s.rec_slot * 8 + 6) * NR + rid];
    }
    // the tape rows are read once, with plain loads: non-temporal loads measured no gain
    // (config 5 adjoint 428 / 428 vs 436 / 430 us on the MI355X)
    const double* tp = ln.tape_at(trow);
    ort::Ray q;
    q.x = tp[0];
    q.y = tp[TS];
    q.z = tp[2 * TS];
    q.L = tp[3 * TS];
    q.M = tp[4 * TS];
    q.N = tp[5 * TS];
    q.i = 1.0;
    q.opd = 0.0;
    q.att = 0.0;
    const double t = tp[6 * TS];
    localize(a, s, q);
    const double x1 = q.x + t * q.L;
    const double y1 = q.y + t * q.M;
    D nx, ny, nz;
    (void)sagnorm(s, x1, y1, nx, ny, nz);

    // globalize adjoint: + cs_t, then the op list transposed in reverse
    // surface slots (radius, conic, vertex z) have tangents only with P = 4: the launch
    // takes P = 2 exactly when no surface tangent table is given (ort_api.hip vjp_run), so
    // then their adjoints are not carried at all
    constexpr bool kSurf = P == 4;
    double bCZ = kSurf ? b.z : 0.0;
    for (int c = s.n_cs_glob - 1; c >= 0; --c) {
      const ort_cs_op op = cst(a.cs)[s.cs_glob_off + c];
      adj_cs_op(b, op);
    }

    // interaction adjoint with the aligned normal m = sign(D.n) n, dot = D.m
    // (real_rays.py:141-181, :511-547)
    const double dr = q.L * nx.v + q.M * ny.v + q.N * nz.v;
    const double sgn = dr > 0.0 ? 1.0 : (dr < 0.0 ? -1.0 : (dr == dr ? 0.0 : dr));
    const double mx = nx.v * sgn, my = ny.v * sgn, mz = nz.v * sgn;
    const double dot = fabs(dr);
    double bmx, bmy, bmz, bdot;
    if (s.flags & ORT_SURF_REFLECTIVE) {  // D' = D - 2 dot m
      bdot = -2.0 * (b.L * mx + b.M * my + b.N * mz);
      bmx = -2.0 * dot * b.L;
      bmy = -2.0 * dot * b.M;
      bmz = -2.0 * dot * b.N;
    } else {  // D' = u D + m (root - u dot), root = sqrt(1 - u^2 (1 - dot^2))
      const double u = o.u;
      const double root = sqrt(1.0 - u * u * (1.0 - dot * dot));
      const double fac = root - u * dot;
      const double bs = b.L * mx + b.M * my + b.N * mz;
      bmx = b.L * fac;
      bmy = b.M * fac;
      bmz = b.N * fac;
      bdot = bs * (ort::rdiv(u * u * dot, root) - u);
      b.L *= u;
      b.M *= u;
      b.N *= u;
    }
    b.L += bdot * mx;
    b.M += bdot * my;
    b.N += bdot * mz;
    bmx += bdot * q.L;
    bmy += bdot * q.M;
    bmz += bdot * q.N;
    const double bnx = sgn * bmx, bny = sgn * bmy, bnz = sgn * bmz;

    // normal adjoint -> hit point, radius, conic, Zernike coefficients
    const double bx1 = b.x + bnx * nx.d[0] + bny * ny.d[0] + bnz * nz.d[0];
    const double by1 = b.y + bnx * nx.d[1] + bny * ny.d[1] + bnz * nz.d[1];
    const double bz1 = b.z;
    double bR = 0.0, bk = 0.0;
    if constexpr (P == 4) {
      bR = bnx * nx.d[2] + bny * ny.d[2] + bnz * nz.d[2];
      bk = bnx * nx.d[3] + bny * ny.d[3] + bnz * nz.d[3];
    }
    zern_adj(s, true, true, x1, y1, 0.0, bnx, bny, bnz, nx.v, ny.v, nz.v);

    // propagation, OPD (|t n|) and absorption adjoint -> t
    double bt = bx1 * q.L + by1 * q.M + bz1 * q.N;
    const double tn = t * o.n_pre;
    bt += bopd * (tn > 0.0 ? o.n_pre : (tn < 0.0 ? -o.n_pre : 0.0));
    if (o.alpha_pre > 0.0) bt += batt * (-o.alpha_pre * 1e3);
    b.x = bx1;
    b.y = by1;
    b.z = bz1;
    b.L += t * bx1;
    b.M += t * by1;
    b.N += t * bz1;

    // intersection distance adjoint
    if (s.geometry == ORT_GEOM_PLANE || s.geometry == ORT_GEOM_STANDARD) {
      closed_adj(s, q, t, bt, b, bR, bk);
    } else if constexpr (KM != 0) {
      // the unrolled Newton updates t' = t - f / f' (newton_raphson.py:140-166) in
      // reverse, newest first, from the taped iterates; then the conic initial guess
      const int U = a.sched ? a.sched[group * a.n_surf + si] : s.max_iter;
      const int Uk = U < kHist ? U : kHist;
      const int m_end = ln.uniform_max(active ? Uk : 0);
      // (a linearly converging surface past the tape: NaN, see the initial guess below)
      double tb = U > kHist && (s.flags & ORT_SURF_SLOPE_INEXACT) ? __builtin_nan("") : bt;
      for (int m = 0; m < m_end; ++m) {
        const bool on = m < Uk;
        // (loaded here, a second round trip per surface; loading the newest iterate with
        // the surface's rows measured the same: config 5 step 0.4917 / 0.4953 vs 0.4925 /
        // 0.4929 ms, tools/gpu_r05u.sh)
        const double tk = tp[(7 + m) * TS];
        const double xk = q.x + tk * q.L, yk = q.y + tk * q.M, zk = q.z + tk * q.N;
        D kx, ky, kz;
        const D sk = sagnorm(s, xk, yk, kx, ky, kz);
        const double f = sk.v - zk;
        const bool zg = fabs(kz.v) > 1e-14;
        const double nzs = zg ? kz.v : 1e-14;
        const double inzs = ort::rrcp(nzs);  // (derivative-only quotients: rdiv)
        const double fx = -kx.v * inzs, fy = -ky.v * inzs;
        const double df = fx * q.L + fy * q.M - q.N;
        const bool dg = fabs(df) > 1e-14;
        const double dfs = dg ? df : 1e-14;
        const double tbo = on ? tb : 0.0;
        const double idfs = ort::rrcp(dfs);
        const double bf = -tbo * idfs;
        const double bdfs = dg ? tbo * f * (idfs * idfs) : 0.0;
        const double bfx = bdfs * q.L, bfy = bdfs * q.M;
        const double knx = -bfx * inzs, kny = -bfy * inzs;
        const double knz = zg ? (bfx * kx.v + bfy * ky.v) * (inzs * inzs) : 0.0;
        if (on) {
          b.L += bdfs * fx;
          b.M += bdfs * fy;
          b.N -= bdfs;
          const double bxk = bf * sk.d[0] + knx * kx.d[0] + kny * ky.d[0] + knz * kz.d[0];
          const double byk = bf * sk.d[1] + knx * kx.d[1] + kny * ky.d[1] + knz * kz.d[1];
          const double bzk = -bf;
          if constexpr (P == 4) {
            bR += bf * sk.d[2] + knx * kx.d[2] + kny * ky.d[2] + knz * kz.d[2];
            bk += bf * sk.d[3] + knx * kx.d[3] + kny * ky.d[3] + knz * kz.d[3];
          }
          b.x += bxk;
          b.y += byk;
          b.z += bzk;
          b.L += tk * bxk;
          b.M += tk * byk;
          b.N += tk * bzk;
          tb = tbo + bxk * q.L + byk * q.M + bzk * q.N;
        }
        zern_adj(s, on, false, xk, yk, bf, knx, kny, knz, kx.v, ky.v, kz.v);
      }
      // initial guess: the base conic's closed form (newton_raphson.py:131-135). More than
      // kHist updates: the earlier ones are dropped -- their share is scaled by the
      // products of f f'' / f'^2 over the kept updates, i.e. by converged residuals. Not so
      // where the Newton slope is not the sag's derivative (ORT_SURF_SLOPE_INEXACT: standard
      // / noll Zernike, linear convergence): the host takes the forward-mode VJP when it
      // knows of such a schedule (autodiff.vjp_mode), and a schedule only the device saw
      // (a device-verified round raised it) poisons the gradient with NaN instead of
      // truncating it silently
      const double t0 = U == 0 ? t : tp[(int64_t)(7 + (U <= kHist ? U - 1 : 0)) * TS];
      closed_adj(s, q, t0, U <= kHist || (s.flags & ORT_SURF_SLOPE_INEXACT) ? tb : 0.0, b, bR,
                 bk);
    }

    // localize adjoint: the op list transposed in reverse, then - cs_t
    for (int c = s.n_cs_loc - 1; c >= 0; --c) {
      const ort_cs_op op = cst(a.cs)[s.cs_loc_off + c];
      adj_cs_op(b, op);
    }
    if constexpr (kSurf) {
      bCZ -= b.z;
      ln.emit(3 * si + 0, bR, true);
      ln.emit(3 * si + 1, bk, true);
      ln.emit(3 * si + 2, bCZ, true);
    }
  }
  // no image-space propagate: the final-thickness slot still gets its (zero) partial,
  // so every needed (slot, wave) partial is written by this launch (no memset)
  if (a.final_mat < 0) ln.emit(3 * a.n_surf + j.n_zern, 0.0, true);
  if constexpr (RES) {
    // cotangents of the input rays: the adjoint state at the first traced surface; opd
    // passes straight through, i through the clip / absorption factors
    if (active) {
      if (j.gin.x) j.gin.x[rid] = b.x;
      if (j.gin.y) j.gin.y[rid] = b.y;
      if (j.gin.z) j.gin.z[rid] = b.z;
      if (j.gin.L) j.gin.L[rid] = b.L;
      if (j.gin.M) j.gin.M[rid] = b.M;
      if (j.gin.N) j.gin.N[rid] = b.N;
      if (j.gin.opd) j.gin.opd[rid] = bopd;
      if (j.gin.i) j.gin.i[rid] = (j.cot.i ? j.cot.i[rid] * factor_f : 0.0) + gi;
    }
  }
}

// =====================================================================================
// Forward-mode VJP of one ray w.r.t. lens parameters (the autograd backward; reference:
// torch autograd through the unrolled trace, backend/torch_backend.py +
// optimization/optimizer/torch/base.py:95-154): Zernike coefficients, surface radius and
// conic, surface vertex z (thickness variables) and the image-space propagation distance.
//
// The ray state carries P tangents (ort::Dual<P>), one per parameter of this chunk,
// through exactly the Newton update counts of the primal trace (opt.sched), so the
// derivative is that of the unrolled iteration the reference differentiates. The ray's
// contraction of its tangents with the ray cotangents is added to acc[0 .. P).
// =====================================================================================

template <int P>
ORT_INLINE void cot_acc(double (&acc)[P], const double* g, int64_t rid,
                        const ort::Dual<P>& v) {
  if (!g) return;
  const double c = g[rid];
#pragma unroll
  for (int k = 0; k < P; ++k) acc[k] += c * v.d[k];
}

// v with the tangents of this chunk's parameters: tan[p * stride + off] (uniform loads)
template <int P>
ORT_INLINE ort::Dual<P> seeded(double v, const double* tan, int64_t stride, int off,
                               const JArgs& j) {
  ort::Dual<P> r(v);
  if (tan) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const int p = j.p0 + k;
      r.d[k] = p < j.n_param ? cst(tan)[(int64_t)p * stride + off] : 0.0;
    }
  }
  return r;
}

// a.px set: rays generated from pupil samples (ort_trace_pupil_vjp); NULL: resident input
// rays a.in (ort_trace_sequential_vjp), per-ray wavelengths when a.w is set
template <int P, uint32_t KM>
ORT_INLINE void vjp_ray(const KArgs& a, const JArgs& j, int64_t rid, bool active,
                        double (&acc)[P]) {
  using D = ort::Dual<P>;
  const int64_t r_ld = active ? rid : 0;
  const int64_t sidx = a.seg ? r_ld / a.seg_len : 0;
  int lam = 0;
  double wl = 0.0;
  ort::RayT<D> r;
  if (a.px) {
    const ort_segment sg = a.seg[sidx];
    lam = sg.lambda_idx;
    const int64_t p = a.pupil_per_ray ? r_ld : (r_ld - sidx * a.seg_len);
    r = ort::promote<D>(ort::generate_ray(sg, a.px[p], a.py[p], a.apod));
  } else {
    if (a.seg) lam = a.seg[sidx].lambda_idx;
    if (a.w) wl = a.w[r_ld];
    ort::Ray q;
    q.x = a.in.x[r_ld];
    q.y = a.in.y[r_ld];
    q.z = a.in.z[r_ld];
    q.L = a.in.L[r_ld];
    q.M = a.in.M[r_ld];
    q.N = a.in.N[r_ld];
    q.i = a.in.i[r_ld];
    q.opd = a.in.opd[r_ld];
    q.att = 0.0;
    r = ort::promote<D>(q);
  }
  const int64_t group = r_ld / a.group_len;
  const ort::ZSeed zs{j.zparam, j.p0};
  const int64_t ts = (int64_t)a.n_surf * 3;
  bool unnorm = false;  // a thin lens left the direction unnormalised (F_IA lenses)
#pragma unroll
  for (int k = 0; k < P; ++k) acc[k] = 0.0;

  for (int si = a.start_surface; si < a.n_surf; ++si) {
    const ort_surface s = cst(a.surf)[si];
    const ort_surface_optics o = a.w ? optics_ray(a, s, wl) : optics_row(a, lam, si);
    const D R = seeded<P>(s.radius, j.tan_surf, ts, si * 3 + 0, j);
    const D K = seeded<P>(s.conic, j.tan_surf, ts, si * 3 + 1, j);
    const D CZ = seeded<P>(s.cs_t[2], j.tan_surf, ts, si * 3 + 2, j);
    // localize (coordinate_system.py:73-107) with the vertex z as a parameter
    r.x = r.x + -s.cs_t[0];
    r.y = r.y + -s.cs_t[1];
    r.z = r.z + -CZ;
    for (int c = 0; c < s.n_cs_loc; ++c) ort::apply_cs_op(r, cst(a.cs)[s.cs_loc_off + c]);
    D t;
    if (s.geometry == ORT_GEOM_PLANE) {
      t = ort::distance_plane(r);
    } else {
      t = ort::distance_conic(r, R, K, (s.flags & ORT_SURF_RADIUS_INF) != 0);
      if (s.geometry != ORT_GEOM_STANDARD) {
        if constexpr (KM != 0) {
          // replay the primal's update count (newton_raphson.py:137-166)
          const int U = a.sched ? a.sched[group * a.n_surf + si] : s.max_iter;
          bool rerr = false;
          for (int it = 0; it < U; ++it) {
            D nx, ny, nz;
            const D f = ort::newton_eval<KM>(s, R, K, cst(a.coef), cst(a.zern), zs, r, t,
                                             ort::kSlope, rerr, nx, ny, nz);
            t = ort::newton_step_any(r, t, f, nx, ny, nz);
          }
        }
      }
    }
    bool done = false;
    if constexpr ((KM & 15u) == 15u) {
      // thin-lens / phase / grating surfaces (F_IA lenses take the all-kinds kernels):
      // trace_kernel<F_IA>'s surface step in duals -- propagate, the normalisation a thin
      // lens left pending (homogeneous.py:55-57), OPD, clipping, the interaction model
      if (s.interaction != ORT_IA_REFRACT_REFLECT || unnorm) {
        ort::propagate(r, t, o.alpha_pre);
        if (unnorm) {
          ort::normalize_dir(r);
          unnorm = false;
        }
        ort::add_opd(r, t, o.n_pre);
        if (s.flags & ORT_SURF_APERTURE) ort::clip_radial(r, s.ap_rmax2, s.ap_rmin2);
        if (s.flags & ORT_SURF_APERTURE_PROG) ort::clip_program(r, cst(a.coef) + s.ap_off, s.ap_len);
        const bool refl = (s.flags & ORT_SURF_REFLECTIVE) != 0;
        const PD ip = cst(a.coef) + s.ia_off;
        if (s.interaction == ORT_IA_THIN_LENS) {
          ort::thin_lens(r, ip[0], o.n_pre, refl ? -o.n_pre : o.n_post);
          unnorm = true;
        } else {
          D nx, ny, nz;
          ort::surface_normal<KM>(s, R, K, cst(a.coef), cst(a.zern), zs, r, nx, ny, nz);
          if (s.interaction == ORT_IA_REFRACT_REFLECT) {
            if (refl)
              ort::reflect(r, nx, ny, nz);
            else
              ort::refract(r, nx, ny, nz, o.u);
          } else {
            const double w = a.w ? wl : (a.n_lambda == 1 ? cst(a.lambdas)[0] : a.lambdas[lam]);
            if (s.interaction == ORT_IA_PHASE)
              ort::phase_interact(r, ip, nx, ny, nz, o.n_pre, refl ? o.n_pre : o.n_post, refl, w);
            else
              ort::diffract(r, ip, nx, ny, nz, o.n_pre, o.n_post, refl, w);
          }
        }
        done = true;
      }
    }
    if (!done)
      ort::finish_surface<KM>(r, s, R, K, cst(a.coef), cst(a.zern), zs, t, o.n_pre, o.u,
                              o.alpha_pre);
    for (int c = 0; c < s.n_cs_glob; ++c) ort::apply_cs_op(r, cst(a.cs)[s.cs_glob_off + c]);
    r.x = r.x + s.cs_t[0];
    r.y = r.y + s.cs_t[1];
    r.z = r.z + CZ;
    if (j.rec_cot && (s.flags & ORT_SURF_RECORD) && active) {  // this surface's record
      const double* rc = j.rec_cot + (int64_t)s.rec_slot * 8 * a.n_rays;
      cot_acc(acc, rc, rid, r.x);
      cot_acc(acc, rc + a.n_rays, rid, r.y);
      cot_acc(acc, rc + 2 * a.n_rays, rid, r.z);
      cot_acc(acc, rc + 3 * a.n_rays, rid, r.L);
      cot_acc(acc, rc + 4 * a.n_rays, rid, r.M);
      cot_acc(acc, rc + 5 * a.n_rays, rid, r.N);
      cot_acc(acc, rc + 6 * a.n_rays, rid, ort::intensity(r));
      cot_acc(acc, rc + 7 * a.n_rays, rid, r.opd);
    }
  }
  if (a.final_mat >= 0) {
    ort::propagate(r, seeded<P>(a.final_thickness, j.tan_final, 1, 0, j),
                   a.w ? ort::absorption_alpha(ort::material_k(cst(a.mats)[a.final_mat], a.coef, wl), wl)
                       : tab(a.alpha_tab, a.n_lambda, a.n_mat, lam, a.final_mat));
    if constexpr ((KM & 15u) == 15u) {
      if (unnorm) ort::normalize_dir(r);
    }
  }

  if (active) {
    cot_acc(acc, j.cot.x, rid, r.x);
    cot_acc(acc, j.cot.y, rid, r.y);
    cot_acc(acc, j.cot.z, rid, r.z);
    cot_acc(acc, j.cot.L, rid, r.L);
    cot_acc(acc, j.cot.M, rid, r.M);
    cot_acc(acc, j.cot.N, rid, r.N);
    if (j.cot.i) cot_acc(acc, j.cot.i, rid, ort::intensity(r));
    cot_acc(acc, j.cot.opd, rid, r.opd);
  }
}

}  // namespace ortk
