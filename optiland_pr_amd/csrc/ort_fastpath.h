// ort_fastpath.h -- the closed-form surface math (plane / conic, ray generation) with
// DEFERRED range checks, for trace_closed_kernel (ort_kernels.h).
//
// ort_core.h's sqrt / shared_div / sdiv run the correctly rounded gfx950 sequences
// without their range wrappers and fall back per operation (a divergent branch around
// every op) when an operand leaves the range where the wrappers are identities. Here the
// same instruction sequences run unconditionally and each operation only ORs "an operand
// was outside that range" into a per-lane flag; a lane that ends its ray with the flag
// set re-traces the whole ray on the per-operation path. Every value a lane keeps is
// therefore bit-identical to ort_core.h's (and so to the reference's IEEE operations):
// inside the ranges the fast sequences ARE the IEEE results, outside them the ray is
// recomputed. What goes away is the exec-mask bookkeeping and the taken branch per op.
//
// Ranges (the same as ort_core.h):
//   sqrt(x):   2^-767 <= x < inf
//   a / b:     2^-300 <= |b| <= 2^300 and 2^-300 <= |a| <= 2^300, or a == +0: the
//              quotient sequence q0 = a y, r = fma(-b, q0, a), q = fma(r, y, q0) then
//              yields +0 * sign(b) exactly (q0 carries the sign, r = +0); -0 and every
//              other value outside the range takes the exact path.
//
// Upper bounds (and the divisors' lower bound) are not tested per operation. Past them the short sequences do not return
// a wrong FINITE value, only a non-finite one: sqrt(+inf) gives NaN (rsq = 0, g = inf*0);
// a numerator large enough to matter overflows q0 = a y to inf and the quotient to inf or
// NaN. Non-finite values are sticky in the ray state -- a non-finite t makes the OPD
// (opd += |t n|, a sum of non-negative terms) non-finite for good, a non-finite direction
// or position makes the next t non-finite or is itself an output -- so the kernel tests
// the finished state once (state_ok) and re-traces such lanes exactly. Only the
// numerators' and sqrt's lower bounds (where the sequences would underflow into a finite,
// wrongly rounded result) and the divisors' upper bound (a reciprocal small enough to
// underflow a quotient) stay per operation.
//
// The sequences themselves (the root from a seed, the two reciprocals, the two quotients)
// are ort_core.h's, written once there with their error bounds and host arms; each wrapper
// here is one of them, its seed, and at most one range test.
//
// The plain form's kernels (F_PLAIN, fast pass only) take three shorter forms where a value
// is already at hand or a test cannot fire on a finite result: a sphere's norm root
// sqrt(dfdx^2 + dfdy^2 + 1) seeded from g = sqrt(1 - q) instead of v_rsq (normal_conic_rcp,
// sqrt_seeded_h), a sphere's 1 / (L^2 + M^2 + N^2) from 2 - a and one step
// (shared_div_unit), and sqrt(1.0 - v) without its lower-bound test (sqrt_untested). Two
// more drop work the stored bits do not need: a sphere's quadratic keeps the one root the
// reference would choose, predicted by a sign and held to it by a guard
// (distance_conic_folded), and the refraction puts the normal's alignment on one sign bit
// (refract). The Newton kernels' calls (template defaults) compile to what they did.
//
// Formulas and their order follow ort_core.h (and through it the reference files cited
// there); only the check placement differs. Host compilation: plain IEEE operations.
#pragma once

#include "ort_core.h"

namespace ort {
namespace fast {

#define ORT_CHK(bad, cond) ::ort::fast::chk((bad), (cond))
#define ORT_CHK_UNIFORM(bad, cond) ::ort::fast::chk_uniform((bad), (cond))

// The flag a sequence ORs its range failures into (the functions' class B): a per-lane
// bool, or WaveFlag, the same flags of a whole wave as a mask (bit = lane). A loop that
// carries a bool across uniform branches keeps it in a vector register and converts it
// to a lane mask and back at every join; the mask is wave-uniform, so it lives in scalar
// registers (the closed-form kernel's surface loop, which ORs each surface's bool in once).
struct WaveFlag {
  uint64_t m;
};
ORT_INLINE void chk(bool& bad, bool cond) { bad = bad | cond; }
// a wave-uniform condition (a lens constant)
ORT_INLINE void chk_uniform(bool& bad, bool cond) { bad = bad | cond; }
#if defined(__HIPCC__)  // device code only: there is no wave on the host
__device__ inline void chk(WaveFlag& bad, bool cond) { bad.m |= __builtin_amdgcn_ballot_w64(cond); }
__device__ inline void chk_uniform(WaveFlag& bad, bool cond) {
  if (cond) bad.m = ~0ull;
}
#endif

ORT_INLINE bool is_pos_zero(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_class(v, 1 << 6);  // v_cmp_class_f64: +0 only
#else
  return v == 0.0 && !signbit(v);
#endif
}

// ---- square roots: ort_core.h's sqrt_seeded_h, which also hands out h (2 h ~ 1 / root, the
// seed of shared_div_seeded below); non-finite results are left to state_ok ---------------

// sqrt(x) for 2^-767 <= x < inf (ort_core.h sqrt)
template <class B>
ORT_INLINE double sqrt_h(double x, B& bad, double& h_out) {
  const double g = sqrt_seeded_h(x, rsq_seed(x), h_out);
  ORT_CHK(bad, !(x >= 0x1p-767));  // +inf gives NaN: left to state_ok
  return g;
}
template <class B>
ORT_INLINE double sqrt(double x, B& bad) {
  double h;
  return sqrt_h(x, bad, h);
}

// sqrt_h without its test, for an x that cannot lie in (0, 2^-767), where the test fires
// on a finite result. Two kinds of caller:
//   x >= 1 unless NaN (sums of squares plus 1): only the upper bound could fail, and
//     +inf / NaN give NaN, which state_ok catches;
//   x = fl(1.0 - v) (the plain form's kernels): it is <= 0 or >= 2^-53 (v <= 1 - 2^-53
//     leaves 1 - v >= 2^-53); x = 0 (rsq = inf, g = 0 inf), x < 0, NaN and +inf (v = -inf)
//     all give NaN, which is sticky in the ray state and caught by state_ok.
ORT_INLINE double sqrt_untested_h(double x, double& h_out) {
  return sqrt_seeded_h(x, rsq_seed(x), h_out);
}
ORT_INLINE double sqrt_untested(double x) {
  double h;
  return sqrt_untested_h(x, h);
}
// (A seed of the caller's own in v_rsq's place: sqrt_seeded_h itself, no test either;
// normal_conic_rcp's sphere branch states where its seed's bound comes from.)

// ---- reciprocals: ort_core.h's rcp_refined / rcp_seeded with the divisor kept beside them
struct Div {
  double b, y;
};

template <class B>
ORT_INLINE Div shared_div(double b, B& bad) {
  const Div d{b, rcp_refined(b)};
  // |b| <= 2^300 (false for NaN). Below 2^-1021 (zero and subnormal divisors included)
  // the reciprocal is infinite and every quotient non-finite -- NaN for a zero
  // numerator, +-inf or NaN otherwise -- which state_ok catches; in between the
  // refined reciprocal is accurate and, as every numerator is >= 2^-300 or an exact zero
  // (sdiv / sdiv0 / num_ok), q0 = a y cannot underflow (|q| >= 2^-600).
  ORT_CHK(bad, !(::fabs(b) <= 0x1p300));
  return d;
}

// shared_div without its test, for a divisor whose range is known another way:
//   a norm sqrt(s), s = a^2 + b^2 + 1 >= 1 unless NaN: it is at most sqrt(DBL_MAX) < 2^512
//     -- its refined reciprocal >= 2^-512 is accurate and the quotients of the checked
//     numerators (|a| >= 2^-300 or +-0, and -1) stay normal -- or, with s overflowed, +inf,
//     whose zero reciprocal makes every quotient NaN for state_ok; NaN likewise. (Round 6:
//     the b <= 2^300 test this had was one of those that cannot fail on a finite result.)
//   the Newton aspheres' positive divisors R^2, |R| (1 + q), |R| q: tested once per
//     evaluation (lens_range below).
ORT_INLINE Div shared_div_untested(double b) { return Div{b, rcp_refined(b)}; }

// shared_div from a seed y0 = (1 + es) / b (rcp_seeded: es^2 after its one step); the
// range test is the unseeded form's, unchanged. A non-finite or zero seed gives NaN
// quotients, for state_ok.
template <class B>
ORT_INLINE Div shared_div_seeded(double b, double y0, B& bad) {
  const Div d{b, rcp_seeded(b, y0)};
  ORT_CHK(bad, !(::fabs(b) <= 0x1p300));
  return d;
}
// divisor in [1, inf) unless NaN (a norm, shared_div_untested's first case): no test
ORT_INLINE Div shared_div_ge1_seeded(double b, double y0) { return Div{b, rcp_seeded(b, y0)}; }

// 1 / b for b = L^2 + M^2 + N^2 of a unit direction (a sphere's quadratic in the plain
// form): y0 = 2 - b = (1 - (1 - b)^2) / b, so with |1 - b| <= 2^-27 (tested; false for
// NaN) the seed's es is within 2^-54 + 2^-53 (2 - b rounds only for b < 1) and
// rcp_seeded's one step leaves es^2 < 2^-104. The test stands in for shared_div's
// |b| <= 2^300 as well.
template <class B>
ORT_INLINE Div shared_div_unit(double b, B& bad) {
  const Div d{b, rcp_seeded(b, 2.0 - b)};
  ORT_CHK(bad, !(::fabs(1.0 - b) <= 0x1p-27));
  return d;
}

// ---- quotients: ort_core.h's quot / quot_pos (the latter for a divisor > 0: an exact-zero
// numerator keeps its sign) ---------------------------------------------------------------
ORT_INLINE double quot(double a, const Div& d) { return ort::quot(a, d.b, d.y); }
ORT_INLINE double quot_pos(double a, const Div& d) { return ort::quot_pos(a, d.b, d.y); }

// |a| >= 2^-300 (false for 0 and NaN); a numerator past 2^300 overflows into a
// non-finite quotient (see the header)
ORT_INLINE bool num_ok(double a) { return ::fabs(a) >= 0x1p-300; }

// a / b, |a| >= 2^-300
template <class B>
ORT_INLINE double sdiv(double a, const Div& d, B& bad) {
  ORT_CHK(bad, !num_ok(a));
  return quot(a, d);
}
// a / b, |a| >= 2^-300 or a == +0 (coordinates on a symmetry plane)
template <class B>
ORT_INLINE double sdiv0(double a, const Div& d, B& bad) {
  ORT_CHK(bad, !(num_ok(a) || is_pos_zero(a)));
  return quot(a, d);
}

// a / b as one IEEE division
template <class B>
ORT_INLINE double div(double a, double b, B& bad) {
  const Div d = shared_div(b, bad);
  return sdiv0(a, d, bad);
}

// rays/ray_generator.py:71-106 + fields/field_types.py:160-181 (ort_core.h generate_ray)
template <class B>
ORT_INLINE Ray generate_ray(const ort_segment& s, double px, double py,
                            const ort_apodization* apod, B& bad) {
  Ray r;
  double x0, y0;
  if (s.mode == ORT_GEN_INFINITE) {
    x0 = px * s.epd / 2.0 * s.vx + s.x_off;
    y0 = py * s.epd / 2.0 * s.vy + s.y_off;
  } else {
    x0 = s.x_off;
    y0 = s.y_off;
  }
  const double z0 = s.z0;
  double x1, y1;
  if (s.mode == ORT_GEN_TELECENTRIC) {
    x1 = px * s.vx + x0;
    y1 = py * s.vy + y0;
  } else {
    x1 = px * s.epd * s.vx / 2.0;
    y1 = py * s.epd * s.vy / 2.0;
  }
  const double z1 = s.epl;
  const double dx = x1 - x0, dy = y1 - y0, dz = z1 - z0;
  // the norm's reciprocal seeded by its own root: |es| <= 1.5 e0^2 + 2^-51, es^2 after
  // the step (shared_div_seeded)
  double hm;
  const double mag = sqrt_h(dx * dx + dy * dy + dz * dz, bad, hm);
  ORT_CHK(bad, (mag < 1e-9));  // the (0, 0, 1) branch of ray_generator.py:82-89
  const Div dm = shared_div_seeded(mag, 2.0 * hm, bad);
  // mag > 0: quot_pos is exact for zero numerators of either sign
  ORT_CHK(bad, !((num_ok(dx) || dx == 0.0) && (num_ok(dy) || dy == 0.0) &&
                 (num_ok(dz) || dz == 0.0)));
  r.L = quot_pos(dx, dm);
  r.M = quot_pos(dy, dm);
  r.N = quot_pos(dz, dm);
  r.x = x0;
  r.y = y0;
  r.z = z0;
  r.i = apod ? apodize(*apod, px, py) : 1.0;  // no range-sensitive operations
  r.opd = 0.0;
  r.att = 0.0;
  return r;
}

// The end-of-trace test of the header: every output of the ray state finite and below
// 2^1000 (false for NaN / inf; the bound also covers a quotient that would overflow only
// in the short sequence, |q| ~ 2^1023). The intensity is not tested: only the clip tests
// write it, on positions that are themselves tested here.
ORT_INLINE bool state_ok(const Ray& r) {
  constexpr double kMax = 0x1p1000;
  return ::fabs(r.x) < kMax && ::fabs(r.y) < kMax && ::fabs(r.z) < kMax &&
         ::fabs(r.L) < kMax && ::fabs(r.M) < kMax && ::fabs(r.N) < kMax && ::fabs(r.opd) < kMax;
}

// plane.py:61-77 (-z / N) and the plane branch of standard.py:100-103
template <class B>
ORT_INLINE double distance_plane(const Ray& r, B& bad) { return div(-r.z, r.N, bad); }

// standard.py:89-140 (ort_core.h distance_conic); s.two_r = 2 R formed on the host.
// The Newton kernels' form; distance_conic_folded below is the closed-form kernel's copy
// with the powers of two folded out: a change here belongs there too -- but for that
// copy's one-root sphere branch (plain form only), which stays out of here: these kernels
// sit at register and scratch edges, their a is not tested to be within 2^-27 of 1 (the
// branch's error bounds lean on it), and nothing shares z + t N with the propagation.
// (The two-root tail is written out in both: as one shared function it compiled to other
// register assignments in six trace_kernel instantiations.)
ORT_INLINE double distance_conic(const Ray& r, const ort_surface& s, bool radius_inf,
                                 bool& bad) {
  if (radius_inf) {
    const double Ns = ::fabs(r.N) > 1e-14 ? r.N : 1e-14;
    return div(-r.z, Ns, bad);
  }
  const double R = s.radius, k = s.conic;
  const double N2 = r.N * r.N;
  const double z2 = r.z * r.z;
  double a, b, c;
  if (k == 0.0) {
    a = r.L * r.L + r.M * r.M + N2;
    b = 2.0 * (r.L * r.x + r.M * r.y - r.N * R + r.N * r.z);
    c = 0.0 - s.two_r * r.z + r.x * r.x + r.y * r.y + z2;
  } else {
    a = k * N2 + r.L * r.L + r.M * r.M + N2;
    b = 2.0 * (k * r.N * r.z + r.L * r.x + r.M * r.y - r.N * R + r.N * r.z);
    c = k * z2 - s.two_r * r.z + r.x * r.x + r.y * r.y + z2;
  }
  const double d = b * b - 4.0 * a * c;
  const double sd = sqrt(d, bad);
  const Div a2 = shared_div(2.0 * a, bad);
  // nonzero numerators (checked): quot_pos and quot agree for either sign of a
  const double n1 = -b + sd, n2 = -b - sd;
  ORT_CHK(bad, !(num_ok(n1) && num_ok(n2)));
  const double t1 = quot_pos(n1, a2);
  const double t2 = quot_pos(n2, a2);
  const double z1 = r.z + t1 * r.N;
  const double zz2 = r.z + t2 * r.N;
  // a == 0 (the -c / b branch, standard.py:138) fails shared_div's range test
  return ::fabs(z1) <= ::fabs(zz2) ? t1 : t2;
}

// x with the sign bit of s, any x and s: one bit-field insert on the high dword
ORT_INLINE double with_sign_of(double x, double s) { return __builtin_copysign(x, s); }

// distance_conic with the powers of two folded out of the quadratic, for the closed-form
// kernel (three multiplications and one subtraction fewer per conic); the Newton kernels
// keep distance_conic above, and a change to either belongs in both. With
// S = L x + M y - N R + N z the reference forms
//   b = 2 S, d = b b - (4 a) c, sd = sqrt(d), t = (-b +- sd) / (2 a);
// this forms
//   d' = S S - a c, sd' = sqrt(d'), t = (-S +- sd') / a.
// Multiplying by 2 or 4 is exact and commutes with the rounding of every product, sum and
// correctly rounded square root it passes through as long as no value involved underflows
// or overflows, so d = 4 d', sd = 2 sd', -b +- sd = 2 (-S +- sd') and the two quotients
// are roundings of the same real numbers: t is the reference's bit for bit. Where that
// premise can fail the lane is flagged:
//   overflow:  b b or (4 a) c may be infinite with S S, a c finite only when S S or |a c|
//              >= 2^1022; both are tested against 2^1020 (then 4 |S S - a c| < 2^1023 too).
//   underflow: a product S S or a c below 2^-1022 is rounded on the subnormal grid and may
//              differ from a quarter of its scaled twin by up to 2^-1075. If the other
//              product is >= 2^-960 that is under 2^-60 of its ulp and both differences
//              round to the other product alone; otherwise |d'| < 2^-959, which fails
//              sqrt's own lower bound 2^-767. A difference that is itself subnormal fails
//              that bound as well.
// The remaining tests are the reference sequence's on the rescaled operands: d' >= 2^-767
// (d >= 2^-765), |a| <= 2^300 (the divisor range itself; 2 a <= 2^300 was tested before),
// |-S +- sd'| >= 2^-300.
// PLAIN, sphere: 1 / a from shared_div_unit (a = |(L, M, N)|^2 ~ 1; its |1 - a| <= 2^-27
// test replaces |a| <= 2^300). sphere: the caller's k == 0.0, a uniform test made once per
// surface for this and the normal.
// k == 0: the reference's c starts (0.0 - 2R z) + x x. 0.0 - p is -p unless p is a zero,
// where it is +0 and -p may be -0; x x is >= +0 or NaN, and (+-0) + (+0) = +0,
// (+-0) + w = w: x x - p is the same value.
//
// PLAIN, sphere: ONE root. The reference takes both quotients t1 = (-S + sd) / a,
// t2 = (-S - sd) / a, forms z1 = fl(z + fl(t1 N)), z2 likewise, and keeps t1 when
// |z1| <= |z2|, else t2. Both hit points of a line with x^2 + y^2 + z^2 = 2 R z have a z
// of R's sign, and z1 - z2 = 2 sd N / a with sd, a > 0: the hit of smaller |z| is root 1
// exactly when N R < 0. That is only the PREDICTION (sd gets the sign bit of N xor that of
// R, n = -S - sd_s is n1 or n2 bit for bit); what makes the kept t the reference's is the
// guard, which proves the reference's comparison of its two ROUNDED z without forming the
// other one. With t_c, z_c the kept root's quotient and z, t_o, z_o the other's (both as
// the reference rounds them), u = 2^-53, and D = z_o - z_c: |z_o| >= |D| - |z_c|, so
//   |D| > 2 |z_c|  implies  |z_c| < |z_o| strictly,
// which selects t_c whichever root it is (root 1 wins ties, root 2 needs the strict sign),
// and needs no fact about the signs of z_c, z_o or R. The guard is
//   fma(-c, |z_c|, P) > 2^-300,  P = fl(sd |N|),  c = 1 + 2^-20  (a product, an fma, a compare),
// and on a lane that raised no flag at all it implies |D| > 2 |z_c|:
//   Size of d.  d = fl(SS - ac) >= 2^-767 (sqrt's test) is a positive difference of two
//     doubles. For ac <= 0, d >= SS. For ac > 0, SS > ac are distinct doubles, so SS - ac is
//     at least the spacing below SS, >= 2^-53 SS (SS >= d is normal). Either way
//     d >= 2^-53 SS, and with SS = S S (1 + e), sd = RN(sqrt d):  |S| < 2^26.6 sd. The root
//     cannot be arbitrarily small against |S|.
//   Separation. n_o, n_c = fl(-S +- sd): n_o - n_c = +-2 sd + e_n, |e_n| <= 2u (|S| + sd) <
//     2^-24.9 sd. The quotients (a within 2^-27 of 1: shared_div_unit's test) add
//     |e_t| <= u (|n_o| + |n_c|) / a, as much again: |t_o - t_c| >= 2 sd (1 - 2^-24.6). The
//     products fl(t N) err by u |t N| each, |t| < 2^27.2 sd: together < 2^-24.8 sd |N|.
//     So |fl(t_o N) - fl(t_c N)| >= 2 sd |N| (1 - 2^-24): the separation is the PRODUCT
//     2 sd |N| / a, with no cancellation in it, and every error above is relative to it.
//   Rounding of the sums. fl(z + w) = (z + w)(1 + e), |e| <= u, is relative to the RESULT,
//     so a |z| that is large against |S N| (a ray started far from the surface) enters
//     only through |t N| above, already bounded by sd |N|: z_o = z_c + D gives
//     |D| (1 + u) >= 2 sd |N| (1 - 2^-24) - 2u |z_c|.
//   The guard.  The fma rounds P - c |z_c| once, and a rounded value above 2^-300 has a
//     positive exact one: c |z_c| < P and P > 2^-300 is normal, P <= sd |N| (1 + u). So
//     |z_c| < sd |N| (1 + u) / c and 2 |z_c| < 2 sd |N| (1 - 2^-20 + 2^-39) < |D|. The
//     2^-300 keeps sd |N| out of the range where a product t N or a quotient could
//     underflow by more than 2^-770 of it (t N is rounded on the subnormal grid to within
//     2^-1075); every lens length the host accepts (|R| >= 2^-150) is far above it.
//   Zero and NaN. N = +-0 makes P = 0 and the compare false (the prediction would be wrong
//     for N = +0, R > 0: the reference's tie keeps root 1); a NaN in z_c, sd or N makes it
//     false; d <= 0 or NaN fails sqrt's test, and d = +inf the 2^1020 test above; an
//     infinite N passes the guard but fails |1 - a| <= 2^-27. All are flagged here, not
//     left to state_ok.
// The other root's |n_o| >= 2^-300 test goes with its quotient: it guarded the short
// sequence, not the reference's value. A wrong prediction cannot store a wrong t -- its z_c
// is the far hit, |z_c| >= |D| - |z_o| -- it only flags the lane. The guard also flags a
// right prediction whose hit lies above half the z-extent of the chord, 3 |z_c| > |z_o|
// (for a ray along the axis r / |R| > 0.866): correct and slow, a divergent exact re-trace.
// The sample objectives at their bench fields flag no ray (tests/test_one_root_cpu.py).
// k != 0, an infinite radius and the Newton kernels (distance_conic) keep both roots: a
// conic's two hits need not lie on one side of z = 0.
constexpr double kOneRootC = 1.0 + 0x1p-20;
template <bool PLAIN = false, class B>
ORT_INLINE double distance_conic_folded(const Ray& r, const ort_surface& s, bool radius_inf,
                                        bool sphere, B& bad) {
  if (radius_inf) {
    const double Ns = ::fabs(r.N) > 1e-14 ? r.N : 1e-14;
    return div(-r.z, Ns, bad);
  }
  const double R = s.radius, k = s.conic;
  const double N2 = r.N * r.N;
  const double z2 = r.z * r.z;
  double a, S, c;
  if (sphere) {
    a = r.L * r.L + r.M * r.M + N2;
    S = r.L * r.x + r.M * r.y - r.N * R + r.N * r.z;
    c = r.x * r.x - s.two_r * r.z + r.y * r.y + z2;
  } else {
    a = k * N2 + r.L * r.L + r.M * r.M + N2;
    S = k * r.N * r.z + r.L * r.x + r.M * r.y - r.N * R + r.N * r.z;
    c = k * z2 - s.two_r * r.z + r.x * r.x + r.y * r.y + z2;
  }
  const double SS = S * S, ac = a * c;
  ORT_CHK(bad, !(SS < 0x1p1020 && ::fabs(ac) < 0x1p1020));
  const double d = SS - ac;
  const double sd = sqrt(d, bad);
  Div a1;
  if (PLAIN && sphere) {
    a1 = shared_div_unit(a, bad);
    // the predicted root: -S + sd (root 1) exactly when N R < 0; sd >= 0 or NaN
    const double sd_s = with_sign_of(sd, __longlong_as_double(__double_as_longlong(r.N) ^
                                                              __double_as_longlong(R)));
    const double n = -S - sd_s;  // x - (-y) is x + y: n1's or n2's bits
    ORT_CHK(bad, !num_ok(n));
    const double t = quot_pos(n, a1);
    const double zc = r.z + t * r.N;  // propagate's own expression: formed once
    ORT_CHK(bad, !(fma(-kOneRootC, ::fabs(zc), ::fabs(sd_s * r.N)) > 0x1p-300));
    return t;
  }
  a1 = shared_div(a, bad);
  // nonzero numerators (checked): quot_pos and quot agree for either sign of a
  const double n1 = -S + sd, n2 = -S - sd;
  ORT_CHK(bad, !(num_ok(n1) && num_ok(n2)));
  const double t1 = quot_pos(n1, a1);
  const double t2 = quot_pos(n2, a1);
  const double z1 = r.z + t1 * r.N;
  const double zz2 = r.z + t2 * r.N;
  // a == 0 (the -c / b branch, standard.py:138) fails shared_div's range test
  return ::fabs(z1) <= ::fabs(zz2) ? t1 : t2;
}

// standard.py:154-167 with the host's inv_r2 = RN(1 / (R * R)) (ort_core.h
// normal_conic_rcp: the Markstein-corrected quotient needs no range check of its own --
// r^2 = 0 / inf / NaN give the reference's 1 - q)
// PLAIN (the plain form's kernels): a surface with ORT_SURF_TWO_INV_R carries RN(2 / R) in
// norm_radius, and 1 / denom, denom = R sqrt(1 - q), is seeded from the root's own h ~
// 1 / (2 sqrt(1 - q)): y0 = (2 / R) h, then shared_div_seeded's one step and its
// |denom| <= 2^300 test. The seed's relative error es: 2 h against 1 / g is within
// 1.5 e0^2 + 2^-51 (sqrt_h, g's rounding included), and three more roundings of 2^-53
// each follow -- R g, RN(2 / R), the product (2 / R) h -- so for e0 <= 2^-20
// |es| < 1.5 2^-40 + 2^-51 + 3 2^-53 < 2^-39, and the step leaves es^2 < 2^-78. (|R| in
// 2^-150 .. 2^150 with the bit, so 2 / R is a normal number and the product rounds as
// one.) A table without the bit (another producer's) keeps shared_div(denom): a uniform
// branch on the loaded flags.
// PLAIN, sphere (k == 0, the caller's uniform test) on a surface with the bit: the norm's
// root sqrt(X), X = fl(dfdx^2 + dfdy^2 + 1), takes y = g = RN(sqrt(w)), w = fl(1 - q), in
// v_rsq(X)'s place (sqrt_seeded_h): g is 1 / sqrt(X) already. With u = 2^-53 and
// T = (x^2 + y^2) / R^2:
//   q = T (1 + e1), |e1| <= 4u: r2's two roundings, r_sq = RN(R R), the Markstein quotient;
//   s = fl(dfdx^2 + dfdy^2) = (T / w)(1 + e2), |e2| <= 8u: g's rounding and R g's, each
//       squared, the two quotients' (squared), the squares', the sum's;
//   so s = (q / w)(1 + e3), |e3| <= 12.2u, and X = (1 + s)(1 + rho), |rho| <= u;
//   w = 1 - q + eta, |eta| <= u / 2 (w in [1/2, 1]; below 1/2 the difference is exact).
// X w = (w + q (1 + e3))(1 + rho) = (1 + eta + q e3)(1 + rho), q <= 1: |X w - 1| < 13.8u.
// The errors are absolute, against 1: a small w does not amplify them. g^2 = w (1 + 2 gam),
// |gam| <= u, so |g sqrt(X) - 1| < 6.9u + u + O(u^2) < 2^-50, whatever the hit height, where
// v_rsq has e0 = 2^-20: the sequence's bounds hold with room (sqrt_seeded_h).
//   q = 0 (vertex): w = 1, g = 1, dfdx = dfdy = +-0, X = 1: the seed is exact.
//   w at its low end: 2^-53, the least positive fl(1 - q) (sqrt_untested_h); s <= 2^54 then, and
//     no product above under- or overflows (|x|, |y| >= 2^-300 or +0, checked by sdiv0).
//   w <= 0: g is NaN, and so are denom, the slopes, X and the normal: state_ok.
// Nothing but the seed changes: mag is the same RN(sqrt(X)) and 2 hm seeds 1 / mag as
// before. (Dropping the coupled step as well -- gm = X g, hm = g / 2 into the two
// corrections -- is not done: the last correction rounds g + d h, which is sqrt(X) off by
// (ulp / 2) |eh|, and lands on the right side of a rounding boundary that sqrt(X) comes
// within 2^-107 of (X = 1 + 2^-52 is one) only because the coupled step leaves h at its
// own rounding, |eh| ~ 2^-53; g / 2 has 2^-50.) k != 0 and tables without the bit keep
// v_rsq(X).
// SPHERES (the all-spheres form, ORT_LENS_SPHERES: PLAIN with every standard surface a
// sphere that carries the bit): `seeded` is a constant, and a = (1 + k) r2 is r2 itself, so
// neither s.one_plus_k nor s.flags is read. 1.0 * r2 has the bits of r2 for every r2 that
// is not a NaN: an IEEE product with 1.0 is exact (nothing to round), zeros and infinities
// keep their sign (sign = xor of the signs, and 1.0 is positive), and fp64 denormals are
// not flushed on gfx950. For a NaN r2 IEEE leaves the payload to the implementation, and
// none is claimed here: r2 is a sum, so it is a quiet NaN either way, q, g, denom and the
// normal are NaN with or without the product, NaN is sticky in the ray state, and state_ok
// sends the lane to the exact re-trace -- no NaN of this function is ever stored.
template <bool PLAIN = false, bool SPHERES = false, class B>
ORT_INLINE void normal_conic_rcp(double x, double y, const ort_surface& s, bool sphere,
                                 double& nx, double& ny, double& nz, B& bad) {
  static_assert(PLAIN || !SPHERES, "the all-spheres form is a plain form");
  const double r2 = x * x + y * y;
  const double a = SPHERES ? r2 : s.one_plus_k * r2;
  const double q0 = a * s.inv_r2;
  const double q = fma(fma(-s.r_sq, q0, a), s.inv_r2, q0);
  double h, g;
  if constexpr (PLAIN)
    g = sqrt_untested_h(1.0 - q, h);
  else
    g = sqrt_h(1.0 - q, bad, h);
  const double denom = s.radius * g;
  Div dd;
  bool seeded = false;  // the surface carries the bit
  if constexpr (PLAIN) {
    seeded = SPHERES || (s.flags & ORT_SURF_TWO_INV_R) != 0;
    if (seeded)
      dd = shared_div_seeded(denom, s.norm_radius * h, bad);
    else
      dd = shared_div(denom, bad);
  } else {
    dd = shared_div(denom, bad);
  }
  const double dfdx = sdiv0(x, dd, bad);
  const double dfdy = sdiv0(y, dd, bad);
  double hm, mag;
  const double X = dfdx * dfdx + dfdy * dfdy + 1.0;
  if (PLAIN && seeded && sphere)
    mag = sqrt_seeded_h(X, g, hm);
  else
    mag = sqrt_untested_h(X, hm);
  // 1 / mag seeded by 2 h of mag's own root: |es| <= 1.5 e0^2 + 2^-51, es^2 after the step
  const Div dm = shared_div_ge1_seeded(mag, 2.0 * hm);
  // dfdx = x / denom with x checked (|x| in [2^-300, 2^300] or +0) and |denom| <= 2^300:
  // |dfdx| >= 2^-600 or +-0, and |dfdx| <= mag -- in range for the positive divisor
  // mag, zeros of either sign included (quot_pos): no check left to make
  nx = quot_pos(dfdx, dm);
  ny = quot_pos(dfdy, dm);
  nz = quot(-1.0, dm);  // constant numerator: always in range
}

// the Newton kernels' call: no sphere branch outside the plain form
template <class B>
ORT_INLINE void normal_conic_rcp(double x, double y, const ort_surface& s, double& nx,
                                 double& ny, double& nz, B& bad) {
  normal_conic_rcp<false>(x, y, s, false, nx, ny, nz, bad);
}

// rays/real_rays.py:511-547 (ort_core.h align_normal) for dot != 0: sign(dot) is +-1 and
// n * sign(dot) is n with its sign bit flipped when dot < 0 -- the same bits as the
// product; dot == 0 (sign 0) and NaN take the exact path
template <class B>
ORT_INLINE double align_normal(const Ray& r, double& nx, double& ny, double& nz, B& bad) {
  const double dot = r.L * nx + r.M * ny + r.N * nz;
  ORT_CHK(bad, !(::fabs(dot) > 0.0));
  const uint64_t sb = (uint64_t)__double_as_longlong(dot) & 0x8000000000000000ull;
  nx = __longlong_as_double((long long)((uint64_t)__double_as_longlong(nx) ^ sb));
  ny = __longlong_as_double((long long)((uint64_t)__double_as_longlong(ny) ^ sb));
  nz = __longlong_as_double((long long)((uint64_t)__double_as_longlong(nz) ^ sb));
  return ::fabs(dot);
}

// rays/real_rays.py:141-163 (ort_core.h refract); u_sq = RN(u * u) from the host table
// PLAIN (the plain form's kernels): the normal is not flipped. With s = sign(dot) = +-1
// the aligned form above computes, per component,
//   u L0 + (s nx) root - (u (s nx)) |dot|,        |dot| = s dot.
// A sign flip is exact and round to nearest is sign-symmetric, RN(-p) = -RN(p), so a flip
// of one factor moves through a rounded product: (s nx) root = nx (s root) and
// (u (s nx)) (s dot) = s s ((u nx) dot) = (u nx) dot, bit for bit, zero products included
// (the sign of a zero product is the xor of its factors' signs, which both sides share),
// and a NaN on one side is a NaN on the other (never stored: state_ok). dot * dot is
// |dot| |dot| likewise. So the raw normal, the signed dot and root_s = root with dot's sign
// bit give the same three sums in the same order; root >= 0 or NaN (sqrt_untested), so putting
// the bit on is the flip. dot == 0 and NaN take the exact path as before.
template <bool PLAIN = false, class B>
ORT_INLINE void refract(Ray& r, double nx, double ny, double nz, double u, double u_sq,
                        B& bad) {
  double dot, root;  // PLAIN: the signed dot and root_s; else |dot| and the root
  if constexpr (PLAIN) {
    dot = r.L * nx + r.M * ny + r.N * nz;
    ORT_CHK(bad, !(::fabs(dot) > 0.0));
    const double v = u_sq * (1.0 - dot * dot);
    root = with_sign_of(sqrt_untested(1.0 - v), dot);
  } else {
    dot = align_normal(r, nx, ny, nz, bad);
    const double v = u_sq * (1.0 - dot * dot);
    root = sqrt(1.0 - v, bad);
  }
  const double L0 = r.L, M0 = r.M, N0 = r.N;
  r.L = u * L0 + nx * root - u * nx * dot;
  r.M = u * M0 + ny * root - u * ny * dot;
  r.N = u * N0 + nz * root - u * nz * dot;
}

// Refraction at a flat surface: the plane normal (0, 0, 1) (plane.py:79-98) or the
// infinite-radius conic's (+-0, +-0, -1) (standard.py:154-167). For finite L, M and
// N != 0 the reference's expressions reduce exactly:
//   dot = L*0 + M*0 + N*1 = N, sign(dot) = sign(N), |dot| = |N|;
//   L' = u L + (+-0) root - u (+-0) |N| = u L + 0.0 (the zero terms only turn a -0
//   product into +0, as adding +0 does), M' likewise;
//   N' = (u N + sign(N) root) - (u sign(N)) |N| = (u N + sign(N) root) - u N.
// N == 0 / NaN takes the exact path; a non-finite L or M only reaches here on a ray that
// already failed a check (or came in non-finite, which closed_ray_in flags).
template <bool PLAIN = false, class B>
ORT_INLINE void refract_flat(Ray& r, double u, double u_sq, B& bad) {
  ORT_CHK(bad, !(::fabs(r.N) > 0.0));
  const double v = u_sq * (1.0 - r.N * r.N);
  double root;
  if constexpr (PLAIN)
    root = sqrt_untested(1.0 - v);
  else
    root = sqrt(1.0 - v, bad);
  const double uN = u * r.N;
  const double sroot = ::copysign(root, r.N);
  r.L = u * r.L + 0.0;
  r.M = u * r.M + 0.0;
  r.N = (uN + sroot) - uN;
}

// ---- Newton geometries (trace_kernel's deferred-check pass) --------------------------
// The quotient for a divisor of either sign with a numerator that may be +-0: IEEE's
// signed zero is quot_pos's for b > 0 and the plain form's for b < 0 (see quot_pos)
ORT_INLINE double quot_signed(double a, const Div& d) {
  return d.b > 0.0 ? quot_pos(a, d) : quot(a, d);
}
// numerator in range or an exact zero of either sign (quot_signed / quot_pos keep its sign)
ORT_INLINE bool num_ok0(double a) { return num_ok(a) || a == 0.0; }

// The asphere formulas divide by R (1 + q) and R q with q = sqrt(...) >= 0: the sign of a
// nonzero divisor is the radius's, a lens constant. With sR = +-1 that sign and the
// divisor's magnitude |R| (1 + q), |R| q (the same products: IEEE multiplication is
// sign-symmetric), a / b = (sR a) / |b| is quot_pos's form on a positive divisor -- the
// same IEEE quotient, signed zeros included (sR a flips an exact zero's sign exactly when
// b < 0) -- without quot_signed's two quotients and select. A zero divisor (q = 0)
// gives an infinite reciprocal and non-finite quotients, as the signed form does.
// |R| <= 2^149 (so |R| (1 + q) <= 2^150, R^2 <= 2^298: inside shared_div's range) is
// tested once per evaluation (lens_range) instead of a test per divisor
// (shared_div_untested).
ORT_INLINE bool lens_range(double R) { return ::fabs(R) <= 0x1p149; }

// kSlope's direct slopes (ort_core.h): norm^2 < 1e28 checked (a steeper normal or NaN
// takes the exact path, which forms the reference's expression from the unit normal)
ORT_INLINE void slope_out(double dfdx, double dfdy, double& nx, double& ny, double& nz,
                          bool& bad) {
  // (two compares, |dfdx|, |dfdy| < 7e13, give the same guarantee: no measurable gain on
  // the MI355X, profiles/r06_ab_slopemax.log, r06_ab_c3_slope_opk.log)
  ORT_CHK(bad, !(dfdx * dfdx + dfdy * dfdy + 1.0 < 1e28));
  nx = dfdx;
  ny = dfdy;
  nz = -1.0;
}

// the unit normal (dz/dx, dz/dy, -1) / norm from kSlope's direct slopes (norm^2 < 1e28
// checked by slope_out), and the tail of sagnorm_even's and sagnorm_odd's kNormal mode
ORT_INLINE void unit_normal_from_slope(double dfdx, double dfdy, double& nx, double& ny,
                                       double& nz, bool& bad) {
  const double mag = sqrt_untested(dfdx * dfdx + dfdy * dfdy + 1.0);  // >= 1
  const Div dm = shared_div_untested(mag);                             // a norm
  ORT_CHK(bad, !(num_ok0(dfdx) && num_ok0(dfdy)));
  nx = quot_pos(dfdx, dm);
  ny = quot_pos(dfdy, dm);
  nz = quot(-1.0, dm);
}

// even_asphere.py:82-129 (ort_core.h sagnorm_even): the same operations in the same order,
// the divisions and square roots as the deferred-check sequences; mode: kNormal or kSlope
template <class PD>
ORT_INLINE double sagnorm_even(double x, double y, const ort_surface& s, PD C,
                               int nc, int mode, double& nx, double& ny, double& nz,
                               bool& bad) {
  const double R = s.radius;
  const double aR = ::fabs(R), sR = R > 0.0 ? 1.0 : -1.0;  // (lens constants)
  ORT_CHK(bad, !lens_range(R));
  const double r2 = x * x + y * y;
  const double a = s.one_plus_k * r2;  // (1 + k) r2: +-0 at the vertex
  const Div rr = shared_div_untested(s.r_sq);
  ORT_CHK(bad, !num_ok0(a));
  const double q = sqrt(1.0 - quot_pos(a, rr), bad);
  const Div dz = shared_div_untested(aR * (1.0 + q));
  ORT_CHK(bad, !num_ok0(r2));
  double P, D;  // the term sums by Horner in r2 (ort_core.h even_horner)
  ort::even_horner(r2, C, nc, P, D);
  const double z = quot_pos(sR * r2, dz) + r2 * P;
  const Div dd = shared_div_untested(aR * q);
  ORT_CHK(bad, !(num_ok0(x) && num_ok0(y)));
  double dfdx = quot_pos(sR * x, dd);
  double dfdy = quot_pos(sR * y, dd);
  dfdx = dfdx + x * D;
  dfdy = dfdy + y * D;
  if (mode == kSlope) {
    slope_out(dfdx, dfdy, nx, ny, nz, bad);
    return z;
  }
  unit_normal_from_slope(dfdx, dfdy, nx, ny, nz, bad);
  return z;
}

// odd_asphere.py:73-130 (ort_core.h sagnorm_odd); non-finite per-term slopes zeroed
template <class PD>
ORT_INLINE double sagnorm_odd(double x, double y, const ort_surface& s, PD C,
                              int nc, int mode, double& nx, double& ny, double& nz,
                              bool& bad) {
  const double R = s.radius;
  const double aR = ::fabs(R), sR = R > 0.0 ? 1.0 : -1.0;  // (lens constants)
  ORT_CHK(bad, !lens_range(R));
  const double r2 = x * x + y * y;
  const double r = sqrt(r2, bad);  // the vertex itself (r2 = 0) takes the exact path
  const double a = s.one_plus_k * r2;
  const Div rr = shared_div_untested(s.r_sq);
  ORT_CHK(bad, !num_ok0(a));
  const double q = sqrt(1.0 - quot_pos(a, rr), bad);
  const Div dz = shared_div_untested(aR * (1.0 + q));
  ORT_CHK(bad, !num_ok0(r2));
  double z = quot_pos(sR * r2, dz);
  double rp = r;
  for (int i = 0; i < nc; ++i) {
    z = z + C[i] * rp;
    rp = rp * r;
  }
  const Div dd = shared_div_untested(aR * q);
  ORT_CHK(bad, !(num_ok0(x) && num_ok0(y)));
  double dfdx = quot_pos(sR * x, dd);
  double dfdy = quot_pos(sR * y, dd);
  const Div dr = shared_div(r, bad);
  double rq = quot_pos(1.0, dr);  // 1 / r
  for (int i = 0; i < nc; ++i) {
    const double f = (double)(i + 1);
    double xt = f * x * C[i] * rq;
    double yt = f * y * C[i] * rq;
    if (!isfinite(xt)) xt = 0.0;
    if (!isfinite(yt)) yt = 0.0;
    rq = (i == 0) ? 1.0 : (i == 1 ? r : rq * r);
    dfdx = dfdx + xt;
    dfdy = dfdy + yt;
  }
  if (mode == kSlope) {
    slope_out(dfdx, dfdy, nx, ny, nz, bad);
    return z;
  }
  unit_normal_from_slope(dfdx, dfdy, nx, ny, nz, bad);
  return z;
}

// newton_raphson.py:154-166 from kSlope's slopes (ort_core.h newton_step_slope)
ORT_INLINE double newton_step_slope(const Ray& r, double t, double f, double fx, double fy,
                                    bool& bad) {
  const double df = fx * r.L + fy * r.M - r.N;
  const double dfs = ::fabs(df) > 1e-14 ? df : 1e-14;
  const Div dd = shared_div(dfs, bad);
  ORT_CHK(bad, !num_ok0(f));
  return t - quot_signed(f, dd);
}

// newton_raphson.py:154-166 (ort_core.h newton_step)
ORT_INLINE double newton_step(const Ray& r, double t, double f, double nx, double ny,
                              double nz, bool& bad) {
  const double nzs = ::fabs(nz) > 1e-14 ? nz : 1e-14;
  const Div dn = shared_div(nzs, bad);
  const double mnx = -nx, mny = -ny;
  ORT_CHK(bad, !(num_ok0(mnx) && num_ok0(mny)));
  const double fx = quot_signed(mnx, dn);
  const double fy = quot_signed(mny, dn);
  const double df = fx * r.L + fy * r.M - r.N;
  const double dfs = ::fabs(df) > 1e-14 ? df : 1e-14;
  const Div dd = shared_div(dfs, bad);
  ORT_CHK(bad, !num_ok0(f));
  return t - quot_signed(f, dd);
}

}  // namespace fast
}  // namespace ort
