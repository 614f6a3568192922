// ort_host.cpp -- the host (CPU) build of the trace core behind include/optiland_host.h:
// the CPU dispatch key of torch.ops.ort.trace_sequential and of its VJP.
//
// Compiled with g++ -O2 -ffp-contract=off -fopenmp (optiland_pr_amd/build.py), from the
// same sources as the HIP kernels: the per-ray arithmetic (ort_core.h, ort_interact.h,
// ort_material.h, ort_polar.h), the argument unpacking, the surface step after the distance
// (interact, pol_step) and the VJP front end (ort_args.h), and the derivative sweeps
// (ort_sweep.h) -- so every value is the GPU's and an argument is checked by the code that
// checks it there. What is host-specific is the control around the per-ray code:
//   * Newton surfaces: the reference's global stop rule (newton_raphson.py:137-166, the
//     test max |f| < tol over every ray of the call, NaN never passing; grid_sag.py:108-140
//     the test max |dt| < tol after each update) evaluated directly, the rays of one Newton
//     group stepped in lockstep the way the reference evaluates them -- no speculate /
//     verify schedule as on the GPU;
//   * the surface step after the distance is the interaction kernels' general path
//     (trace_kernel<F_IA>: propagate, normalise after a thin lens, OPD, clip, interact,
//     globalize, record), which for refractive / reflective surfaces is finish_surface;
//   * the VJPs run adj_ray / vjp_ray per ray with a host lane (ray-local tape, per-chunk
//     slot accumulators) and reduce the chunks in index order; the refusals only this
//     library makes are named in host_vjp_run;
//   * one specialisation with every Newton kind compiled in (kAllKinds).
#define ORT_HD
#include "../../include/optiland_host.h"

#include <omp.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "ort_dft.h"
#include "ort_huygens.h"
#include "ort_irradiance.h"
#include "ort_sampled_otf.h"
#include "ort_sweep.h"

namespace {

using namespace ortk;
using ort::Ray;

constexpr int64_t kChunk = 256;  // rays per reduction chunk (the GPU's block)
constexpr int64_t kParMin = 2048;  // below this many rays a phase runs on one thread

int g_threads = 0;

int threads_for(int64_t n) {
  if (n < kParMin) return 1;
  return g_threads > 0 ? g_threads : omp_get_max_threads();
}

ort_surface_optics optics_of(const KArgs& a, const ort_surface& s, int si, int lam, double wl) {
  return a.w ? optics_ray(a, s, wl) : optics_row(a, lam, si);
}

// One reference trace call: rays [r0, r1) of the batch (one Newton group).
void trace_group(const KArgs& a, int64_t r0, int64_t r1, int32_t* updates, int& status) {
  const int64_t n = r1 - r0;
  const int nt = threads_for(n);
  std::vector<Ray> rays(n);
  std::vector<int> lam(n, 0);
  std::vector<double> wl(n, 0.0), t(n), f, nx, ny, nz;
  std::vector<char> unnorm(n, 0);
  std::vector<ort::PolState> pol(a.coat ? n : 0);  // ort_host_trace_*_polarized
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int64_t k = 0; k < n; ++k) {
    const int64_t r = r0 + k;
    if (a.seg) lam[k] = a.seg[a.n_seg == 1 ? 0 : r / a.seg_len].lambda_idx;
    if (a.w) wl[k] = a.w[r];
    Ray& q = rays[k];
    load_ray(a, r, q);
    if (a.coat) ort::pol_init(pol[k], q.L, q.M, q.N, q.i);
  }
  for (int si = a.start_surface; si < a.n_surf; ++si) {
    const ort_surface s = a.surf[si];
    if (updates) updates[si] = 0;
    const bool known = known_geometry(s.geometry);
    if (!known) status |= ORT_STATUS_BAD_GEOMETRY;
    const bool grid = s.geometry == ORT_GEOM_GRID_SAG;
    // localize and the closed-form distance (the Newton kinds' initial guess)
#pragma omp parallel for num_threads(nt) schedule(static)
    for (int64_t k = 0; k < n; ++k) {
      localize(a, s, rays[k]);
      if (!known)
        t[k] = __builtin_nan("");
      else if (s.geometry == ORT_GEOM_PLANE)
        t[k] = ort::distance_plane(rays[k]);
      else if (grid)
        t[k] = 0.0;  // grid_sag.py:110
      else if (s.geometry == ORT_GEOM_NURBS)  // per-ray (u, v) solve (ort_nurbs.h)
        t[k] = ort::nurbs_distance(ort::nurbs_view(a.coef + s.coef_off), s.tol, s.max_iter,
                                   rays[k]);
      else
        t[k] = ort::distance_conic(rays[k], s.radius, s.conic,
                                   (s.flags & ORT_SURF_RADIUS_INF) != 0);
    }
    if (known && grid) {
      // grid_sag.py:111-140: t += dt until max |dt| < tol over the call (NaN: never)
      const ort::GridView g = ort::grid_view(a.coef + s.coef_off);
      int j = 0;
      while (j < s.max_iter) {
        double dmax = 0.0;
        int nan = 0;
#pragma omp parallel for num_threads(nt) schedule(static) reduction(max : dmax) reduction(| : nan)
        for (int64_t k = 0; k < n; ++k) {
          const double dt = ort::grid_step(g, rays[k], t[k]);
          t[k] = t[k] + dt;
          const double ad = fabs(dt);
          if (ad != ad)
            nan = 1;
          else if (ad > dmax)
            dmax = ad;
        }
        ++j;
        if (!nan && dmax < s.tol) break;
      }
#pragma omp parallel for num_threads(nt) schedule(static)
      for (int64_t k = 0; k < n; ++k) t[k] = ort::grid_final(g, rays[k], t[k]);
      if (updates) updates[si] = j;
    } else if (known && scheduled_geometry(s.geometry)) {
      // newton_raphson.py:137-166: stop when max |f| < tol over the whole call
      f.resize(n);
      nx.resize(n);
      ny.resize(n);
      nz.resize(n);
      int j = 0;
      for (;; ++j) {
        double fmax = 0.0;
        int nan = 0, rbits = 0;
        const int rb = range_bit(s);
#pragma omp parallel for num_threads(nt) schedule(static) reduction(max : fmax) reduction(| : nan, rbits)
        for (int64_t k = 0; k < n; ++k) {
          bool rerr = false;
          f[k] = ort::newton_eval<kAllKinds>(s, s.radius, s.conic, a.coef, a.zern, kNoSeed,
                                             rays[k], t[k], ort::kSlope, rerr, nx[k], ny[k],
                                             nz[k]);
          // the reference evaluates the sag at j = 0 .. max_iter - 1 only
          if (rerr && j < s.max_iter) rbits |= rb;
          const double v = fabs(f[k]);
          if (v != v)
            nan = 1;
          else if (v > fmax)
            fmax = v;
        }
        status |= rbits;
        if (j >= s.max_iter || (!nan && fmax < s.tol)) break;
#pragma omp parallel for num_threads(nt) schedule(static)
        for (int64_t k = 0; k < n; ++k)
          t[k] = ort::newton_step_any(rays[k], t[k], f[k], nx[k], ny[k], nz[k]);
      }
      if (updates) updates[si] = j;
    }
    // the rest of Surface.trace (standard_surface.py:215-231) and the record (:266-286)
#pragma omp parallel for num_threads(nt) schedule(static)
    for (int64_t k = 0; k < n; ++k) {
      Ray& r = rays[k];
      const ort_surface_optics o = optics_of(a, s, si, lam[k], wl[k]);
      ort::propagate(r, t[k], o.alpha_pre);
      if (unnorm[k]) {  // homogeneous.py:55-57
        ort::normalize_dir(r);
        unnorm[k] = 0;
      }
      ort::add_opd(r, t[k], o.n_pre);
      if (s.flags & ORT_SURF_APERTURE) ort::clip_radial(r, s.ap_rmax2, s.ap_rmin2);
      if (s.flags & ORT_SURF_APERTURE_PROG) ort::clip_program(r, a.coef + s.ap_off, s.ap_len);
      bool un = false;
      if (a.coat) {  // trace_kernel<F_POL>'s step (refractive / reflective surfaces only)
        double ux, uy, uz;
        pol_step<kAllKinds>(a, s, o, si, lam[k], r, pol[k], false, ux, uy, uz);
      } else if (a.bsdf) {  // trace_kernel<F_SCAT>'s step
        double ux, uy, uz;
        const int bits = scat_step<kAllKinds>(a, s, o, si, r0 + k, r, false, ux, uy, uz);
        if (bits) {
#pragma omp atomic
          status |= bits;
        }
      } else if (a.w)
        interact<kAllKinds, true>(a, s, r, o, lam[k], wl[k], un);
      else
        interact<kAllKinds, false>(a, s, r, o, lam[k], wl[k], un);
      if (un) unnorm[k] = 1;
      globalize(a, s, r);
      if (a.rec && (s.flags & ORT_SURF_RECORD)) store_record<PlainStore>(a, s, r0 + k, r);
    }
  }
  // real_ray_tracer.py:84-89: image-space propagate (final_mat < 0: none)
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int64_t k = 0; k < n; ++k) {
    Ray& r = rays[k];
    if (a.final_mat >= 0) {
      const double alpha =
          a.w ? ort::absorption_alpha(ort::material_k(a.mats[a.final_mat], a.coef, wl[k]), wl[k])
              : tab(a.alpha_tab, a.n_lambda, a.n_mat, lam[k], a.final_mat);
      ort::propagate(r, a.final_thickness, alpha);
      if (unnorm[k]) ort::normalize_dir(r);
    }
    const int64_t q = r0 + k;
    if (!a.coat) {
      store_ray<PlainStore>(a, q, r);
    } else {
      const double inten =
          ort::pol_intensity(pol[k], a.pol_mode, a.pol_ex, a.pol_ey, ort::intensity(r));
      store_ray<PlainStore>(a, q, r, &inten);
      if (a.p_out) {
        for (int e = 0; e < 9; ++e) {
          a.p_out[(int64_t)(2 * e) * a.n_rays + q] = pol[k].re[e];
          a.p_out[(int64_t)(2 * e + 1) * a.n_rays + q] = pol[k].im[e];
        }
      }
    }
  }
}

// adj_ray's lane policy on the host (ort_sweep.h): one ray at a time, its tape in a
// ray-local array of at most S kTapeRows rows (stride 1), slot contributions added to the chunk's
// accumulator acc[slot] in the ray's order
struct HostLane {
  const AArgs& j;
  double* acc;
  double* tp;
  void emit(int slot, double v, bool) {
    if (j.need[slot]) acc[slot] += v;
  }
  double* tape_at(int64_t row) const { return tp + row; }
  int64_t tape_stride() const { return 1; }
  int uniform_max(int v) const { return v; }
  void mono_put(int base, int i, double v) { acc[base + i] += v; }
  void mono_flush(int, int) {}
};

template <uint32_t KM, int P, bool RES = true>
void adj_chunks(const KArgs& a, const AArgs& j, std::vector<double>& part, int64_t n_chunk) {
  const int nt = threads_for(a.n_rays);
#pragma omp parallel num_threads(nt)
  {
    std::vector<double> tape((size_t)a.n_surf * kTapeRows);
#pragma omp for schedule(static)
    for (int64_t c = 0; c < n_chunk; ++c) {
      double* acc = part.data() + c * j.n_slot;
      HostLane ln{j, acc, tape.data()};
      const int64_t e = std::min(a.n_rays, (c + 1) * kChunk);
      for (int64_t rid = c * kChunk; rid < e; ++rid) adj_ray<KM, P, RES>(a, j, ln, rid, true);
    }
  }
}

template <uint32_t KM>
void vjp_chunks(const KArgs& a, const JArgs& j, std::vector<double>& part, int64_t n_chunk) {
  const int nt = threads_for(a.n_rays);
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int64_t c = 0; c < n_chunk; ++c) {
    double* sums = part.data() + c * 4;
    for (int k = 0; k < 4; ++k) sums[k] = 0.0;
    const int64_t e = std::min(a.n_rays, (c + 1) * kChunk);
    for (int64_t rid = c * kChunk; rid < e; ++rid) {
      double acc[4];
      vjp_ray<4, KM>(a, j, rid, true, acc);
      for (int k = 0; k < 4; ++k) sums[k] += acc[k];
    }
  }
}

}  // namespace

// every Newton group of the batch through trace_group (updates: [n_groups][n_surfaces])
static int trace_groups(const KArgs& a, int32_t* updates, int32_t* status, int st) {
  const int64_t n_groups = (a.n_rays + a.group_len - 1) / a.group_len;
  for (int64_t g = 0; g < n_groups; ++g) {
    const int64_t r0 = g * a.group_len, r1 = std::min(a.n_rays, r0 + a.group_len);
    int32_t* up = updates ? updates + g * a.n_surf : nullptr;
    if (up)
      for (int s = 0; s < a.n_surf; ++s) up[s] = 0;
    trace_group(a, r0, r1, up, st);
  }
  if (status) *status = st;
  return ORT_OK;
}

// sum of term(k), lo <= k < hi: halves down to runs of at most 8 terms added in order
template <class F>
static double pairwise_sum(int64_t lo, int64_t hi, const F& term) {
  if (hi - lo <= 8) {
    double s = 0.0;
    for (int64_t k = lo; k < hi; ++k) s += term(k);
    return s;
  }
  const int64_t mid = lo + (hi - lo) / 2;
  return pairwise_sum(lo, mid, term) + pairwise_sum(mid, hi, term);
}

extern "C" {

int ort_host_abi_version(void) { return ORT_HOST_ABI_VERSION; }

void ort_host_set_threads(int32_t n) { g_threads = n; }

// shared body of ort_host_trace_sequential and its polarized form (pol: NULL or the
// coatings / mode of ort_host_trace_sequential_polarized)
static int host_trace_sequential(const ort_lens* lens, const ort_rays* rays_in,
                                 ort_rays* rays_out, const ort_batch* batch,
                                 const ort_options* opt, double* rec, int32_t* updates,
                                 int32_t* status, const ort_polarization* pol,
                                 const ort_scatter* scat = nullptr) {
  if (!rays_in || !rays_out || !batch) return ORT_ERR_ARG;
  const ort_options dflt{ORT_NEWTON_SCHEDULE, 0, nullptr, 0, 0};
  if (!opt) opt = &dflt;
  if (opt->tape || opt->verify_stats || opt->run_if) return ORT_ERR_ARG;
  KArgs a{};
  uint32_t feat = 0;
  int rc = fill_args(a, lens, batch, opt, rec, nullptr, status, feat);
  if (rc) return rc;
  if (pol && (rc = fill_pol(a, batch, opt, pol, feat))) return rc;
  if (scat && (rc = fill_scat(a, batch, opt, scat, feat))) return rc;
  a.in = *rays_in;
  a.out = *rays_out;
  if (status) *status = 0;
  if (a.n_rays == 0) return ORT_OK;
  return trace_groups(a, updates, status, 0);
}

int ort_host_trace_sequential(const ort_lens* lens, const ort_rays* rays_in,
                              ort_rays* rays_out, const ort_batch* batch,
                              const ort_options* opt, double* rec, int32_t* updates,
                              int32_t* status) {
  return host_trace_sequential(lens, rays_in, rays_out, batch, opt, rec, updates, status,
                               nullptr);
}

int ort_host_trace_sequential_polarized(const ort_lens* lens, const ort_rays* rays_in,
                                        ort_rays* rays_out, const ort_batch* batch,
                                        const ort_options* opt, double* rec, int32_t* updates,
                                        int32_t* status, const ort_polarization* pol) {
  if (!pol) return ORT_ERR_ARG;
  return host_trace_sequential(lens, rays_in, rays_out, batch, opt, rec, updates, status, pol);
}

int ort_host_trace_sequential_scatter(const ort_lens* lens, const ort_rays* rays_in,
                                      ort_rays* rays_out, const ort_batch* batch,
                                      const ort_options* opt, double* rec, int32_t* updates,
                                      int32_t* status, const ort_scatter* scat) {
  if (!scat) return ORT_ERR_ARG;
  return host_trace_sequential(lens, rays_in, rays_out, batch, opt, rec, updates, status,
                               nullptr, scat);
}

int ort_host_bsdf_scatter(const double* L, const double* M, const double* N, const double* nx,
                          const double* ny, const double* nz, int64_t n, int32_t surface_index,
                          const ort_bsdf* bsdf, const ort_scatter* scat, double* out_L,
                          double* out_M, double* out_N, int32_t* status) {
  if (!bsdf || !scat || n < 0 || surface_index < 0) return ORT_ERR_ARG;
  if (bsdf->kind != ORT_BSDF_LAMBERTIAN && bsdf->kind != ORT_BSDF_GAUSSIAN) return ORT_ERR_ARG;
  if (scat->max_attempts < 1 || scat->ray_offset < 0) return ORT_ERR_ARG;
  if (status) *status = 0;
  if (n == 0) return ORT_OK;
  if (!L || !M || !N || !nx || !ny || !nz || !out_L || !out_M || !out_N) return ORT_ERR_ARG;
  int st = 0;
  const int nt = threads_for(n);
#pragma omp parallel for num_threads(nt) schedule(static) reduction(| : st)
  for (int64_t r = 0; r < n; ++r) {
    double l = L[r], m = M[r], k = N[r];
    if (!ort::bsdf_scatter(*bsdf, scat->seed, (uint64_t)(r + scat->ray_offset),
                           (uint32_t)surface_index, scat->max_attempts, nx[r], ny[r], nz[r], l,
                           m, k))
      st |= ORT_STATUS_SCATTER_ATTEMPTS;
    out_L[r] = l;
    out_M[r] = m;
    out_N[r] = k;
  }
  if (status) *status = st;
  return ORT_OK;
}

}  // extern "C"

namespace {

// Shared body of the two host VJP entry points: resident rays (rays_in, resident = true) or
// rays generated from pupil samples (px, py, the batch's segments: ort_trace_pupil_vjp's
// counterpart). The checks and assignments the device library makes too are ort_args.h's
// front end (vjp_check_call, vjp_prepare, vjp_fill_*); what follows them here is the
// host's own: the need[] flags, the chunk loops and reductions, and the refusals marked
// "host only".
int host_vjp_run(const ort_lens* lens, const double* px, const double* py,
                 const ort_rays* rays_in, bool resident, const ort_batch* batch,
                 const ort_options* opt, const ort_vjp_params* params,
                 const ort_rays* cotangent, const double* rec_cotangent, const double* rec,
                 double* grad, const ort_rays* grad_in) {
  bool want_in = false, nothing = false;
  int rc = vjp_check_call(batch, params, cotangent, grad, grad_in, want_in, nothing);
  if (rc) return rc;
  // host only: the options and the rays are required of an empty call too (the device
  // library returns ORT_OK for one before it looks at them)
  if (!opt || !vjp_inputs_ok(resident, rays_in, px, py, batch)) return ORT_ERR_ARG;
  const int32_t n_param = params->n_param;
  // host only: an overwritten gradient is zeroed here, before anything is traced, and the
  // sums below accumulate (the device zeroes it in the empty return and otherwise hands
  // grad_init to its reduce kernels: the same outcome)
  if (params->grad_init)
    for (int p = 0; p < n_param; ++p) grad[p] = 0.0;
  if (nothing) return ORT_OK;
  // host only: no tape -- the trace writes none (opt->tape) and the adjoint always replays
  // the forward (params->tape); the device library takes both
  if (opt->tape || params->tape) return ORT_ERR_ARG;
  // host only: a generated-ray VJP starts at the first surface (the device library replays
  // from opt->start_surface)
  if (!resident && opt->start_surface) return ORT_ERR_ARG;
  KArgs a{};
  uint32_t feat = 0;
  if ((rc = vjp_prepare(a, feat, lens, px, py, rays_in, resident, batch, opt, params,
                        rec_cotangent, rec)))
    return rc;
  // (host only by omission: opt->newton_mode is not looked at -- the sweeps replay
  // opt->sched or the surfaces' max_iter -- and a lens past the device's LDS slot limit,
  // ORT_VJP_ADJOINT_MAX_SLOTS, is served in adjoint mode.)
  const int64_t n_chunk = (a.n_rays + kChunk - 1) / kChunk;
  if (params->mode == ORT_VJP_ADJOINT) {
    AArgs j{};
    if ((rc = vjp_fill_adjoint(j, lens, params, cotangent, rec_cotangent, rec, grad, grad_in,
                               want_in)))
      return rc;
    j.mono_on = mono_enabled(j);
    // (rms_stats / rms_grad: the forward is replayed, so the final point is the traced state)
    std::vector<int32_t> need(j.n_slot, 0);
    for (int slot = 0; slot < j.n_slot; ++slot) {
      if (params->slot_need) {
        need[slot] = params->slot_need[slot] != 0;
      } else {
        for (int p = 0; p < n_param && !need[slot]; ++p) need[slot] = slot_weight(j, slot, p) != 0.0;
      }
    }
    j.need = need.data();
    std::vector<double> part((size_t)n_chunk * j.n_slot, 0.0);
    if (params->surf_tangent)
      resident ? adj_chunks<kAllKinds, 4, true>(a, j, part, n_chunk)
               : adj_chunks<kAllKinds, 4, false>(a, j, part, n_chunk);
    else
      resident ? adj_chunks<kAllKinds, 2, true>(a, j, part, n_chunk)
               : adj_chunks<kAllKinds, 2, false>(a, j, part, n_chunk);
    // grad[p] += sum over slots of d slot / d p * (the chunks' sums in index order)
    std::vector<double> slot_sum(j.n_slot, 0.0);
    for (int slot = 0; slot < j.n_slot; ++slot) {
      if (!need[slot]) continue;
      double v = 0.0;
      for (int64_t c = 0; c < n_chunk; ++c) v += part[(size_t)c * j.n_slot + slot];
      slot_sum[slot] = v;
    }
    for (int p = 0; p < n_param; ++p) {
      double g = 0.0;
      for (int slot = 0; slot < j.n_slot; ++slot) {
        const double w = need[slot] ? slot_weight(j, slot, p) : 0.0;
        if (w != 0.0) g += slot_sum[slot] * w;
      }
      grad[p] += g;
    }
    return ORT_OK;
  }
  if (params->mode != ORT_VJP_UNROLLED) return ORT_ERR_ARG;
  JArgs j{};
  if ((rc = vjp_fill_unrolled(j, params, cotangent, rec_cotangent, grad, want_in))) return rc;
  std::vector<double> part((size_t)n_chunk * 4);
  for (int p0 = 0; p0 < n_param; p0 += 4) {
    j.p0 = p0;
    vjp_chunks<kAllKinds>(a, j, part, n_chunk);
    for (int k = 0; k < 4 && p0 + k < n_param; ++k) {
      double v = 0.0;
      for (int64_t c = 0; c < n_chunk; ++c) v += part[(size_t)c * 4 + k];
      grad[p0 + k] += v;
    }
  }
  return ORT_OK;
}

// rays of a pupil trace generated on the host (ray_generator.py:28-106 via ort::generate_ray,
// the GPU's source): ray r of segment r / seg_len at pupil sample r (pupil_per_ray) or
// r - segment * seg_len
void generate_host(const KArgs& a, const double* px, const double* py, std::vector<double>& buf,
                   ort_rays& rays) {
  const int64_t n = a.n_rays;
  buf.assign((size_t)n * 8, 0.0);
  double* f[8];
  for (int k = 0; k < 8; ++k) f[k] = buf.data() + (size_t)k * n;
  rays = ort_rays{f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7]};
  const int nt = threads_for(n);
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int64_t r = 0; r < n; ++r) {
    const int64_t sidx = r / a.seg_len;
    const ort_segment sg = a.seg[sidx];
    const int64_t p = a.pupil_per_ray ? r : r - sidx * a.seg_len;
    const Ray q = ort::generate_ray(sg, px[p], py[p], a.apod);
    f[0][r] = q.x;
    f[1][r] = q.y;
    f[2][r] = q.z;
    f[3][r] = q.L;
    f[4][r] = q.M;
    f[5][r] = q.N;
    f[6][r] = ort::intensity(q);
    f[7][r] = q.opd;
  }
}

}  // namespace

extern "C" {

int ort_host_trace_sequential_vjp(const ort_lens* lens, const ort_rays* rays_in,
                                  const ort_batch* batch, const ort_options* opt,
                                  const ort_vjp_params* params, const ort_rays* cotangent,
                                  const double* rec_cotangent, const double* rec,
                                  double* grad, const ort_rays* grad_in) {
  return host_vjp_run(lens, nullptr, nullptr, rays_in, true, batch, opt, params, cotangent,
                      rec_cotangent, rec, grad, grad_in);
}

// shared body of ort_host_trace_pupil and its polarized form
static int host_trace_pupil(const ort_lens* lens, const double* px, const double* py,
                            ort_rays* rays_out, const ort_batch* batch, const ort_options* opt,
                            double* rec, int32_t* updates, int32_t* status,
                            const ort_polarization* pol, const ort_scatter* scat = nullptr) {
  if (!px || !py || !rays_out || !batch || !batch->seg || batch->n_seg < 1 || batch->w)
    return ORT_ERR_ARG;
  const ort_options dflt{ORT_NEWTON_SCHEDULE, 0, nullptr, 0, 0};
  if (!opt) opt = &dflt;
  if (opt->tape || opt->verify_stats || opt->run_if || opt->start_surface) return ORT_ERR_ARG;
  KArgs a{};
  uint32_t feat = 0;
  int rc = fill_args(a, lens, batch, opt, rec, nullptr, status, feat);
  if (rc) return rc;
  if (pol && (rc = fill_pol(a, batch, opt, pol, feat))) return rc;
  if (scat && (rc = fill_scat(a, batch, opt, scat, feat))) return rc;
  if (batch->n_rays != (int64_t)batch->n_seg * batch->seg_len) return ORT_ERR_ARG;
  a.out = *rays_out;
  if (status) *status = 0;
  if (a.n_rays == 0) return ORT_OK;
  std::vector<double> buf;
  ort_rays gen;
  generate_host(a, px, py, buf, gen);
  a.in = gen;
  int st = 0;
  if (a.apod && (uint32_t)a.apod->kind > (uint32_t)ORT_APOD_TUKEY) st |= ORT_STATUS_BAD_APODIZATION;
  return trace_groups(a, updates, status, st);
}

int ort_host_trace_pupil(const ort_lens* lens, const double* px, const double* py,
                         ort_rays* rays_out, const ort_batch* batch, const ort_options* opt,
                         int32_t* updates, int32_t* status) {
  return host_trace_pupil(lens, px, py, rays_out, batch, opt, nullptr, updates, status, nullptr);
}

int ort_host_trace_pupil_polarized(const ort_lens* lens, const double* px, const double* py,
                                   ort_rays* rays_out, const ort_batch* batch,
                                   const ort_options* opt, double* rec, int32_t* updates,
                                   int32_t* status, const ort_polarization* pol) {
  if (!pol) return ORT_ERR_ARG;
  return host_trace_pupil(lens, px, py, rays_out, batch, opt, rec, updates, status, pol);
}

int ort_host_trace_pupil_scatter(const ort_lens* lens, const double* px, const double* py,
                                 ort_rays* rays_out, const ort_batch* batch,
                                 const ort_options* opt, double* rec, int32_t* updates,
                                 int32_t* status, const ort_scatter* scat) {
  if (!scat) return ORT_ERR_ARG;
  return host_trace_pupil(lens, px, py, rays_out, batch, opt, rec, updates, status, nullptr,
                          scat);
}

int ort_host_generate_rays(const double* px, const double* py, ort_rays* rays_out,
                           const ort_batch* batch) {
  if (!rays_out || !batch) return ORT_ERR_ARG;
  if (batch->n_rays == 0) return ORT_OK;
  if (!px || !py || !batch->seg || batch->seg_len < 1 || batch->n_rays < 0) return ORT_ERR_ARG;
  KArgs a{};
  a.n_rays = batch->n_rays;
  a.seg_len = batch->seg_len;
  a.seg = batch->seg;
  a.pupil_per_ray = batch->pupil_per_ray;
  a.apod = batch->apod;
  std::vector<double> buf;
  ort_rays gen;
  generate_host(a, px, py, buf, gen);
  const double* src[8] = {gen.x, gen.y, gen.z, gen.L, gen.M, gen.N, gen.i, gen.opd};
  double* dst[8] = {rays_out->x, rays_out->y, rays_out->z, rays_out->L,
                    rays_out->M, rays_out->N, rays_out->i, rays_out->opd};
  for (int k = 0; k < 8; ++k)
    if (dst[k]) std::copy(src[k], src[k] + a.n_rays, dst[k]);
  return ORT_OK;
}

int ort_host_trace_pupil_vjp(const ort_lens* lens, const double* px, const double* py,
                             const ort_batch* batch, const ort_options* opt,
                             const ort_vjp_params* params, const ort_rays* cotangent,
                             double* grad) {
  return host_vjp_run(lens, px, py, nullptr, false, batch, opt, params, cotangent, nullptr,
                      nullptr, grad, nullptr);
}

// RayOperand.rms_spot_size (optimization/operand/ray.py:300-340) on host memory: the mean
// of x and y over all n points, then sqrt(mean((x - mx)^2 + (y - my)^2)); pairwise sums
// (halves down to runs of 8 terms, a chain of 8 + log2(n / 8) additions: a running sum's
// error grows with sqrt(n) and at 65,537 points 20 mm off axis passed the device tree's
// bound, tests/test_reductions_cpu.py; one thread: no thread count in the value). stats:
// n, mean x, mean y, rms, max radius (the ort_rms_spot layout; n = 0: count 0, the rest NaN).
int ort_host_rms_spot(const double* x, const double* y, int64_t n, double* stats, double* rms) {
  if (n < 0 || !stats || !rms || (n > 0 && (!x || !y))) return ORT_ERR_ARG;
  const double sx = pairwise_sum(0, n, [&](int64_t k) { return x[k]; });
  const double sy = pairwise_sum(0, n, [&](int64_t k) { return y[k]; });
  const double mx = sx / (double)n, my = sy / (double)n;
  const double s2 = pairwise_sum(0, n, [&](int64_t k) {
    const double dx = x[k] - mx, dy = y[k] - my;
    return dx * dx + dy * dy;
  });
  double rmax = 0.0;
  for (int64_t k = 0; k < n; ++k) {
    const double dx = x[k] - mx, dy = y[k] - my;
    const double r = sqrt(dx * dx + dy * dy);
    if (r > rmax || r != r) rmax = r;
  }
  const double v = sqrt(s2 / (double)n);
  stats[0] = (double)n;
  stats[1] = mx;
  stats[2] = my;
  stats[3] = v;
  stats[4] = n > 0 ? rmax : v;  // no point: NaN like the rest (0 / 0), as ort_rms_spot's row
  *rms = v;
  return ORT_OK;
}

// its VJP: d rms / d (x_k, y_k) = (x_k - mx, y_k - my) / (n rms), times grad_out
int ort_host_rms_spot_vjp(const double* x, const double* y, int64_t n, const double* stats,
                          const double* grad_out, double* gx, double* gy) {
  if (n < 0 || !stats || !grad_out || (n > 0 && (!x || !y || !gx || !gy))) return ORT_ERR_ARG;
  const double mx = stats[1], my = stats[2];
  const double s = grad_out[0] / (stats[0] * stats[3]);
  for (int64_t k = 0; k < n; ++k) {
    gx[k] = (x[k] - mx) * s;
    gy[k] = (y[k] - my) * s;
  }
  return ORT_OK;
}

// HuygensPSF's summation (psf/huygens_fresnel_strategies.py:97-172) on host memory: the
// kernel's term and its order of additions (ort_huygens.h, ort_k_huygens.hip), the image
// points split over OpenMP threads.
int ort_host_huygens_psf(const double* ix, const double* iy, const double* iz, int64_t n_image,
                         const double* px, const double* py, const double* pz,
                         const double* amp, const double* opd_mm, int64_t n_pupil,
                         double wavelength_mm, double rp, double* psf) {
  if (n_image < 0 || n_pupil < 0 || !(wavelength_mm > 0.0)) return ORT_ERR_ARG;
  if (n_image > 0 && (!ix || !iy || !iz || !psf)) return ORT_ERR_ARG;
  if (n_pupil > 0 && (!px || !py || !pz || !amp || !opd_mm)) return ORT_ERR_ARG;
  const double inv_wl = 1.0 / wavelength_mm, inv_rp = 1.0 / rp;
  // (one thread below kParMin terms, as the ray phases)
  const int nt = n_image < 2 ? 1 : threads_for(n_image * std::max<int64_t>(n_pupil, 1));
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int64_t p = 0; p < n_image; ++p) {
    double re = 0.0, im = 0.0;
    int64_t j0 = 0;
    do {  // (an empty pupil: one empty chunk, as the kernel's grid)
      const int64_t j1 = std::min<int64_t>(j0 + ORT_HUYGENS_CHUNK, n_pupil);
      double cr, ci;
      ort::huygens_chunk(ix[p], iy[p], iz[p], px, py, pz, amp, opd_mm, j0, j1, inv_wl, inv_rp,
                         cr, ci);
      re += cr;
      im += ci;
      j0 = j1;
    } while (j0 < n_pupil);
    psf[p] = re * re + im * im;
  }
  return ORT_OK;
}

// The FFT / MMDFT PSF transform (psf/mmdft.py:164-184, psf/fft.py:169-234) on host memory:
// the kernels' terms and their order of additions (ort_dft.h, ort_k_dft.hip). Per pupil the
// complex pupil g and the twiddles W(u - m/2, k - n/2) are formed once (the twiddles of stage
// B are the same family: W is symmetric in its arguments), then T = g R row by row and
// |R^T T|^2 row by row over OpenMP threads.
int ort_host_dft_psf(const double* amp, const double* opd_waves, int64_t batch, int64_t n,
                     int64_t m, double pad, double* out) {
  const int rc = dft_check(amp, opd_waves, batch, n, m, pad, out);
  if (rc != ORT_OK) return rc;
  if (batch == 0 || m == 0) return ORT_OK;
  const int64_t ipad = ort::dft_int_pad(pad), hn = n / 2, hm = m / 2;
  const int nt = threads_for(n * m * (n + m));
  std::vector<double> w(2 * m * n), g(2 * n * n), t(2 * n * m);  // W[u][k], g[j][k], T[j][u]
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int64_t u = 0; u < m; ++u)
    for (int64_t k = 0; k < n; ++k)
      ort::dft_twiddle(u - hm, k - hn, pad, ipad, w[2 * (u * n + k)], w[2 * (u * n + k) + 1]);
  for (int64_t b = 0; b < batch; ++b) {
    const double* am = amp + b * n * n;
    const double* op = opd_waves + b * n * n;
    double* o = out + b * m * m;
#pragma omp parallel for num_threads(nt) schedule(static)
    for (int64_t j = 0; j < n; ++j) {
      for (int64_t k = 0; k < n; ++k)
        ort::dft_pupil(am[j * n + k], op[j * n + k], g[2 * (j * n + k)], g[2 * (j * n + k) + 1]);
      for (int64_t u = 0; u < m; ++u) {
        double sr = 0.0, si = 0.0;
        for (int64_t k = 0; k < n; ++k)
          ort::dft_mac(g[2 * (j * n + k)], g[2 * (j * n + k) + 1], w[2 * (u * n + k)],
                       w[2 * (u * n + k) + 1], sr, si);
        t[2 * (j * m + u)] = sr;
        t[2 * (j * m + u) + 1] = si;
      }
    }
#pragma omp parallel for num_threads(nt) schedule(static)
    for (int64_t v = 0; v < m; ++v)
      for (int64_t u = 0; u < m; ++u) {
        double sr = 0.0, si = 0.0;
        for (int64_t j = 0; j < n; ++j)
          ort::dft_mac(w[2 * (v * n + j)], w[2 * (v * n + j) + 1], t[2 * (j * m + u)],
                       t[2 * (j * m + u) + 1], sr, si);
        o[v * m + u] = sr * sr + si * si;
      }
  }
  return ORT_OK;
}

// SampledMTF's overlap sum (mtf/sampled.py:162-205) on host memory: the kernel's term
// (ort_sampled_otf.h) and its order of additions (ort_k_sampled_otf.hip with ort_reduce.h's
// block sum): a chunk's 256 lane values -- 0.0 past the pupil's end -- are added 64 at a time
// as the wave's DPP tree adds them (lane i with lane i ^ 1, then pairs, quads, ... : floating-
// point addition commutes, so the tree's value does not depend on which lane holds it), the
// four wave sums in index order onto 0.0, the chunk sums in chunk order onto 0.0.
int ort_host_sampled_otf(const double* x, const double* y, int64_t n_pupil,
                         const double* intensity, const double* opd_waves, int64_t n_batch,
                         const ort_zernike_term* terms, const double* radial,
                         const double* coeffs, int64_t n_terms, const double* shift_x,
                         const double* shift_y, int64_t n_freq, double* otf) {
  const int rc = sampled_otf_check(x, y, n_pupil, intensity, opd_waves, n_batch, terms, radial,
                                   coeffs, n_terms, shift_x, shift_y, n_freq, otf);
  if (rc != ORT_OK) return rc;
  const int64_t pairs = n_batch * n_freq;
  if (pairs == 0) return ORT_OK;
  constexpr int64_t kC = ORT_SAMPLED_OTF_CHUNK;
  const int nt =
      pairs < 2 ? 1 : threads_for(pairs * std::max<int64_t>(n_pupil, 1) * (n_terms + 1));
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int64_t p = 0; p < pairs; ++p) {
    const int64_t b = p / n_freq, f = p - b * n_freq;
    const double sx = shift_x[f], sy = shift_y[f];
    double re = 0.0, im = 0.0;
    int64_t j0 = 0;
    do {  // (an empty pupil: one empty chunk, as the kernel's grid)
      double lane[2][kC];
      for (int64_t k = 0; k < kC; ++k) {
        const int64_t j = j0 + k;
        lane[0][k] = lane[1][k] = 0.0;
        if (j < n_pupil)
          ort::sampled_otf_term(x[j], y[j], intensity[b * n_pupil + j],
                                opd_waves[b * n_pupil + j], sx, sy, terms, radial,
                                coeffs + b * n_terms, (int)n_terms, lane[0][k], lane[1][k]);
      }
      for (int q = 0; q < 2; ++q) {
        double* v = lane[q];
        for (int64_t w = 0; w < kC; w += 64)
          for (int64_t stride = 1; stride < 64; stride *= 2)
            for (int64_t k = w; k < w + 64; k += 2 * stride) v[k] = v[k] + v[k + stride];
        double s = 0.0;
        for (int64_t w = 0; w < kC; w += 64) s += v[w];
        (q == 0 ? re : im) += s;
      }
      j0 += kC;
    } while (j0 < n_pupil);
    otf[2 * p] = re;
    otf[2 * p + 1] = im;
  }
  return ORT_OK;
}

// IncoherentIrradiance's binning (analysis/irradiance.py:243-330) on host memory: the kernels'
// per-ray pieces (ort_irradiance.h) and their fixed-point sums. Integer adds commute, so the
// threads may take the rays in any split.
int ort_host_irradiance_bin(const double* x, const double* y, const double* power, int64_t n,
                            const double* x_edges, int64_t nx, const double* y_edges,
                            int64_t ny, int32_t mode, double pixel_area, double* out) {
  if (mode != ORT_BIN_HISTOGRAM && mode != ORT_BIN_BILINEAR) return ORT_ERR_ARG;
  const int64_t lo = mode == ORT_BIN_BILINEAR ? 2 : 1;
  if (n < 0 || nx < lo || ny < lo || nx > ORT_IRRADIANCE_MAX_PIXELS ||
      ny > ORT_IRRADIANCE_MAX_PIXELS || nx * ny > ORT_IRRADIANCE_MAX_PIXELS)
    return ORT_ERR_ARG;
  if (!x_edges || !y_edges || !out || (n > 0 && (!x || !y || !power))) return ORT_ERR_ARG;
  const ort::IrrGrid g{x_edges, y_edges, nx, ny, mode};
  const int64_t npix = nx * ny;
  const int nt = threads_for(n);
  uint64_t cmax = 0;
#pragma omp parallel for num_threads(nt) schedule(static) reduction(max : cmax)
  for (int64_t i = 0; i < n; ++i) {
    int64_t pix[4];
    double c[4];
    const int k = ort::irr_contributions(g, x[i], y[i], power[i], pix, c);
    for (int j = 0; j < k; ++j)
      if (ort::irr_finite(c[j])) cmax = std::max(cmax, ort::irr_abs_bits(c[j]));
  }
  const int E = ort::irr_exponent(cmax, ort::irr_log2_ceil(n));
  std::vector<uint64_t> acc((size_t)npix, 0);
  std::vector<uint32_t> flags((size_t)npix, 0);
  uint64_t* const sums = acc.data();
  uint32_t* const marks = flags.data();
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int64_t i = 0; i < n; ++i) {
    int64_t pix[4];
    double c[4];
    const int k = ort::irr_contributions(g, x[i], y[i], power[i], pix, c);
    for (int j = 0; j < k; ++j) {
      if (ort::irr_finite(c[j])) {
        const uint64_t q = (uint64_t)ort::irr_quantise(c[j], E);
#pragma omp atomic
        sums[pix[j]] += q;
      } else {
#pragma omp atomic write
        marks[pix[j]] = 1u;
      }
    }
  }
  const double area = ort::irr_area(g, pixel_area);
  for (int64_t j = 0; j < npix; ++j)
    out[j] = ort::irr_finish((int64_t)acc[(size_t)j], flags[(size_t)j], E, area);
  return ORT_OK;
}

int ort_host_irradiance_bin_vjp(const double* x, const double* y, const double* power,
                                int64_t n, const double* x_edges, int64_t nx,
                                const double* y_edges, int64_t ny, double pixel_area,
                                const double* grad_out, double* grad_x, double* grad_y,
                                double* grad_power) {
  if (n < 0 || nx < 2 || ny < 2 || nx > ORT_IRRADIANCE_MAX_PIXELS ||
      ny > ORT_IRRADIANCE_MAX_PIXELS || nx * ny > ORT_IRRADIANCE_MAX_PIXELS)
    return ORT_ERR_ARG;
  if (!x_edges || !y_edges || !grad_out) return ORT_ERR_ARG;
  if (n == 0) return ORT_OK;
  if (!x || !y || !power || !grad_x || !grad_y || !grad_power) return ORT_ERR_ARG;
  const ort::IrrGrid g{x_edges, y_edges, nx, ny, ORT_BIN_BILINEAR};
  const double area = ort::irr_area(g, pixel_area);
  const int nt = threads_for(n);
#pragma omp parallel for num_threads(nt) schedule(static)
  for (int64_t i = 0; i < n; ++i)
    ort::irr_vjp(g, grad_out, x[i], y[i], power[i], area, grad_x[i], grad_y[i], grad_power[i]);
  return ORT_OK;
}

}  // extern "C"
