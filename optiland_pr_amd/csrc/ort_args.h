// ort_args.h -- the argument layer and the front end shared by the device library
// (ort_api.hip and the ort_k_*.hip kernels) and the host library (ort_host.cpp).
//
// Everything here is plain C++ without HIP calls (ORT_HD: __host__ __device__ under hipcc,
// plain functions under g++), in four parts:
//
//   arguments    the kernel argument blocks KArgs / AArgs / JArgs, the F_* specialisation
//                bits, and their unpacking from the C ABI structs with the argument checks
//                (fill_args, fill_pol);
//   per-ray      table lookups (tab, optics_row, optics_ray), frame changes (localize,
//                globalize), the surface step after the distance of the interaction-model
//                and coated paths (interact, pol_step), the geometry predicates, the ray
//                load / store and the record store (Plain / a kernel's store policy);
//   slots        the adjoint's tape rows and parameter slots (tape_rows, mono_*,
//                slot_weight, vjp_slot_count);
//   VJP front    vjp_check_call, vjp_inputs_ok, vjp_prepare, vjp_fill_adjoint and
//                vjp_fill_unrolled: the checks and assignments of ort_trace_*_vjp and
//                ort_host_trace_*_vjp that do not depend on where memory lives. What a
//                library does differently (workspace and launches on the device, chunk
//                loops on the host, and the refusals only one of them makes) stays in that
//                library as a named check.
//
// The derivative sweeps themselves (adj_ray, vjp_ray) are in ort_sweep.h.
// Reference files are cited as path:line under optiland/.
#pragma once

#include "ort_core.h"
#include "ort_interact.h"
#include "ort_material.h"
#include "ort_polar.h"
#include "ort_scatter.h"

namespace ortk {

// Lens tables are read-only for the whole launch and indexed by wave-uniform values, so
// the kernels read them through the constant address space: the compiler then emits
// scalar loads (s_load -> SGPRs) instead of per-lane vector loads. Identity on the host.
#if defined(__HIP_DEVICE_COMPILE__)
#define ORT_CONST_AS __attribute__((address_space(4)))
#else
#define ORT_CONST_AS
#endif
template <class T>
using cptr = const ORT_CONST_AS T*;
template <class T>
ORT_INLINE cptr<T> cst(const T* p) {
  return (cptr<T>)(p);
}
using PD = cptr<double>;
using PZ = cptr<ort_zernike_term>;
constexpr ort::ZSeed kNoSeed{nullptr, 0};

// Kernel specialisation bits: bits 0-3 = Newton kinds present (ort::KM_*), bit 4 = rays
// generated in-kernel from pupil coordinates.
enum : uint32_t {
  F_KM = 15u | ort::KM_NURBS,  // the kinds (bits 0-3 and KM_NURBS = bit 16)
  F_GEN = 1u << 4,
  F_REC = 1u << 5,   // some surfaces are recorded (standard_surface.py:266-286)
  F_MONO = 1u << 6,  // the wavelength row is wave-uniform (one wavelength in the lens
                     // tables, or segments aligned to 64 rays): scalar table loads
  F_WRAY = 1u << 7,  // per-ray wavelengths: n, k from lens.materials (ort_batch.w)
  F_IA = 1u << 8,    // thin-lens / phase / grating interactions (ort_interaction)
  F_AXIAL = 1u << 9, // ORT_LENS_AXIAL: every frame a +z translation (closed-form kernels)
  F_TAPE = 1u << 10, // write the adjoint tape as the trace runs (ort_options.tape)
  F_SPOT = 1u << 11, // closed-form kernel: spot pass 1 in the epilogue (ort_trace_spot)
  F_RMS = 1u << 12,  // taped Newton kernel: the rms spot size's workgroup rows in the
                     // epilogue (ort_options.rms_part)
  F_STRIDE = 1u << 13,  // Newton kernel of a verify-and-re-trace round: a grid of at most
                        // kVerifyGrid workgroups strides over the blocks of rays
  F_POL = 1u << 14,  // coatings / the polarization matrix per ray (ort_polar.h,
                     // ort_trace_*_polarized)
  F_PLAIN = 1u << 15,  // ORT_LENS_PLAIN: planes and conics only, no aperture, mirror or
                       // recorded surface (closed-form kernels: the fast pass's plain form)
  F_SCAT = 1u << 17,  // BSDF scattering after the interaction (ort_scatter.h,
                      // ort_trace_*_scatter); bit 16 is ort::KM_NURBS
  F_SPHERES = 1u << 18,  // ORT_LENS_SPHERES beside F_PLAIN: every standard surface a seeded
                         // sphere of finite radius (closed-form kernels: the plain form with
                         // those uniform decisions compiled in; select_closed drops the bit
                         // wherever it drops F_PLAIN)
};
// every Newton kind compiled in: the host library's one specialisation (the GPU's per-lens
// KM specialisations only prune code: the values are the same)
constexpr uint32_t kAllKinds =
    ort::KM_EVEN | ort::KM_ODD | ort::KM_ZERN | ort::KM_FREE | ort::KM_NURBS;

// Adjoint tape (adj_ray): per surface, rows of n_rays doubles -- the incoming global
// x y z L M N, the distance t (7 rows), and for a Newton surface kHist more: the iterates
// before the last kHist updates, row 7 + m = t_{U-1-m} for m < min(U, kHist), the initial
// guess t_0 in the rows m >= U (ABI v19: closed-form surfaces take no iterate rows, and
// every row of the tape is written -- it is the trace op's output, ops.py)
constexpr int kTapeRows = 11;  // the most rows of one surface
constexpr int kHist = 4;

// tape rows of surface s, and the first row of surface si (the surfaces before it)
ORT_INLINE int tape_rows(const ort_surface& s) {
  return (s.geometry == ORT_GEOM_PLANE || s.geometry == ORT_GEOM_STANDARD) ? 7 : kTapeRows;
}
ORT_INLINE int64_t tape_row0(const ort_surface* surf, int si) {
  int64_t r = 0;
  for (int k = 0; k < si; ++k) r += tape_rows(cst(surf)[k]);
  return r;
}

struct KArgs {
  // lens
  const ort_surface* surf;
  const ort_cs_op* cs;
  const double* coef;
  const ort_zernike_term* zern;
  const double* n_tab;
  const double* alpha_tab;
  const ort_surface_optics* optics;
  int32_t n_surf;
  int32_t n_lambda;
  int32_t n_mat;
  int32_t final_mat;
  double final_thickness;
  // rays
  ort_rays in;
  ort_rays out;
  const double* px;
  const double* py;
  // batch
  int64_t n_rays;
  int64_t seg_len;
  int64_t group_len;
  const ort_segment* seg;
  int32_t n_seg;
  int32_t pupil_per_ray;
  // options
  int32_t newton_mode;
  int32_t start_surface;
  const int32_t* sched;
  int32_t conv_base;  // first stop index of the ort_newton_stat.conv_mask window
  // outputs
  double* rec;
  ort_newton_stat* stats;
  int32_t* status;
  // per-ray wavelengths (F_WRAY)
  const double* w;
  const ort_material* mats;
  // wavelength of each table row (F_IA: phase / grating interactions)
  const double* lambdas;
  // pupil apodization of generated rays (NULL: intensity 1)
  const ort_apodization* apod;
  // trace_kernel: blocks walk the pupil chunk by chunk over all (field, lambda) segments
  // (pair_major_ray); set by the host only when it is a bijection (see launch)
  int32_t block_remap;
  // nullable: the launch is a no-op unless *run_if == 1 (ort_options.run_if)
  const int32_t* run_if;
  int32_t no_init;  // host side only: ORT_OPT_NO_INIT (skip init_outputs)
  int32_t exact_only;  // ORT_OPT_EXACT: every ray on the exact sequences (trace_kernel skips
                       // its deferred-check pass, trace_closed_kernel re-traces every lane)
  // verify-and-re-trace (ort_options.verify_*): the launch decides from vstats first
  const ort_newton_stat* vstats;
  const int32_t* vprev;
  int32_t* vflag;
  int32_t* sched_out;
  double* tape;     // F_TAPE: [sum of tape_rows][n_rays] (ort_options.tape)
  // F_SPOT (ort_trace_spot): block b traces chunk b % spot_chunks of pair b / spot_chunks
  // (kClosedBlock rays of seg_len, the tail lanes idle) and writes the chunk's count, sum x,
  // sum y of its i > 0 image points, in the image frame, to spot_part1[b][3] -- the rows
  // spot_sum_kernel would write (ort_k_spot.hip), by the same block reduction
  double* spot_part1;
  const ort_cs_op* spot_ops;
  int32_t spot_n_ops;
  int32_t spot_chunks;
  double* rms_part;  // F_RMS: [workgroup][4] (ort_options.rms_part)
  // F_POL (ort_polarization): the surfaces' coatings, the intensity mode with the input
  // field (ex, ey) and the optional [18][n_rays] planes of P
  const ort_coating* coat;
  int32_t pol_mode;
  ort::Cplx pol_ex, pol_ey;
  double* p_out;
  // F_SCAT (ort_scatter): the surfaces' BSDFs and the random stream's seed, ray offset and
  // attempt cap
  const ort_bsdf* bsdf;
  uint64_t scat_seed;
  int64_t scat_offset;
  int32_t scat_max;
};

// ort_trace_*_polarized: the checks beyond fill_args and the F_POL arguments. Lenses with
// thin-lens / phase / grating surfaces (and NURBS lenses, which ride on F_IA), per-ray
// wavelengths, a tape or an rms request are refused.
inline int fill_pol(KArgs& a, const ort_batch* batch, const ort_options* opt,
                    const ort_polarization* pol, uint32_t& feat) {
  if (!pol || !pol->coatings || batch->w || opt->tape || opt->rms_part) return ORT_ERR_ARG;
  if (pol->mode < ORT_POL_IGNORE || pol->mode > ORT_POL_UNPOLARIZED) return ORT_ERR_ARG;
  if (feat & (F_IA | F_WRAY | ort::KM_NURBS)) return ORT_ERR_ARG;
  a.coat = pol->coatings;
  a.pol_mode = pol->mode;
  a.pol_ex = {pol->ex_re, pol->ex_im};
  a.pol_ey = {pol->ey_re, pol->ey_im};
  a.p_out = pol->p_out;
  feat |= F_POL;
  return ORT_OK;
}

// ort_trace_*_scatter: the checks beyond fill_args and the F_SCAT arguments, with the same
// refusals as fill_pol (the scatter step sits in the refractive / reflective surface step).
inline int fill_scat(KArgs& a, const ort_batch* batch, const ort_options* opt,
                     const ort_scatter* scat, uint32_t& feat) {
  if (!scat || !scat->bsdf || batch->w || opt->tape || opt->rms_part) return ORT_ERR_ARG;
  if (scat->max_attempts < 1 || scat->ray_offset < 0) return ORT_ERR_ARG;
  if (feat & (F_IA | F_WRAY | ort::KM_NURBS)) return ORT_ERR_ARG;
  a.bsdf = scat->bsdf;
  a.scat_seed = scat->seed;
  a.scat_offset = scat->ray_offset;
  a.scat_max = scat->max_attempts;
  feat = (feat | F_SCAT) & ~(F_PLAIN | F_SPHERES);  // never the closed-form kernels' fast pass
  return ORT_OK;
}

// KArgs from the C ABI structs (argument checks included) and the kernel feature bits the
// lens and batch call for (F_KM kinds, F_REC, F_WRAY / F_MONO, F_IA, F_AXIAL, F_PLAIN).
inline int fill_args(KArgs& a, const ort_lens* lens, const ort_batch* batch,
                     const ort_options* opt, double* rec, ort_newton_stat* stats,
                     int32_t* status, uint32_t& feat) {
  if (!lens || !batch || !opt) return ORT_ERR_ARG;
  if (lens->n_surfaces < 0 || lens->n_surfaces > ORT_MAX_SURFACES) return ORT_ERR_SURFACES;
  if (lens->n_surfaces > 0 &&
      (!lens->surfaces || !lens->n_tab || !lens->alpha_tab || !lens->optics))
    return ORT_ERR_ARG;
  if (batch->n_rays < 0 || batch->seg_len < 1 || batch->group_len < 1) return ORT_ERR_ARG;
  if (lens->n_lambda < 1 || lens->n_mat < 1) return ORT_ERR_ARG;
  if (opt->start_surface < 0) return ORT_ERR_ARG;
  a.surf = lens->surfaces;
  a.cs = lens->cs_ops;
  a.coef = lens->coef;
  a.zern = lens->zern;
  a.n_tab = lens->n_tab;
  a.alpha_tab = lens->alpha_tab;
  a.optics = lens->optics;
  a.n_surf = lens->n_surfaces;
  a.n_lambda = lens->n_lambda;
  a.n_mat = lens->n_mat;
  a.final_mat = lens->final_mat;
  a.final_thickness = lens->final_thickness;
  a.n_rays = batch->n_rays;
  a.seg_len = batch->seg_len;
  a.group_len = batch->group_len;
  a.seg = batch->seg;
  a.n_seg = batch->n_seg;
  a.pupil_per_ray = batch->pupil_per_ray;
  a.apod = batch->apod;
  a.newton_mode = opt->newton_mode;
  a.start_surface = opt->start_surface;
  a.sched = opt->sched;
  a.conv_base = opt->conv_base;
  a.run_if = opt->run_if;
  a.no_init = (opt->flags & ORT_OPT_NO_INIT) != 0;
  a.exact_only = (opt->flags & ORT_OPT_EXACT) != 0;
  a.tape = opt->tape;
  a.rms_part = opt->rms_part;
  if (opt->conv_base < 0) return ORT_ERR_ARG;
  // geometry ids this library knows (enum ort_geometry): anything else is refused here
  // rather than traced as some other kind
  if (lens->geometry_mask & ~((2u << ORT_GEOM_NURBS) - 1u)) return ORT_ERR_ARG;
  a.rec = rec;
  a.stats = stats;
  a.status = status;
  feat = 0;
  if (lens->geometry_mask & (1u << ORT_GEOM_EVEN_ASPHERE)) feat |= ort::KM_EVEN;
  if (lens->geometry_mask & (1u << ORT_GEOM_ODD_ASPHERE)) feat |= ort::KM_ODD;
  if (lens->geometry_mask & (1u << ORT_GEOM_ZERNIKE)) feat |= ort::KM_ZERN;
  if (lens->geometry_mask & ((1u << ORT_GEOM_POLYNOMIAL) | (1u << ORT_GEOM_CHEBYSHEV) |
                             (1u << ORT_GEOM_BICONIC) | (1u << ORT_GEOM_TOROIDAL) |
                             (1u << ORT_GEOM_FORBES_QBFS) | (1u << ORT_GEOM_FORBES_Q2D) |
                             (1u << ORT_GEOM_GRID_SAG)))
    feat |= ort::KM_FREE;
  // NURBS lenses take the all-kinds kernels of ort_k_trace_ia.hip (the only trace kernels
  // with the NURBS solves compiled in)
  if (lens->geometry_mask & (1u << ORT_GEOM_NURBS))
    feat |= ort::KM_NURBS | F_IA | ort::KM_EVEN | ort::KM_ODD | ort::KM_ZERN | ort::KM_FREE;
  if (rec) feat |= F_REC;
  if (batch->w) {  // per-ray wavelengths: n, k from the material tables
    if (!lens->materials) return ORT_ERR_ARG;
    a.w = batch->w;
    a.mats = lens->materials;
    feat |= F_WRAY;
  } else if (lens->n_lambda == 1 || batch->n_seg <= 1 || batch->seg_len % 64 == 0) {
    // every wave reads one wavelength row: one row, one segment, or segment boundaries
    // on the 64-ray wave boundaries (ray r is in segment r / seg_len)
    feat |= F_MONO;
  }
  if (lens->interaction_mask & ~(1u << ORT_IA_REFRACT_REFLECT)) {
    feat |= F_IA;
    a.lambdas = lens->wavelengths;
    const uint32_t need_w = (1u << ORT_IA_PHASE) | (1u << ORT_IA_DIFFRACTIVE);
    if ((lens->interaction_mask & need_w) && !batch->w && !lens->wavelengths) return ORT_ERR_ARG;
  }
  if (lens->frame_flags & ORT_LENS_AXIAL) feat |= F_AXIAL;
  // the closed-form kernels' bit alone: a lens with a Newton or interaction surface is not
  // plain whatever its flags say, and the other kernel families are selected without it
  if ((lens->frame_flags & ORT_LENS_PLAIN) && (feat & (F_KM | F_IA)) == 0) feat |= F_PLAIN;
  // form_flags was a reserved word: honoured only when it holds the one known bit and
  // nothing else, so a caller that never cleared it gets the plain form, not this one
  if ((feat & F_PLAIN) != 0 && lens->form_flags == ORT_LENS_SPHERES) feat |= F_SPHERES;
  if (opt->newton_mode != ORT_NEWTON_SCHEDULE && opt->newton_mode != ORT_NEWTON_WAVE)
    return ORT_ERR_ARG;
  a.vstats = opt->verify_stats;
  a.vprev = opt->verify_prev_flag;
  a.vflag = opt->verify_flag;
  a.sched_out = opt->sched_out;
  if (opt->verify_stats) {  // verify-and-re-trace (see ort_options)
    const int64_t ng = (batch->n_rays + batch->group_len - 1) / batch->group_len;
    if ((feat & F_KM) == 0 || opt->newton_mode != ORT_NEWTON_SCHEDULE || !opt->sched ||
        !opt->verify_flag || !opt->sched_out || opt->sched_out == opt->sched ||
        !(opt->flags & ORT_OPT_NO_INIT) ||
        opt->run_if || ng * (int64_t)lens->n_surfaces > ORT_VERIFY_MAX_SCHED)
      return ORT_ERR_ARG;
  }
  return ORT_OK;
}

// ort_dft_psf / ort_host_dft_psf: the checks both libraries make (the device adds its
// workspace and grid limits).
inline int dft_check(const double* amp, const double* opd, int64_t batch, int64_t n, int64_t m,
                     double pad, const double* out) {
  if (batch < 0 || n < 1 || m < 0 || n > ORT_DFT_MAX_SIZE || m > ORT_DFT_MAX_SIZE)
    return ORT_ERR_ARG;
  if (!(pad > 0.0) || !(pad <= 1.79769313486231570815e308)) return ORT_ERR_ARG;
  if (batch > 0 && (!amp || !opd)) return ORT_ERR_ARG;
  if (batch > 0 && m > 0 && !out) return ORT_ERR_ARG;
  if (batch > INT64_MAX / 16 / ORT_DFT_MAX_SIZE / ORT_DFT_MAX_SIZE) return ORT_ERR_ARG;
  return ORT_OK;
}

// ort_sampled_otf / ort_host_sampled_otf: the checks both libraries make (the device adds
// its workspace and grid limits). An empty pupil, term list, batch or frequency list is valid.
inline int sampled_otf_check(const double* x, const double* y, int64_t n_pupil,
                             const double* intensity, const double* opd, int64_t n_batch,
                             const ort_zernike_term* terms, const double* radial,
                             const double* coeffs, int64_t n_terms, const double* shift_x,
                             const double* shift_y, int64_t n_freq, const double* otf) {
  if (n_pupil < 0 || n_batch < 0 || n_terms < 0 || n_freq < 0) return ORT_ERR_ARG;
  if (n_terms > 0x7fffffff || n_freq > 0x7fffffff) return ORT_ERR_ARG;
  if (n_pupil > 0 && (!x || !y)) return ORT_ERR_ARG;
  if (n_pupil > 0 && n_batch > 0 && (!intensity || !opd)) return ORT_ERR_ARG;
  if (n_terms > 0 && (!terms || !radial)) return ORT_ERR_ARG;
  if (n_terms > 0 && n_batch > 0 && !coeffs) return ORT_ERR_ARG;
  if (n_freq > 0 && (!shift_x || !shift_y)) return ORT_ERR_ARG;
  if (n_freq > 0 && n_batch > 0 && !otf) return ORT_ERR_ARG;
  if (n_pupil > 0 && n_batch > INT64_MAX / 8 / n_pupil) return ORT_ERR_ARG;
  return ORT_OK;
}

// Table lookup n_tab[lam][mat]: a uniform scalar load when the lens is traced at one
// wavelength (the common case), else a per-lane load of the small L1-resident table.
ORT_INLINE double tab(const double* t, int n_lambda, int n_mat, int lam, int mat) {
  if (n_lambda == 1) return cst(t)[mat];
  return t[lam * n_mat + mat];
}

// optical constants of surface si at wavelength row lam
ORT_INLINE ort_surface_optics optics_row(const KArgs& a, int lam, int si) {
  if (a.n_lambda == 1) return cst(a.optics)[si];
  return a.optics[lam * a.n_surf + si];
}

// F_WRAY: the surface's optical constants at this ray's own wavelength w, evaluated from
// the material tables as the reference evaluates material.n(rays.w) / .k(rays.w)
// (standard_surface.py:218, refractive_reflective_model.py:32-55, homogeneous.py:45-54)
ORT_INLINE ort_surface_optics optics_ray(const KArgs& a, const ort_surface& s, double w) {
  const ort_material mp = cst(a.mats)[s.mat_pre];
  const ort_material mq = cst(a.mats)[s.mat_post];
  ort_surface_optics o;
  o.n_pre = ort::material_n(mp, a.coef, w);
  o.n_post = ort::material_n(mq, a.coef, w);
  o.u = o.n_pre / o.n_post;
  o.u_sq = o.u * o.u;
  o.alpha_pre = ort::absorption_alpha(ort::material_k(mp, a.coef, w), w);
  return o;
}

// localize / globalize (coordinate_system.py:73-107): the root frame's translation
// (cs_t) inline and unconditional, the rest (rotations, reference_cs chains) through the
// op lists, which are empty for plain decentred surfaces (no branch, no register
// shuffling around one)
template <class T>
ORT_INLINE void localize(const KArgs& a, const ort_surface& s, ort::RayT<T>& r) {
  {
    r.x = r.x + -s.cs_t[0];
    r.y = r.y + -s.cs_t[1];
  }
  r.z = r.z + -s.cs_t[2];
  for (int c = 0; c < s.n_cs_loc; ++c) ort::apply_cs_op(r, cst(a.cs)[s.cs_loc_off + c]);
}

template <class T>
ORT_INLINE void globalize(const KArgs& a, const ort_surface& s, ort::RayT<T>& r) {
  for (int c = 0; c < s.n_cs_glob; ++c) ort::apply_cs_op(r, cst(a.cs)[s.cs_glob_off + c]);
  r.x = r.x + s.cs_t[0];
  r.y = r.y + s.cs_t[1];
  r.z = r.z + s.cs_t[2];
}

// geometry ids this library implements (enum ort_geometry); the traces turn any other
// id into NaN rays plus ORT_STATUS_BAD_GEOMETRY
ORT_INLINE bool known_geometry(int g) { return g >= ORT_GEOM_PLANE && g <= ORT_GEOM_NURBS; }
// surfaces of the Newton schedule / statistics machinery (not plane, conic or NURBS); on
// the host, the surfaces trace_group steps in lockstep under the reference's stop rule
ORT_INLINE bool scheduled_geometry(int g) {
  return g != ORT_GEOM_PLANE && g != ORT_GEOM_STANDARD && g != ORT_GEOM_NURBS;
}

// status bit of a normalisation-range error at surface s (zernike.py:234-246,
// chebyshev.py:203-215: both raise ValueError in the reference)
ORT_INLINE int range_bit(const ort_surface& s) {
  return s.geometry == ORT_GEOM_CHEBYSHEV ? (int)ORT_STATUS_CHEBYSHEV_RANGE
                                          : (int)ORT_STATUS_ZERNIKE_RANGE;
}

// F_IA: the surface's interaction model after propagation / OPD / clipping
// (standard_surface.py:225 -> interactions/*.py). unnorm tracks the reference's
// rays.is_normalized flag, which only a thin lens clears (homogeneous.py:55-57).
// KM: the Newton kinds compiled in (trace_kernel<F_IA>: the lens's, the host: kAllKinds);
// WRAY: the wavelength of a phase / grating surface is the ray's own wl, else row lam's.
template <uint32_t KM, bool WRAY>
ORT_INLINE void interact(const KArgs& a, const ort_surface& s, ort::Ray& r,
                         const ort_surface_optics& o, int lam, double wl, bool& unnorm) {
  const bool refl = (s.flags & ORT_SURF_REFLECTIVE) != 0;
  const PD p = cst(a.coef) + s.ia_off;
  if (s.interaction == ORT_IA_THIN_LENS) {
    ort::thin_lens(r, p[0], o.n_pre, refl ? -o.n_pre : o.n_post);
    unnorm = true;
    return;
  }
  double nx, ny, nz;
  ort::surface_normal<KM>(s, s.radius, s.conic, cst(a.coef), cst(a.zern), kNoSeed, r, nx, ny,
                          nz);
  if (s.interaction == ORT_IA_REFRACT_REFLECT) {
    if (refl)
      ort::reflect(r, nx, ny, nz);
    else
      ort::refract(r, nx, ny, nz, o.u);
    return;
  }
  double w = wl;
  if constexpr (!WRAY) w = a.n_lambda == 1 ? cst(a.lambdas)[0] : a.lambdas[lam];
  if (s.interaction == ORT_IA_PHASE)
    ort::phase_interact(r, p, nx, ny, nz, o.n_pre, refl ? o.n_pre : o.n_post, refl, w);
  else
    ort::diffract(r, p, nx, ny, nz, o.n_pre, o.n_post, refl, w);
}

// F_POL: the step of a coated refractive / reflective surface si at the hit point --
// interact()'s operations on the ray, with the normal and the direction before the
// interaction kept for the polarization update (the coating's own materials n1, n2 at
// wavelength row lam). hn: the caller's (nx, ny, nz) is the normal there (the last Newton
// evaluation's); otherwise it is evaluated into them here. (The normal is the caller's
// variable, not a by-value copy: with copies trace_kernel<F_POL> compiles to the same
// instructions in another order.)
template <uint32_t KM>
ORT_INLINE void pol_step(const KArgs& a, const ort_surface& s, const ort_surface_optics& o,
                         int si, int lam, ort::Ray& r, ort::PolState& pol, bool hn,
                         double& nx, double& ny, double& nz) {
  if (!hn)
    ort::surface_normal<KM>(s, s.radius, s.conic, cst(a.coef), cst(a.zern), kNoSeed, r, nx, ny,
                            nz);
  const double k0x = r.L, k0y = r.M, k0z = r.N;
  const bool refl = (s.flags & ORT_SURF_REFLECTIVE) != 0;
  if (refl)
    ort::reflect(r, nx, ny, nz);
  else
    ort::refract(r, nx, ny, nz, o.u);
  const ort_coating ct = cst(a.coat)[si];
  double n1 = 1.0, n2 = 1.0;  // the coating's own materials at this wavelength
  if (ct.kind == ORT_COAT_FRESNEL) {
    n1 = tab(a.n_tab, a.n_lambda, a.n_mat, lam, ct.mat_pre);
    n2 = tab(a.n_tab, a.n_lambda, a.n_mat, lam, ct.mat_post);
  }
  ort::pol_surface(pol, ct, refl, nx, ny, nz, k0x, k0y, k0z, r.L, r.M, r.N, n1, n2, r.i);
}

// F_SCAT: the step of a refractive / reflective surface si at the hit point -- interact()'s
// operations on the ray with the raw normal kept, then the BSDF of the surface (kind NONE:
// nothing more, so the ray is the plain trace's). rid: the ray's index in the batch.
// Returns the status bits to raise. hn, nx, ny, nz: as pol_step.
template <uint32_t KM>
ORT_INLINE int scat_step(const KArgs& a, const ort_surface& s, const ort_surface_optics& o,
                         int si, int64_t rid, ort::Ray& r, bool hn, double& nx, double& ny,
                         double& nz) {
  if (!hn)
    ort::surface_normal<KM>(s, s.radius, s.conic, cst(a.coef), cst(a.zern), kNoSeed, r, nx, ny,
                            nz);
  if (s.flags & ORT_SURF_REFLECTIVE)
    ort::reflect(r, nx, ny, nz);
  else
    ort::refract(r, nx, ny, nz, o.u);
  const ort_bsdf f = cst(a.bsdf)[si];
  if (f.kind == ORT_BSDF_NONE) return 0;
  const bool ok = ort::bsdf_scatter(f, a.scat_seed, (uint64_t)(rid + a.scat_offset),
                                    (uint32_t)si, a.scat_max, nx, ny, nz, r.L, r.M, r.N);
  return ok ? 0 : (int)ORT_STATUS_SCATTER_ATTEMPTS;
}

// The caller's ray r_ld (traces of resident rays).
ORT_INLINE void load_ray(const KArgs& a, int64_t r_ld, ort::Ray& r) {
  r.x = a.in.x[r_ld];
  r.y = a.in.y[r_ld];
  r.z = a.in.z[r_ld];
  r.L = a.in.L[r_ld];
  r.M = a.in.M[r_ld];
  r.N = a.in.N[r_ld];
  r.i = a.in.i[r_ld];
  r.opd = a.in.opd[r_ld];
  r.att = 0.0;
}

// How a trace writes an output value that a later launch / the caller reads: a plain store
// here; the kernels pass their non-temporal policy (ort_kernels.h StreamStore). Every call
// names its policy: no default, so a kernel cannot lose its streaming store by omission.
struct PlainStore {
  static ORT_INLINE void put(double& lhs, double v) { lhs = v; }
};

// Ray rid of the outputs. The ray is stored field by field with the intensity (whose exp is
// a branch) evaluated in place, between the N and the opd store.
// inten: the intensity to store instead of the ray's own (an apodized / polarized one)
template <class St>
ORT_INLINE void store_ray(const KArgs& a, int64_t rid, const ort::Ray& r,
                          const double* inten = nullptr) {
  St::put(a.out.x[rid], r.x);
  St::put(a.out.y[rid], r.y);
  St::put(a.out.z[rid], r.z);
  St::put(a.out.L[rid], r.L);
  St::put(a.out.M[rid], r.M);
  St::put(a.out.N[rid], r.N);
  St::put(a.out.i[rid], inten ? *inten : ort::intensity(r));
  St::put(a.out.opd[rid], r.opd);
}

// F_REC: ray rid's row of a recording surface (after globalize). apod: the pupil factor
// the closed kernel multiplies into a recorded intensity (closed_surfaces)
template <class St>
ORT_INLINE void store_record(const KArgs& a, const ort_surface& s, int64_t rid,
                             const ort::Ray& r, const double* apod = nullptr) {
  double* base = a.rec + (int64_t)s.rec_slot * 8 * a.n_rays + rid;
  St::put(base[0 * a.n_rays], r.x);
  St::put(base[1 * a.n_rays], r.y);
  St::put(base[2 * a.n_rays], r.z);
  St::put(base[3 * a.n_rays], r.L);
  St::put(base[4 * a.n_rays], r.M);
  St::put(base[5 * a.n_rays], r.N);
  St::put(base[6 * a.n_rays], apod ? *apod * ort::intensity(r) : ort::intensity(r));
  St::put(base[7 * a.n_rays], r.opd);
}

// =====================================================================================
// The derivative sweeps' argument blocks (the sweeps: ort_sweep.h)
// =====================================================================================
// Reverse mode (adj_ray, ORT_VJP_ADJOINT)
struct AArgs {
  const int32_t* zparam;    // [n_zern] parameter per Zernike term (< 0: constant)
  const double* tan_surf;   // [n_param][n_surf][3]: d radius, d conic, d vertex z
  const double* tan_final;  // [n_param]: d final_thickness
  int32_t n_param;
  int32_t n_zern;
  int32_t n_slot;           // vjp_slot_count
  int32_t n_surf;
  int64_t n_wave;           // partial columns (GPU: one per block of the main launch)
  ort_rays cot;             // cotangents of the outputs (NULL field: zero)
  // cotangents of the per-surface record buffer [n_rec][8][n_rays] (NULL: zero) and the
  // primal's record buffer (its intensity rows weight the absorption adjoint)
  const double* rec_cot;
  const double* rec;
  ort_rays gin;             // RES: d / d rays_in (NULL field: not wanted)
  double* tape;             // [sum of tape_rows][n_rays]
  double* partial;          // [n_slot][n_wave]
  double* slot_sum;         // [n_slot]
  const int32_t* need;      // [n_slot]: some parameter depends on this slot
  int32_t zero_partials;    // adj_run: memset the partials first (start_surface > 0: the
                            // earlier surfaces' slots are never written)
  int32_t tape_ready;       // the primal trace wrote the tape (F_TAPE): reverse sweep only,
  ort_rays primal;          // the final ray state read from its outputs (L, M, N, i)
  double* grad;             // [n_param], accumulated (grad_store: overwritten)
  int32_t grad_store;
  // Zernike coefficient adjoints in the Cartesian monomial basis (ort_vjp_params.n_mono,
  // ABI v18): every Zernike surface with a Cartesian block (zm_deg >= 0) owns 2 K slots
  // after the final-thickness slot -- S_k = sum w_sag m_k and D_k = sum (a_x dm_k/dxn +
  // a_y dm_k/dyn) over its evaluations, m_k = xn^p yn^q in the block's order -- and the
  // parameter reduce applies the term matrices Ms / Mn once per launch (mono_weight).
  // mono_on: n_mono equals that count (mono_slots); otherwise the per-term slots serve.
  int32_t n_mono;
  int32_t mono_on;
  const ort_surface* surf;  // the lens tables the reduce reads the term matrices from
  const ort_zernike_term* zern;
  const double* coef;
  // an rms spot size's cotangent folded into the x, y cotangents (ort_vjp_params.rms_*)
  const double* rms_stats;
  const double* rms_grad;
};

// Forward mode (vjp_ray, ORT_VJP_UNROLLED)
struct JArgs {
  const int32_t* zparam;   // [n_zern_terms] parameter index per term, < 0: constant
  const double* tan_surf;  // [n_param][n_surf][3]: d radius, d conic, d vertex z
  const double* tan_final; // [n_param]: d final_thickness
  int32_t n_param;
  int32_t p0;              // first parameter of this launch
  ort_rays cot;            // cotangents of the outputs (NULL field: zero)
  const double* rec_cot;   // cotangents of the record buffer [n_rec][8][n_rays] (or NULL)
  double* grad;            // [n_param]
  double* partial;         // device: [n_block][P] block sums of this chunk (fixed-order
                           // reduction by vjp_reduce_kernel; no atomics)
};

// monomials of a Cartesian block of degree N
ORT_INLINE int mono_count(int N) { return (N + 1) * (N + 2) / 2; }
// the highest Cartesian-block degree with a specialised monomial adjoint (zmono_adjoint_deg;
// the host lowers blocks up to geometries.ZM_MAX_DEG = 6). A block of a higher degree --
// only through a hand-made ort_lens: the forward kernels evaluate any degree -- takes the
// per-term slots, so its coefficient adjoint stays exact.
constexpr int kMonoMaxDeg = 6;
// slots of a surface in the monomial basis (0: none)
ORT_INLINE int mono_slots(const ort_surface& s) {
  return (s.geometry == ORT_GEOM_ZERNIKE && s.zm_deg >= 0 && s.zm_deg <= kMonoMaxDeg)
             ? 2 * mono_count(s.zm_deg)
             : 0;
}
// the lens's monomial slot count (every surface, in order)
ORT_INLINE int mono_total(const ort_surface* surf, int n_surf) {
  int t = 0;
  for (int si = 0; si < n_surf; ++si) t += mono_slots(cst(surf)[si]);
  return t;
}

// the monomial slots serve (AArgs.mono_on): the caller's n_mono is the lens's count
ORT_INLINE bool mono_enabled(const AArgs& j) {
  return j.n_mono > 0 && j.zparam && j.surf && j.coef && j.zern &&
         mono_total(j.surf, j.n_surf) == j.n_mono;
}

// the traced surface whose Zernike terms include row `row` of lens.zern (-1: none)
ORT_INLINE int term_surface(const AArgs& j, int row) {
  for (int si = 0; si < j.n_surf; ++si) {
    const ort_surface s = cst(j.surf)[si];
    if (s.geometry == ORT_GEOM_ZERNIKE && row >= s.coef_off && row < s.coef_off + s.n_coef)
      return si;
  }
  return -1;
}

// d(monomial slot m) / d(parameter p): slot m (0-based after the final-thickness slot) is
// S_k or D_k of some surface; its weight is the sum over the surface's terms j that are
// parameter p of Ms[j][k] (the sag: d sag / d c_j = sum_k Ms[j][k] m_k) resp. Mn[j][k] (the
// normal's slopes; zero for c_j == 0, whose term the reference's normal skips,
// zernike.py:213-214)
ORT_INLINE double mono_weight(const AArgs& j, int m, int p) {
  int base = 0;
  for (int si = 0; si < j.n_surf; ++si) {
    const ort_surface s = cst(j.surf)[si];
    const int ms = mono_slots(s);
    if (m < base + ms) {
      const int K = mono_count(s.zm_deg), r = m - base;
      const bool sag = r < K;
      const int k = sag ? r : r - K;
      const int nt = s.n_coef;
      const double* Ms = j.coef + s.zm_off + 2 * K;
      const double* Mn = Ms + (int64_t)nt * K;
      double w = 0.0;
      for (int jt = 0; jt < nt; ++jt) {
        if (!j.zparam || j.zparam[s.coef_off + jt] != p) continue;
        if (sag)
          w = w + Ms[(int64_t)jt * K + k];
        else if (j.zern[s.coef_off + jt].c != 0.0)
          w = w + Mn[(int64_t)jt * K + k];
      }
      return w;
    }
    base += ms;
  }
  return 0.0;
}

// d(slot) / d(parameter p)
ORT_INLINE double slot_weight(const AArgs& j, int slot, int p) {
  const int ns = 3 * j.n_surf;
  if (slot < ns) return j.tan_surf ? j.tan_surf[(int64_t)p * ns + slot] : 0.0;
  if (slot < ns + j.n_zern) {
    if (!j.zparam || j.zparam[slot - ns] != p) return 0.0;
    // a term of a surface served by the monomial slots has no per-term slot of its own
    if (j.mono_on) {
      const int si = term_surface(j, slot - ns);
      if (si >= 0 && mono_slots(cst(j.surf)[si]) > 0) return 0.0;
    }
    return 1.0;
  }
  if (slot == ns + j.n_zern) return j.tan_final ? j.tan_final[p] : 0.0;
  return j.mono_on ? mono_weight(j, slot - ns - j.n_zern - 1, p) : 0.0;
}

// =====================================================================================
// The VJP front end: what ort_trace_{sequential,pupil}_vjp (ort_api.hip vjp_run) and
// ort_host_trace_{sequential,pupil}_vjp (ort_host.cpp host_vjp_run) check and assign alike.
// Each library calls these in order -- vjp_check_call, its own grad_init zeroing and
// empty-batch return, vjp_prepare, then vjp_fill_adjoint or vjp_fill_unrolled by
// params->mode -- with its own refusals (named there) in between. Every refusal here is
// ORT_ERR_ARG but fill_args' own codes.
// =====================================================================================
// The adjoint's parameter slots: radius / conic / vertex z of each surface, each Zernike
// term, the image-space propagation distance, then the monomial-basis slots.
inline int32_t vjp_slot_count(int32_t n_surf, const ort_vjp_params* params) {
  return 3 * n_surf + params->n_zern + 1 + params->n_mono;
}

// The call's pointers and counts. want_in: the caller wants d / d rays_in (some field of
// grad_in is set); nothing: no ray or no derivative is asked for -- the library returns
// ORT_OK once an overwritten gradient (params->grad_init) is zero.
inline int vjp_check_call(const ort_batch* batch, const ort_vjp_params* params,
                          const ort_rays* cotangent, const double* grad,
                          const ort_rays* grad_in, bool& want_in, bool& nothing) {
  if (!batch || !cotangent || !params || params->n_param < 0) return ORT_ERR_ARG;
  want_in = grad_in && (grad_in->x || grad_in->y || grad_in->z || grad_in->L || grad_in->M ||
                        grad_in->N || grad_in->i || grad_in->opd);
  if (params->n_param > 0 && !grad) return ORT_ERR_ARG;
  nothing = batch->n_rays == 0 || (params->n_param == 0 && !want_in);
  return ORT_OK;
}

// the rays to differentiate: resident (rays_in) or generated from pupil samples (px, py
// and the batch's segments, one wavelength row per segment)
inline bool vjp_inputs_ok(bool resident, const ort_rays* rays_in, const double* px,
                          const double* py, const ort_batch* batch) {
  return resident ? rays_in != nullptr : (px && py && batch->seg && !batch->w);
}

// KArgs and the feature bits of a VJP call, with the refusals both libraries make.
inline int vjp_prepare(KArgs& a, uint32_t& feat, const ort_lens* lens, const double* px,
                       const double* py, const ort_rays* rays_in, bool resident,
                       const ort_batch* batch, const ort_options* opt,
                       const ort_vjp_params* params, const double* rec_cotangent,
                       const double* rec) {
  if (rec_cotangent && !rec) return ORT_ERR_ARG;  // intensity rows weight the absorption
  if (!opt || opt->verify_stats) return ORT_ERR_ARG;  // trace launches only
  const int rc = fill_args(a, lens, batch, opt, nullptr, nullptr, nullptr, feat);
  if (rc) return rc;
  if (params->zern_param && (feat & ort::KM_ZERN) == 0) return ORT_ERR_ARG;
  // thin-lens / phase / grating surfaces: the forward-mode VJP only (vjp_ray's all-kinds
  // instantiation carries their interactions in duals; the adjoint has no reverse for them)
  if ((feat & F_IA) && params->mode != ORT_VJP_UNROLLED) return ORT_ERR_ARG;
  if (lens->geometry_mask & ((1u << ORT_GEOM_GRID_SAG) | (1u << ORT_GEOM_NURBS)))
    return ORT_ERR_ARG;  // nor grid sags / NURBS (no derivative sweeps)
  if (resident) {
    a.in = *rays_in;
  } else {
    a.px = px;
    a.py = py;
  }
  return ORT_OK;
}

// ORT_VJP_ADJOINT: the fields of AArgs that are the caller's. The library adds where its
// memory lives (device: tape, partial, slot_sum, need, n_wave, the primal's tape; host:
// need, mono_on).
inline int vjp_fill_adjoint(AArgs& j, const ort_lens* lens, const ort_vjp_params* params,
                            const ort_rays* cotangent, const double* rec_cotangent,
                            const double* rec, double* grad, const ort_rays* grad_in,
                            bool want_in) {
  if (params->n_mono < 0 || (params->n_mono > 0 && !params->zern_param)) return ORT_ERR_ARG;
  // an rms spot size's cotangent folded into the x, y cotangent load: both or neither
  if ((params->rms_stats != nullptr) != (params->rms_grad != nullptr)) return ORT_ERR_ARG;
  j.zparam = params->zern_param;
  j.tan_surf = params->surf_tangent;
  j.tan_final = params->final_tangent;
  j.n_param = params->n_param;
  j.n_zern = params->n_zern;
  j.n_slot = vjp_slot_count(lens->n_surfaces, params);
  j.n_surf = lens->n_surfaces;
  j.cot = *cotangent;
  j.rec_cot = rec_cotangent;
  j.rec = rec;
  if (want_in) j.gin = *grad_in;
  j.grad = grad;
  j.n_mono = params->n_mono;
  j.surf = lens->surfaces;
  j.zern = lens->zern;
  j.coef = lens->coef;
  j.rms_stats = params->rms_stats;
  j.rms_grad = params->rms_grad;
  return ORT_OK;
}

// ORT_VJP_UNROLLED: likewise for JArgs (device: partial; p0 per chunk of tangents)
inline int vjp_fill_unrolled(JArgs& j, const ort_vjp_params* params, const ort_rays* cotangent,
                             const double* rec_cotangent, double* grad, bool want_in) {
  if (want_in) return ORT_ERR_ARG;  // forward mode carries parameter tangents only
  if (params->rms_stats || params->rms_grad) return ORT_ERR_ARG;  // the adjoint's fold only
  j.zparam = params->zern_param;
  j.tan_surf = params->surf_tangent;
  j.tan_final = params->final_tangent;
  j.n_param = params->n_param;
  j.cot = *cotangent;
  j.rec_cot = rec_cotangent;
  j.grad = grad;
  return ORT_OK;
}

}  // namespace ortk
