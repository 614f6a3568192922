// ort_k_ensemble.hip -- ort_trace_ensemble: V variants of one closed-form lens traced in one
// launch, RayOperand.rms_spot_size reduced per (variant, pair) on the device (tolerancing/
// monte_carlo.py and sensitivity_analysis.py trace thousands of slightly different lenses
// with a few hundred rays each: one lens per launch leaves that bound by launch latency).
//
// Two kernels:
//   trace_ensemble_kernel  one workgroup per (variant, pair, chunk of 256 pupil points), the
//                          three indices from a linear blockIdx.x (V P may pass 65535). The
//                          workgroup's KArgs are the launch's with the lens tables, the
//                          segment, the final thickness and the outputs moved to its variant
//                          and pair, and the rays run through trace_closed_kernel's per-ray
//                          code (closed_ray_in, closed_surfaces: the fast pass, then the exact
//                          re-trace of the lanes that left its ranges), so every ray is
//                          ort_trace_pupil's bit for bit. The variant comes from the block
//                          index alone: the surface record and the optics row stay the
//                          scalar-load batch they are there. Epilogue: rms_epilogue's row
//                          {n, sum x, sum y, M2 about the chunk's own centroid}.
//   ensemble_finish_kernel one workgroup per (variant, pair): rms_finish_block over its rows
//                          in index order -> stats[variant][pair][5].
// Fixed-order sums only (ort_reduce.h); the one atomic is the status word's OR.

#include "ort_kernels.h"  // closed_ray_in, closed_surfaces, rms_epilogue, store_ray
#include "ort_reduce.h"   // rms_finish_block

namespace ortk {
namespace {

struct EArgs {
  int32_t pairs;      // P
  int32_t chunks;     // workgroups per (variant, pair): ceil(n_pupil / 256)
  int32_t cs_stride;  // ort_cs_op records per variant
  int32_t store;      // rays_out given
  const double* final_thickness;  // nullable [V]
};

// The launch's arguments as workgroup (variant v, pair vp - v P) sees them: one lens, one
// segment of n_pupil rays, its own slice of the outputs.
__device__ inline KArgs variant_args(const KArgs& a0, const EArgs& e, uint32_t v, uint32_t vp) {
  KArgs a = a0;
  const int64_t rows = (int64_t)v * a0.n_lambda;
  a.surf = a0.surf + (int64_t)v * a0.n_surf;
  a.optics = a0.optics + rows * a0.n_surf;
  a.n_tab = a0.n_tab + rows * a0.n_mat;
  a.alpha_tab = a0.alpha_tab + rows * a0.n_mat;
  a.cs = a0.cs + (int64_t)v * e.cs_stride;
  if (e.final_thickness) a.final_thickness = cst(e.final_thickness)[v];
  a.seg = a0.seg + vp;
  a.n_seg = 1;
  const int64_t r0 = (int64_t)vp * a0.seg_len;
  if (e.store) {
    a.out.x += r0; a.out.y += r0; a.out.z += r0;
    a.out.L += r0; a.out.M += r0; a.out.N += r0;
    a.out.i += r0; a.out.opd += r0;
  }
  return a;
}

template <uint32_t FEAT>
__global__ __launch_bounds__(kClosedBlock) __attribute__((amdgpu_waves_per_eu(8)))
void trace_ensemble_kernel(const KArgs a0, const EArgs e) {
  static_assert((FEAT & (F_GEN | F_MONO)) == (F_GEN | F_MONO),
                "generated rays, one wavelength row per workgroup");
  // block -> (variant, pair, chunk), wave-uniform (32-bit: the host checks the grid)
  const uint32_t vp = __builtin_amdgcn_readfirstlane(blockIdx.x / (uint32_t)e.chunks);
  const uint32_t chunk = blockIdx.x - vp * (uint32_t)e.chunks;
  const uint32_t v = __builtin_amdgcn_readfirstlane(vp / (uint32_t)e.pairs);
  const KArgs a = variant_args(a0, e, v, vp);

  const int64_t rid = (int64_t)chunk * kClosedBlock + threadIdx.x;  // within the pair
  const bool active = rid < a.seg_len;
  const int64_t r_ld = active ? rid : 0;  // idle lanes compute on ray 0 and store nothing
  int lam = 0;
  double wl = 0.0;
  bool bad = false, geom_bad = false;
  // trace_closed_kernel's two passes
  ort::fast::WaveFlag fbad{0};
  ort::Ray r = closed_ray_in<FEAT, true>(a, r_ld, lam, wl, fbad);
  closed_surfaces<FEAT, true>(a, r, lam, wl, rid, active, fbad, geom_bad);
  bad = ((fbad.m >> (threadIdx.x & 63)) & 1) != 0 || !ort::fast::state_ok(r);
  if (__builtin_expect(bad, 0)) {  // this lane left the fast path's ranges: exact re-trace
    r = closed_ray_in<FEAT, false>(a, r_ld, lam, wl, bad);
    closed_surfaces<FEAT, false>(a, r, lam, wl, rid, active, bad, geom_bad);
  }
  if (a.final_mat >= 0) ort::propagate(r, a.final_thickness, final_alpha<FEAT>(a, lam, wl));
  if (geom_bad && a.status && threadIdx.x == 0) atomicOr(a.status, (int)ORT_STATUS_BAD_GEOMETRY);
  if (a.apod && a.status && threadIdx.x == 0 &&
      (uint32_t)cst(a.apod)->kind > (uint32_t)ORT_APOD_TUKEY)
    atomicOr(a.status, (int)ORT_STATUS_BAD_APODIZATION);
  rms_epilogue(a, r, active, blockIdx.x);  // every thread of the block
  if (!active || !e.store) return;
  double inten = ort::intensity(r);
  // the pupil apodization on the stored intensity, as trace_closed_kernel applies it
  if (a.apod) inten = ort::apodize(*cst(a.apod), a.px[r_ld], a.py[r_ld]) * inten;
  store_ray<StreamStore>(a, rid, r, &inten);
}

__global__ __launch_bounds__(kRmsFinThreads) void ensemble_finish_kernel(const double* part,
                                                                         int chunks,
                                                                         double* stats) {
  __shared__ double lds[kRmsFinThreads / 64 * 3];
  const int64_t vp = blockIdx.x;
  rms_finish_block<kRmsFinThreads, kRmsFinRows>(part + vp * chunks * 4, chunks, stats + vp * 5,
                                                nullptr, lds);
}

constexpr int64_t kMaxGrid = 0x7fffffff;

int64_t ensemble_chunks(int64_t n_pupil) { return (n_pupil + kClosedBlock - 1) / kClosedBlock; }

// V P chunks, or -1 when the arguments or the grid are out of range
int64_t ensemble_blocks(const ort_ensemble* e, int64_t n_pupil) {
  if (!e || e->n_variants < 1 || e->pairs < 1 || e->cs_stride < 0 || n_pupil < 1) return -1;
  const int64_t vp = (int64_t)e->n_variants * e->pairs;
  const int64_t chunks = ensemble_chunks(n_pupil);
  if (vp > kMaxGrid || chunks > kMaxGrid / vp) return -1;
  return vp * chunks;
}

}  // namespace
}  // namespace ortk

using namespace ortk;

extern "C" {

int64_t ort_ensemble_workspace_size(const ort_ensemble* e, int64_t n_pupil) {
  const int64_t blocks = ensemble_blocks(e, n_pupil);
  return blocks < 0 ? (int64_t)ORT_ERR_ARG : blocks * 4 * (int64_t)sizeof(double);
}

int ort_trace_ensemble(const ort_lens* lens, const ort_ensemble* e, const double* px,
                       const double* py, int64_t n_pupil, const ort_segment* seg,
                       const ort_apodization* apod, ort_rays* rays_out, double* stats,
                       void* workspace, int64_t workspace_size, int32_t* status, void* stream) {
  const int64_t blocks = ensemble_blocks(e, n_pupil);
  if (blocks < 0 || !lens || !px || !py || !seg || !stats || !workspace) return ORT_ERR_ARG;
  if (workspace_size < blocks * 4 * (int64_t)sizeof(double)) return ORT_ERR_ARG;
  if (lens->n_surfaces < 1) return ORT_ERR_ARG;
  // closed-form lenses with refractive / reflective surfaces only: anything else is the
  // one-lens entry points' (the caller falls back to them)
  if (lens->geometry_mask & ~((1u << ORT_GEOM_PLANE) | (1u << ORT_GEOM_STANDARD)))
    return ORT_ERR_ARG;
  if (lens->interaction_mask & ~(1u << ORT_IA_REFRACT_REFLECT)) return ORT_ERR_ARG;
  if (rays_out && (!rays_out->x || !rays_out->y || !rays_out->z || !rays_out->L ||
                   !rays_out->M || !rays_out->N || !rays_out->i || !rays_out->opd))
    return ORT_ERR_ARG;
  // the lens and one (variant, pair) as a one-segment batch through the shared front end
  ort_batch b{};
  b.n_rays = n_pupil;
  b.seg_len = n_pupil;
  b.group_len = n_pupil;
  b.n_seg = 1;
  b.seg = seg;
  b.apod = apod;
  const ort_options opt{ORT_NEWTON_SCHEDULE, 0, nullptr, 0, 0};
  KArgs a{};
  uint32_t feat = 0;
  const int rc = fill_args(a, lens, &b, &opt, nullptr, nullptr, status, feat);
  if (rc) return rc;
  a.px = px;
  a.py = py;
  if (rays_out) a.out = *rays_out;
  a.rms_part = (double*)workspace;
  EArgs ea{};
  ea.pairs = e->pairs;
  ea.chunks = (int32_t)ensemble_chunks(n_pupil);
  ea.cs_stride = e->cs_stride;
  ea.store = rays_out != nullptr;
  ea.final_thickness = e->final_thickness;
  hipStream_t s = (hipStream_t)stream;
  if (status && hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess)
    return ORT_ERR_LAUNCH;
  // the plain axial form where every variant is plain and axial (the caller ANDs the
  // flags over the variants), else the generic form, which is right for any lens
  const uint32_t plain = ORT_LENS_AXIAL | ORT_LENS_PLAIN;
  auto fn = (lens->frame_flags & plain) == plain
                ? trace_ensemble_kernel<F_GEN | F_MONO | F_AXIAL | F_PLAIN>
                : trace_ensemble_kernel<F_GEN | F_MONO>;
  hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(kClosedBlock), 0, s, a, ea);
  hipLaunchKernelGGL(ensemble_finish_kernel, dim3((unsigned)(blocks / ea.chunks)),
                     dim3(kRmsFinThreads), 0, s, (const double*)workspace, ea.chunks, stats);
  return hipGetLastError() == hipSuccess ? ORT_OK : ORT_ERR_LAUNCH;
}

}  // extern "C"
