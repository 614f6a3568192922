/*
 * optiland_host.h -- C ABI of the host (CPU) build of the trace core: the CPU dispatch key
 * of the torch custom op torch.ops.ort.trace_sequential and of its VJP (SURVEY.md 8b:
 * "registered for the CUDA(HIP) and CPU dispatch keys").
 *
 * It replaces the same reference interfaces as ort_trace_sequential / ort_trace_pupil /
 * ort_rms_spot (optiland_rt.h):
 *   optiland/surfaces/surface_group.py:232-244      SurfaceGroup.trace(rays, skip)
 *   optiland/surfaces/standard_surface.py:186-233   Surface.trace (real-ray branch)
 * for rays held in HOST memory -- the reference's own default (backend/torch_backend.py:
 * 66-77 device "cpu"; its test fixture tests/conftest.py:5-19 runs the torch backend on the
 * CPU), and its backward under autograd (optimization/optimizer/torch/base.py:116-131).
 *
 * Same structs as optiland_rt.h, every pointer a HOST pointer. The per-ray arithmetic is
 * the GPU kernels' own source (csrc/ort_core.h, ort_interact.h, ort_material.h, the argument
 * layer of csrc/ort_args.h and the derivative sweeps of csrc/ort_sweep.h) compiled with g++ -ffp-contract=off, so a trace
 * gives the GPU's bits. Newton surfaces follow the reference's global stop rule
 * (newton_raphson.py:137-166: stop when max |f| < tol over the rays of one trace call)
 * directly: every Newton group (batch->group_len rays) is stepped in lockstep, as the
 * reference evaluates it, and the update counts it made are written to `updates`. Calls
 * are synchronous; OpenMP threads split the rays (results do not depend on the thread
 * count: every reduction runs in a fixed order).
 */
#ifndef OPTILAND_HOST_H
#define OPTILAND_HOST_H

#include "optiland_rt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORT_HOST_ABI_VERSION 3

int ort_host_abi_version(void);

/* lens->frame_flags: ORT_LENS_AXIAL and ORT_LENS_PLAIN (optiland_rt.h) are both
 * accepted and ignored, as is lens->form_flags (ORT_LENS_SPHERES): the host library has
 * one form of every trace. */

/* ort_trace_sequential on host memory. updates (nullable): int32 [n_groups][n_surfaces],
 * the Newton updates the reference's stop rule made per (group, surface) (0 for closed-form
 * surfaces) -- the schedule ort_host_trace_sequential_vjp replays. opt->sched and
 * opt->newton_mode are ignored (the stop rule is evaluated exactly); opt->start_surface is
 * the SurfaceGroup.trace skip. status (nullable): ort_status bits (Zernike / Chebyshev
 * range errors, unknown geometry). rays_out may alias rays_in. Returns 0 or an ort_error. */
int ort_host_trace_sequential(const ort_lens* lens, const ort_rays* rays_in,
                              ort_rays* rays_out, const ort_batch* batch,
                              const ort_options* opt, double* rec, int32_t* updates,
                              int32_t* status);

/* ort_trace_sequential_vjp on host memory, with the same parameters (ADJOINT or UNROLLED
 * mode; params->workspace unused: the host allocates its own scratch; params->slot_need
 * nullable). opt->sched: the `updates` the primal host trace reported. */
int ort_host_trace_sequential_vjp(const ort_lens* lens, const ort_rays* rays_in,
                                  const ort_batch* batch, const ort_options* opt,
                                  const ort_vjp_params* params, const ort_rays* cotangent,
                                  const double* rec_cotangent, const double* rec,
                                  double* grad, const ort_rays* grad_in);

/* ort_trace_pupil on host memory (v2): rays generated from the pupil samples px, py by the
 * batch's segments (ray r of segment r / seg_len; pupil sample r with pupil_per_ray, else
 * r - segment * seg_len; ray_generator.py:28-106 through the GPU's generate_ray), then
 * traced in Newton groups of batch->group_len rays with the reference's stop rule as in
 * ort_host_trace_sequential (updates: [n_groups][n_surfaces]). No records, no start surface,
 * no per-ray wavelengths; n_rays must be n_seg * seg_len. Replaces RealRayTracer.trace
 * (raytrace/real_ray_tracer.py:37-97) for host tensors. */
int ort_host_trace_pupil(const ort_lens* lens, const double* px, const double* py,
                         ort_rays* rays_out, const ort_batch* batch, const ort_options* opt,
                         int32_t* updates, int32_t* status);

/* ort_trace_pupil_vjp on host memory (v2): the adjoint / forward-mode sweeps of the pupil
 * trace (generation included, not differentiated), opt->sched = the primal's updates. */
int ort_host_trace_pupil_vjp(const ort_lens* lens, const double* px, const double* py,
                             const ort_batch* batch, const ort_options* opt,
                             const ort_vjp_params* params, const ort_rays* cotangent,
                             double* grad);

/* ort_rms_spot / ort_rms_spot_vjp on host memory (v2): RayOperand.rms_spot_size
 * (optimization/operand/ray.py:300-340), stats = n, mean x, mean y, rms, max radius; pairwise
 * sums in a fixed order (n = 0: count 0, the rest NaN). */
int ort_host_rms_spot(const double* x, const double* y, int64_t n, double* stats, double* rms);
int ort_host_rms_spot_vjp(const double* x, const double* y, int64_t n, const double* stats,
                          const double* grad_out, double* gx, double* gy);

/* ort_huygens_psf on host memory (v3): the Huygens-Fresnel sum of
 * psf/huygens_fresnel_strategies.py:97-172 with the kernel's own term (csrc/ort_huygens.h)
 * and its summation order -- per image point the pupil in chunks of ORT_HUYGENS_CHUNK, each
 * from zero in index order, the chunk sums added in chunk order -- OpenMP over the image
 * points (the value does not depend on the thread count). Same argument checks as
 * ort_huygens_psf, no workspace. */
int ort_host_huygens_psf(const double* ix, const double* iy, const double* iz, int64_t n_image,
                         const double* px, const double* py, const double* pz,
                         const double* amp, const double* opd_mm, int64_t n_pupil,
                         double wavelength_mm, double rp, double* psf);

/* ort_irradiance_bin / ort_irradiance_bin_vjp on host memory (added within v3): the kernels' own pixel
 * search, weights, quantisation and finish (csrc/ort_irradiance.h); the integer sums make the
 * result independent of the thread count and identical to the device's, bit for bit. Same
 * argument checks, no workspace. */
int ort_host_irradiance_bin(const double* x, const double* y, const double* power, int64_t n,
                            const double* x_edges, int64_t nx, const double* y_edges,
                            int64_t ny, int32_t mode, double pixel_area, double* out);
int ort_host_irradiance_bin_vjp(const double* x, const double* y, const double* power,
                                int64_t n, const double* x_edges, int64_t nx,
                                const double* y_edges, int64_t ny, double pixel_area,
                                const double* grad_out, double* grad_x, double* grad_y,
                                double* grad_power);

/* ort_dft_psf on host memory (added within v3): the kernels' own terms (csrc/ort_dft.h) in
 * the kernels' order -- T = g R summed over k, then |R^T T|^2 summed over j, each from zero in
 * index order -- OpenMP over the rows (the value does not depend on the thread count). Same
 * argument checks as ort_dft_psf, no workspace. */
int ort_host_dft_psf(const double* amp, const double* opd_waves, int64_t batch, int64_t n,
                     int64_t m, double pad, double* out);

/* ort_sampled_otf on host memory (added within v3): the kernel's own term
 * (csrc/ort_sampled_otf.h) in the kernel's order -- per (batch entry, frequency) the pupil in
 * chunks of ORT_SAMPLED_OTF_CHUNK points, each chunk's terms added as the workgroup adds
 * them (64 lanes pairwise: neighbours, pairs of neighbours, ...; then the four groups of 64
 * in index order from zero), the chunk sums in chunk order from zero -- OpenMP over the
 * (batch entry, frequency) pairs (the value does not depend on the thread count). Same
 * argument checks as ort_sampled_otf, no workspace. */
int ort_host_sampled_otf(const double* x, const double* y, int64_t n_pupil,
                         const double* intensity, const double* opd_waves, int64_t n_batch,
                         const ort_zernike_term* terms, const double* radial,
                         const double* coeffs, int64_t n_terms, const double* shift_x,
                         const double* shift_y, int64_t n_freq, double* otf);

/* ort_trace_pupil_polarized / ort_trace_sequential_polarized on host memory (added within
 * v3): the kernels' per-ray polarization code (csrc/ort_polar.h) inside the host trace, so
 * the ray geometry is ort_host_trace_pupil's / ort_host_trace_sequential's bit for bit.
 * pol->coatings and pol->p_out are host pointers; rec: [n_rec][8][n_rays] or NULL. Same
 * argument checks as the device entry points. */
int ort_host_trace_pupil_polarized(const ort_lens* lens, const double* px, const double* py,
                                   ort_rays* rays_out, const ort_batch* batch,
                                   const ort_options* opt, double* rec, int32_t* updates,
                                   int32_t* status, const ort_polarization* pol);
int ort_host_trace_sequential_polarized(const ort_lens* lens, const ort_rays* rays_in,
                                        ort_rays* rays_out, const ort_batch* batch,
                                        const ort_options* opt, double* rec, int32_t* updates,
                                        int32_t* status, const ort_polarization* pol);

/* ort_generate_rays on host memory (added within v3): the rays ort_host_trace_pupil
 * generates, without a trace (NULL fields of rays_out are skipped). */
int ort_host_generate_rays(const double* px, const double* py, ort_rays* rays_out,
                           const ort_batch* batch);

/* ort_trace_pupil_scatter / ort_trace_sequential_scatter / ort_bsdf_scatter on host memory
 * (added within v3): the kernels' scatter step (csrc/ort_scatter.h) inside the host trace.
 * scat->bsdf is a host pointer; same argument checks as the device entry points. */
int ort_host_trace_pupil_scatter(const ort_lens* lens, const double* px, const double* py,
                                 ort_rays* rays_out, const ort_batch* batch,
                                 const ort_options* opt, double* rec, int32_t* updates,
                                 int32_t* status, const ort_scatter* scat);
int ort_host_trace_sequential_scatter(const ort_lens* lens, const ort_rays* rays_in,
                                      ort_rays* rays_out, const ort_batch* batch,
                                      const ort_options* opt, double* rec, int32_t* updates,
                                      int32_t* status, const ort_scatter* scat);
int ort_host_bsdf_scatter(const double* L, const double* M, const double* N, const double* nx,
                          const double* ny, const double* nz, int64_t n, int32_t surface_index,
                          const ort_bsdf* bsdf, const ort_scatter* scat, double* out_L,
                          double* out_M, double* out_N, int32_t* status);

/* threads used by the calls (OpenMP; <= 0: the OpenMP default) */
void ort_host_set_threads(int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* OPTILAND_HOST_H */
