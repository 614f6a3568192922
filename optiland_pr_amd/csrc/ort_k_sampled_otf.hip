// ort_k_sampled_otf.hip -- SampledMTF's overlap sum on the device (mtf/sampled.py:162-205,
// the reference's Python loop over frequencies of whole-array operations; the term itself is
// ort_sampled_otf.h).
//
// sampled_otf_partial_kernel: one pupil point per lane, one (batch entry, frequency, chunk)
//   per workgroup: workgroup w works on chunk c = w % n_chunks of pair w / n_chunks = b *
//   n_freq + f, pupil points [c, c + 1) * ORT_SAMPLED_OTF_CHUNK. The shear, the batch entry's
//   coefficients and the term table are workgroup-uniform and come through scalar loads; a
//   lane past the pupil's end adds 0.0 and stays in the reduction, so every wave reduces with
//   all lanes active (ort_reduce.h's DPP tree: pairs, quads, ... in one fixed order). The
//   chunk's complex sum goes to part[w][2].
// sampled_otf_final_kernel: one (batch entry, frequency) per thread adds its rows in chunk
//   order from 0.0 and writes otf[b][f][2]. No atomics; the chunk size is a compile-time
//   constant, so a value depends on its own pupil, coefficients and shear alone -- not on the
//   other frequencies or batch entries of the call.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ort_args.h"
#include "ort_reduce.h"
#include "ort_sampled_otf.h"

namespace ortk {
namespace {

static_assert(ORT_SAMPLED_OTF_CHUNK == kRedThreads, "one lane per point of a chunk");

struct SotfArgs {
  const double* x;
  const double* y;
  const double* inten;  // [n_batch][n_pupil]
  const double* opd;    // [n_batch][n_pupil]
  const ort_zernike_term* terms;
  const double* radial;
  const double* coef;  // [n_batch][n_terms]
  const double* sx;
  const double* sy;
  int64_t n_pupil;
  int64_t n_pairs;  // n_batch * n_freq
  double* part;     // [n_pairs][n_chunks][2]
  double* otf;      // [n_pairs][2]
  int32_t n_freq;
  int32_t n_terms;
  int32_t n_chunks;
};

__global__ __launch_bounds__(kRedThreads) void sampled_otf_partial_kernel(const SotfArgs a) {
  const int64_t pair = blockIdx.x / (uint32_t)a.n_chunks;
  const int64_t c = blockIdx.x - pair * (uint32_t)a.n_chunks;
  const int64_t b = pair / a.n_freq;
  const int64_t f = pair - b * a.n_freq;
  const int64_t j = c * ORT_SAMPLED_OTF_CHUNK + threadIdx.x;
  double v[2] = {0.0, 0.0};
  if (j < a.n_pupil) {
    const double sx = cst(a.sx)[f], sy = cst(a.sy)[f];
    const int64_t row = b * a.n_pupil + j;
    ort::sampled_otf_term(a.x[j], a.y[j], a.inten[row], a.opd[row], sx, sy, cst(a.terms),
                          cst(a.radial), cst(a.coef) + b * a.n_terms, a.n_terms, v[0], v[1]);
  }
  const double* rows = block_sum_lead<2>(v);
  if (threadIdx.x == 0) {
    double* o = a.part + (int64_t)blockIdx.x * 2;
    o[0] = block_sum_at<2>(rows, 0);
    o[1] = block_sum_at<2>(rows, 1);
  }
}

__global__ __launch_bounds__(kRedThreads) void sampled_otf_final_kernel(const SotfArgs a) {
  const int64_t pair = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
  if (pair >= a.n_pairs) return;
  const double* q = a.part + pair * a.n_chunks * 2;
  double re = 0.0, im = 0.0;
  for (int64_t c = 0; c < a.n_chunks; ++c) {
    re += q[2 * c];
    im += q[2 * c + 1];
  }
  a.otf[2 * pair] = re;
  a.otf[2 * pair + 1] = im;
}

}  // namespace
}  // namespace ortk

using namespace ortk;

extern "C" {

int64_t ort_sampled_otf_workspace_size(int64_t n_batch, int64_t n_freq, int64_t n_pupil) {
  if (n_batch < 0 || n_freq < 0 || n_pupil < 0) return ORT_ERR_ARG;
  const int64_t chunks = ort::sampled_otf_chunks(n_pupil);
  const int64_t per = 2 * (int64_t)sizeof(double);
  if (n_batch > 0 && n_freq > INT64_MAX / per / chunks / n_batch) return ORT_ERR_ARG;
  return n_batch * n_freq * chunks * per;
}

int ort_sampled_otf(const double* x, const double* y, int64_t n_pupil, const double* intensity,
                    const double* opd_waves, int64_t n_batch, const ort_zernike_term* terms,
                    const double* radial, const double* coeffs, int64_t n_terms,
                    const double* shift_x, const double* shift_y, int64_t n_freq, double* otf,
                    void* workspace, int64_t workspace_size, void* stream) {
  const int rc = sampled_otf_check(x, y, n_pupil, intensity, opd_waves, n_batch, terms, radial,
                                   coeffs, n_terms, shift_x, shift_y, n_freq, otf);
  if (rc != ORT_OK) return rc;
  const int64_t need = ort_sampled_otf_workspace_size(n_batch, n_freq, n_pupil);
  if (need < 0 || workspace_size < need || (need > 0 && !workspace)) return ORT_ERR_ARG;
  if (n_batch == 0 || n_freq == 0) return ORT_OK;
  const int64_t chunks = ort::sampled_otf_chunks(n_pupil);
  const int64_t pairs = n_batch * n_freq;
  if (chunks > 0x7fffffff || pairs > 0x7fffffff / chunks) return ORT_ERR_ARG;
  SotfArgs a{};
  a.x = x;
  a.y = y;
  a.inten = intensity;
  a.opd = opd_waves;
  a.terms = terms;
  a.radial = radial;
  a.coef = coeffs;
  a.sx = shift_x;
  a.sy = shift_y;
  a.n_pupil = n_pupil;
  a.n_pairs = pairs;
  a.part = (double*)workspace;
  a.otf = otf;
  a.n_freq = (int32_t)n_freq;
  a.n_terms = (int32_t)n_terms;
  a.n_chunks = (int32_t)chunks;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sampled_otf_partial_kernel, dim3((unsigned)(pairs * chunks)),
                     dim3(kRedThreads), 0, s, a);
  hipLaunchKernelGGL(sampled_otf_final_kernel,
                     dim3((unsigned)((pairs + kRedThreads - 1) / kRedThreads)),
                     dim3(kRedThreads), 0, s, a);
  return hipGetLastError() == hipSuccess ? ORT_OK : ORT_ERR_LAUNCH;
}

}  // extern "C"
