// ort_k_huygens.hip -- the Huygens-Fresnel PSF summation on the device
// (psf/huygens_fresnel_strategies.py:97-172, the reference's Numba double loop over
// image points x pupil points; the term itself is ort_huygens.h).
//
// huygens_partial_kernel: one image point per lane, one (image tile, pupil chunk) per
//   workgroup: workgroup b works on tile b / n_chunks of kHuyThreads image points against
//   pupil points [c, c + 1) * ORT_HUYGENS_CHUNK, c = b % n_chunks. A 128 x 128 image alone
//   is 256 waves for 1,024 SIMDs; split over the pupil (12.9k points = 26 chunks) it is
//   6.6k waves. The pupil index is wave-uniform, so the five doubles of a pupil point come
//   through scalar loads into SGPRs (the chunk is read once per workgroup from L2, off the
//   vector pipe; nothing is staged in LDS and there is no barrier). Each lane sums its
//   chunk in index order and writes one complex partial to part[c][p].
// huygens_final_kernel: one image point per thread adds its partials in chunk order and
//   writes |field|^2. No atomics; the chunk size is a compile-time constant, so the value
//   of an image point depends on nothing but its own coordinates and the pupil arrays.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ort_huygens.h"

namespace ortk {
namespace {

constexpr int kHuyThreads = 256;  // image points per tile (ort_reduce.h kRedThreads)

struct HuyArgs {
  const double* ix;
  const double* iy;
  const double* iz;
  int64_t n_image;
  const double* px;
  const double* py;
  const double* pz;
  const double* amp;
  const double* opd;
  int64_t n_pupil;
  double inv_wl;
  double inv_rp;
  double* part;  // [n_chunks][n_image][2]
  double* psf;   // [n_image]
  int32_t n_chunks;
};

__global__ __launch_bounds__(kHuyThreads) void huygens_partial_kernel(const HuyArgs a) {
  const int64_t tile = blockIdx.x / (uint32_t)a.n_chunks;
  const int64_t c = blockIdx.x - tile * (uint32_t)a.n_chunks;
  const int64_t p = tile * kHuyThreads + threadIdx.x;
  if (p >= a.n_image) return;
  const int64_t j0 = c * ORT_HUYGENS_CHUNK;
  const int64_t j1 = j0 + ORT_HUYGENS_CHUNK < a.n_pupil ? j0 + ORT_HUYGENS_CHUNK : a.n_pupil;
  double re, im;
  ort::huygens_chunk(a.ix[p], a.iy[p], a.iz[p], a.px, a.py, a.pz, a.amp, a.opd, j0, j1,
                     a.inv_wl, a.inv_rp, re, im);
  double* o = a.part + (c * a.n_image + p) * 2;
  o[0] = re;
  o[1] = im;
}

__global__ __launch_bounds__(kHuyThreads) void huygens_final_kernel(const HuyArgs a) {
  const int64_t p = (int64_t)blockIdx.x * kHuyThreads + threadIdx.x;
  if (p >= a.n_image) return;
  double re = 0.0, im = 0.0;
  for (int64_t c = 0; c < a.n_chunks; ++c) {
    const double* q = a.part + (c * a.n_image + p) * 2;
    re += q[0];
    im += q[1];
  }
  a.psf[p] = re * re + im * im;
}

int64_t huygens_chunks(int64_t n_pupil) {
  return n_pupil > 0 ? (n_pupil + ORT_HUYGENS_CHUNK - 1) / ORT_HUYGENS_CHUNK : 1;
}

}  // namespace
}  // namespace ortk

using namespace ortk;

extern "C" {

int64_t ort_huygens_workspace_size(int64_t n_image, int64_t n_pupil) {
  if (n_image < 0 || n_pupil < 0) return ORT_ERR_ARG;
  const int64_t chunks = huygens_chunks(n_pupil);
  const int64_t per = 2 * (int64_t)sizeof(double);
  if (n_image > 0 && chunks > INT64_MAX / per / n_image) return ORT_ERR_ARG;
  return chunks * n_image * per;
}

int ort_huygens_psf(const double* ix, const double* iy, const double* iz, int64_t n_image,
                    const double* px, const double* py, const double* pz,
                    const double* amp, const double* opd_mm, int64_t n_pupil,
                    double wavelength_mm, double rp, double* psf, void* workspace,
                    int64_t workspace_size, void* stream) {
  if (n_image < 0 || n_pupil < 0 || !(wavelength_mm > 0.0)) return ORT_ERR_ARG;
  if (n_image > 0 && (!ix || !iy || !iz || !psf)) return ORT_ERR_ARG;
  if (n_pupil > 0 && (!px || !py || !pz || !amp || !opd_mm)) return ORT_ERR_ARG;
  const int64_t need = ort_huygens_workspace_size(n_image, n_pupil);
  if (need < 0 || workspace_size < need || (need > 0 && !workspace)) return ORT_ERR_ARG;
  if (n_image == 0) return ORT_OK;
  const int64_t chunks = huygens_chunks(n_pupil);
  const int64_t tiles = (n_image + kHuyThreads - 1) / kHuyThreads;
  if (chunks > 0x7fffffff || tiles > 0x7fffffff / chunks) return ORT_ERR_ARG;
  HuyArgs a{};
  a.ix = ix;
  a.iy = iy;
  a.iz = iz;
  a.n_image = n_image;
  a.px = px;
  a.py = py;
  a.pz = pz;
  a.amp = amp;
  a.opd = opd_mm;
  a.n_pupil = n_pupil;
  a.inv_wl = 1.0 / wavelength_mm;
  a.inv_rp = 1.0 / rp;
  a.part = (double*)workspace;
  a.psf = psf;
  a.n_chunks = (int32_t)chunks;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(huygens_partial_kernel, dim3((unsigned)(tiles * chunks)),
                     dim3(kHuyThreads), 0, s, a);
  hipLaunchKernelGGL(huygens_final_kernel, dim3((unsigned)tiles), dim3(kHuyThreads), 0, s, a);
  return hipGetLastError() == hipSuccess ? ORT_OK : ORT_ERR_LAUNCH;
}

}  // extern "C"
