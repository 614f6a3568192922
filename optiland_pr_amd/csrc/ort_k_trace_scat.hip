// ort_k_trace_scat.hip -- trace kernels for lenses with BSDF scattering surfaces (F_SCAT:
// the scatter step of ort_scatter.h between the interaction and globalize; every Newton
// kind compiled in, 4 specialisations: generated or resident rays, with or without
// per-surface records) and the one-ray-per-lane kernel of ort_bsdf_scatter
// (kernel templates: ort_kernels.h; compiled as its own translation unit)

#include "ort_kernels.h"

namespace ortk {

KernelFn select_trace_scat(uint32_t feat) {
  constexpr uint32_t kAll = 15u;  // every Newton kind
  switch (feat & (F_GEN | F_REC)) {
#define ORT_C(F) \
  case (F):      \
    return trace_kernel<F_SCAT | kAll | (F)>;
    ORT_C(0) ORT_C(F_GEN) ORT_C(F_REC) ORT_C(F_GEN | F_REC)
#undef ORT_C
    default:
      return nullptr;
  }
}

// BaseBSDF.scatter (scatter.py:158-194): ray r of n draws as ray r + ray_offset
__global__ __launch_bounds__(kBlock) void bsdf_scatter_kernel(
    const double* L, const double* M, const double* N, const double* nx, const double* ny,
    const double* nz, int64_t n, int32_t surface, ort_bsdf f, uint64_t seed, int64_t ray_offset,
    int32_t max_attempts, double* oL, double* oM, double* oN, int32_t* status) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n) return;
  double l = L[r], m = M[r], k = N[r];
  const bool ok = ort::bsdf_scatter(f, seed, (uint64_t)(r + ray_offset), (uint32_t)surface,
                                    max_attempts, nx[r], ny[r], nz[r], l, m, k);
  oL[r] = l;
  oM[r] = m;
  oN[r] = k;
  if (!ok && status) atomicOr(status, (int32_t)ORT_STATUS_SCATTER_ATTEMPTS);
}

void launch_bsdf_scatter(const double* L, const double* M, const double* N, const double* nx,
                         const double* ny, const double* nz, int64_t n, int32_t surface,
                         ort_bsdf f, uint64_t seed, int64_t ray_offset, int32_t max_attempts,
                         double* oL, double* oM, double* oN, int32_t* status,
                         hipStream_t stream) {
  const int64_t blocks = (n + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(bsdf_scatter_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, L, M,
                     N, nx, ny, nz, n, surface, f, seed, ray_offset, max_attempts, oL, oM, oN,
                     status);
}

}  // namespace ortk
