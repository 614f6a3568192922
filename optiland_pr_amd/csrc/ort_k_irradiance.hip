// ort_k_irradiance.hip -- IncoherentIrradiance's binning on the device
// (analysis/irradiance.py:243-330; the per-ray pieces are ort_irradiance.h).
//
// The sum of a pixel is a 64-bit integer in units of 2^-E, so it depends on nothing but the
// multiset of contributions to that pixel: permuting the rays or changing the grid, the
// stream or the tiling leaves every bit unchanged. Four stream operations, no host
// synchronisation:
//   hipMemsetAsync      the workspace (cmax, integer image, flags) to zero
//   irr_cmax_kernel     one ray per lane, grid-stride: the largest finite |contribution| as
//                       its bit pattern (integer max: order-independent), one LDS max per
//                       lane and one global max per workgroup
//   irr_bin_kernel      one ray per lane, grid-stride: E from (n, cmax), each contribution
//                       rounded once to an integer. Images of up to
//                       ORT_IRRADIANCE_TILE_PIXELS pixels: a private int64 tile in LDS per
//                       workgroup (ds_add_u64), its non-zero entries flushed once with
//                       global 64-bit integer atomics. Larger images: the global atomics
//                       directly (they run in L2). Lanes of a wave that hit one pixel are
//                       summed across the wave first and one lane adds (the contention case:
//                       a focused spot puts whole waves on one address). A non-finite
//                       contribution sets its pixel's flag instead.
//   irr_finish_kernel   one pixel per lane: integer -> fp64, 2^-E, / area; NaN where flagged
// irr_vjp_kernel (ORT_BIN_BILINEAR's backward) is a gather, one ray per lane, no atomics.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ort_irradiance.h"

namespace ortk {
namespace {

constexpr int kIrrThreads = 1024;      // one workgroup per CU holds a full tile: 16 waves
constexpr int kIrrSmallThreads = 256;  // finish / VJP
constexpr int kIrrCombineRounds = 4;   // distinct pixels peeled per wave and contribution
constexpr int kIrrCombineMin = 16;     // same-pixel lanes of a wave worth a cross-lane sum
constexpr int64_t kIrrHeader = 64;     // bytes in front of the integer image

struct IrrArgs {
  ort::IrrGrid g;
  const double* x;
  const double* y;
  const double* p;
  int64_t n;
  int64_t rounds;  // grid-stride rounds (the same for every workgroup: no lane leaves early)
  unsigned long long* cmax;  // workspace: [0] the bits of cmax
  unsigned long long* acc;   // [npix] integer sums
  uint32_t* flags;           // [npix] non-finite marks
  double* out;
  double area;
  int32_t log2_n;
};

__global__ __launch_bounds__(kIrrThreads) void irr_cmax_kernel(const IrrArgs a) {
  __shared__ unsigned long long s_max;
  if (threadIdx.x == 0) s_max = 0;
  __syncthreads();
  unsigned long long m = 0;
  const int64_t stride = (int64_t)gridDim.x * kIrrThreads;
  for (int64_t i = (int64_t)blockIdx.x * kIrrThreads + threadIdx.x; i < a.n; i += stride) {
    int64_t pix[4];
    double c[4];
    const int k = ort::irr_contributions(a.g, a.x[i], a.y[i], a.p[i], pix, c);
    for (int j = 0; j < 4; ++j)
      if (j < k && ort::irr_finite(c[j])) {
        const unsigned long long b = ort::irr_abs_bits(c[j]);
        m = b > m ? b : m;
      }
  }
  if (m) atomicMax(&s_max, m);
  __syncthreads();
  if (threadIdx.x == 0 && s_max) atomicMax(a.cmax, s_max);
}

// One contribution per lane (has: this lane holds one) added to dst[pix]. Every lane of the
// wave calls this together.
__device__ inline void irr_add(unsigned long long* dst, int64_t pix, int64_t q, bool has) {
  unsigned long long rem = __ballot(has);
  const int lane = threadIdx.x & 63;
  for (int r = 0; rem && r < kIrrCombineRounds; ++r) {
    const int lead = __ffsll((long long)rem) - 1;
    const int64_t lp = __shfl(pix, lead);
    const bool mine = has && pix == lp;
    const unsigned long long m = __ballot(mine);
    if (__popcll(m) < kIrrCombineMin) break;
    int64_t v = mine ? q : 0;
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    if (lane == lead && v) atomicAdd(dst + lp, (unsigned long long)v);
    has = has && !mine;
    rem &= ~m;
  }
  if (has) atomicAdd(dst + pix, (unsigned long long)q);
}

template <bool kTile>
__global__ __launch_bounds__(kIrrThreads) void irr_bin_kernel(const IrrArgs a) {
  extern __shared__ unsigned long long s_tile[];
  const int64_t npix = a.g.nx * a.g.ny;
  if (kTile) {
    for (int64_t j = threadIdx.x; j < npix; j += kIrrThreads) s_tile[j] = 0;
    __syncthreads();
  }
  unsigned long long* dst = kTile ? s_tile : a.acc;
  const int E = ort::irr_exponent(*a.cmax, a.log2_n);
  const int64_t stride = (int64_t)gridDim.x * kIrrThreads;
  int64_t i = (int64_t)blockIdx.x * kIrrThreads + threadIdx.x;
  for (int64_t r = 0; r < a.rounds; ++r, i += stride) {
    int64_t pix[4] = {0, 0, 0, 0};
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    int k = 0;
    if (i < a.n) k = ort::irr_contributions(a.g, a.x[i], a.y[i], a.p[i], pix, c);
    const int kmax = a.g.mode == ORT_BIN_HISTOGRAM ? 1 : 4;
    for (int j = 0; j < kmax; ++j) {
      bool has = j < k;
      int64_t q = 0;
      if (has) {
        if (ort::irr_finite(c[j])) {
          q = ort::irr_quantise(c[j], E);
          has = q != 0;
        } else {
          atomicOr(a.flags + pix[j], 1u);
          has = false;
        }
      }
      irr_add(dst, pix[j], q, has);
    }
  }
  if (kTile) {
    __syncthreads();
    for (int64_t j = threadIdx.x; j < npix; j += kIrrThreads) {
      const unsigned long long v = s_tile[j];
      if (v) atomicAdd(a.acc + j, v);
    }
  }
}

__global__ __launch_bounds__(kIrrSmallThreads) void irr_finish_kernel(const IrrArgs a) {
  const int64_t j = (int64_t)blockIdx.x * kIrrSmallThreads + threadIdx.x;
  if (j >= a.g.nx * a.g.ny) return;
  const int E = ort::irr_exponent(*a.cmax, a.log2_n);
  a.out[j] = ort::irr_finish((int64_t)a.acc[j], a.flags[j], E, ort::irr_area(a.g, a.area));
}

struct IrrVjpArgs {
  ort::IrrGrid g;
  const double* x;
  const double* y;
  const double* p;
  int64_t n;
  const double* grad;
  double area;
  double* gx;
  double* gy;
  double* gp;
};

__global__ __launch_bounds__(kIrrSmallThreads) void irr_vjp_kernel(const IrrVjpArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kIrrSmallThreads + threadIdx.x;
  if (i >= a.n) return;
  double gx, gy, gp;
  ort::irr_vjp(a.g, a.grad, a.x[i], a.y[i], a.p[i], ort::irr_area(a.g, a.area), gx, gy, gp);
  a.gx[i] = gx;
  a.gy[i] = gy;
  a.gp[i] = gp;
}

bool irr_grid_ok(int64_t nx, int64_t ny, int32_t mode) {
  if (mode != ORT_BIN_HISTOGRAM && mode != ORT_BIN_BILINEAR) return false;
  const int64_t lo = mode == ORT_BIN_BILINEAR ? 2 : 1;
  if (nx < lo || ny < lo || nx > ORT_IRRADIANCE_MAX_PIXELS || ny > ORT_IRRADIANCE_MAX_PIXELS)
    return false;
  return nx * ny <= ORT_IRRADIANCE_MAX_PIXELS;
}

}  // namespace
}  // namespace ortk

using namespace ortk;

extern "C" {

int64_t ort_irradiance_workspace_size(int64_t nx, int64_t ny) {
  if (nx < 1 || ny < 1 || nx > ORT_IRRADIANCE_MAX_PIXELS || ny > ORT_IRRADIANCE_MAX_PIXELS ||
      nx * ny > ORT_IRRADIANCE_MAX_PIXELS)
    return ORT_ERR_ARG;
  return kIrrHeader + nx * ny * (int64_t)(sizeof(unsigned long long) + sizeof(uint32_t));
}

int ort_irradiance_bin(const double* x, const double* y, const double* power, int64_t n,
                       const double* x_edges, int64_t nx, const double* y_edges, int64_t ny,
                       int32_t mode, double pixel_area, double* out, void* workspace,
                       int64_t workspace_size, void* stream) {
  if (n < 0 || !irr_grid_ok(nx, ny, mode) || !x_edges || !y_edges || !out) return ORT_ERR_ARG;
  if (n > 0 && (!x || !y || !power)) return ORT_ERR_ARG;
  const int64_t need = ort_irradiance_workspace_size(nx, ny);
  if (need < 0 || workspace_size < need || !workspace) return ORT_ERR_ARG;
  const int64_t npix = nx * ny;
  hipStream_t s = (hipStream_t)stream;
  IrrArgs a{};
  a.g = ort::IrrGrid{x_edges, y_edges, nx, ny, mode};
  a.x = x;
  a.y = y;
  a.p = power;
  a.n = n;
  a.cmax = (unsigned long long*)workspace;
  a.acc = (unsigned long long*)((char*)workspace + kIrrHeader);
  a.flags = (uint32_t*)(a.acc + npix);
  a.out = out;
  a.area = pixel_area;
  a.log2_n = ort::irr_log2_ceil(n);
  if (hipMemsetAsync(workspace, 0, (size_t)need, s) != hipSuccess) return ORT_ERR_LAUNCH;
  if (n > 0) {
    const bool tile = npix <= ORT_IRRADIANCE_TILE_PIXELS;
    const size_t lds = tile ? (size_t)npix * sizeof(unsigned long long) : 0;
    // workgroups: at most what the CUs hold at once (a tile above half the LDS: one per CU),
    // so a workgroup's tile flush is paid once per CU and not once per 1,024 rays
    const int64_t cap = tile && lds > 80 * 1024 ? 256 : 512;
    const int64_t want = (n + kIrrThreads - 1) / kIrrThreads;
    const int64_t blocks = want < cap ? want : cap;
    a.rounds = (want + blocks - 1) / blocks;
    hipLaunchKernelGGL(irr_cmax_kernel, dim3((unsigned)blocks), dim3(kIrrThreads), 0, s, a);
    if (tile) {
      if (lds > 64 * 1024 &&
          hipFuncSetAttribute((const void*)irr_bin_kernel<true>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              ORT_IRRADIANCE_TILE_PIXELS * (int)sizeof(unsigned long long)) !=
              hipSuccess)
        return ORT_ERR_LAUNCH;
      hipLaunchKernelGGL(irr_bin_kernel<true>, dim3((unsigned)blocks), dim3(kIrrThreads), lds, s,
                         a);
    } else {
      hipLaunchKernelGGL(irr_bin_kernel<false>, dim3((unsigned)blocks), dim3(kIrrThreads), 0, s,
                         a);
    }
  }
  hipLaunchKernelGGL(irr_finish_kernel,
                     dim3((unsigned)((npix + kIrrSmallThreads - 1) / kIrrSmallThreads)),
                     dim3(kIrrSmallThreads), 0, s, a);
  return hipGetLastError() == hipSuccess ? ORT_OK : ORT_ERR_LAUNCH;
}

int ort_irradiance_bin_vjp(const double* x, const double* y, const double* power, int64_t n,
                           const double* x_edges, int64_t nx, const double* y_edges, int64_t ny,
                           double pixel_area, const double* grad_out, double* grad_x,
                           double* grad_y, double* grad_power, void* stream) {
  if (n < 0 || !irr_grid_ok(nx, ny, ORT_BIN_BILINEAR) || !x_edges || !y_edges || !grad_out)
    return ORT_ERR_ARG;
  if (n == 0) return ORT_OK;
  if (!x || !y || !power || !grad_x || !grad_y || !grad_power) return ORT_ERR_ARG;
  const int64_t blocks = (n + kIrrSmallThreads - 1) / kIrrSmallThreads;
  if (blocks > 0x7fffffff) return ORT_ERR_ARG;
  IrrVjpArgs a{};
  a.g = ort::IrrGrid{x_edges, y_edges, nx, ny, ORT_BIN_BILINEAR};
  a.x = x;
  a.y = y;
  a.p = power;
  a.n = n;
  a.grad = grad_out;
  a.area = pixel_area;
  a.gx = grad_x;
  a.gy = grad_y;
  a.gp = grad_power;
  hipLaunchKernelGGL(irr_vjp_kernel, dim3((unsigned)blocks), dim3(kIrrSmallThreads), 0,
                     (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? ORT_OK : ORT_ERR_LAUNCH;
}

}  // extern "C"
