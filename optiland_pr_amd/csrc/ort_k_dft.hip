// ort_k_dft.hip -- the pupil-to-image DFT of FFTPSF / MMDFTPSF / FFTMTF on the device
// (psf/mmdft.py:164-184 G = L g R, psf/fft.py:169-234; the terms are ort_dft.h).
//
// L = R^T, so there is one twiddle family W(a, b) = exp(-2 pi i a b / pad). Two dependent
// launches, fp64 VALU FMAs, every output summed by one thread from zero in index order:
//
// dft_rows_kernel (stage A, T = g R): a workgroup owns kDftRows rows j x kDftColsA columns u of
//   one pupil's T. Per chunk of ORT_DFT_TILE_K pupil columns k it builds two LDS tiles once --
//   g[k][j] from amp and opd (one sincos per entry; the complex pupil is never in memory) and
//   W[k][u] (one sincos per entry) -- and then lane u of wave w adds g[j,k] W(u,k) for its 8
//   rows j = 8 w .. 8 w + 7: the twiddle is the lane's own LDS word, the pupil value a
//   broadcast read.
// dft_cols_kernel (stage B, out = |R^T T|^2): a workgroup owns kDftStrip rows v x 2 x
//   ORT_DFT_TILE_M columns u (a thread: columns u and u + ORT_DFT_TILE_M). Per chunk of
//   ORT_DFT_TILE_K rows j it builds W[j][v] in LDS (one sincos per thread) and adds
//   W(v,j) T[j,u]: T comes in coalesced 16-byte loads, the twiddle is a broadcast read. A
//   twiddle serves 512 multiply-adds here and 32 in stage A.
//
// No cross-lane or cross-wave sum, no atomics: the bits of an output depend on its pupil, n,
// m and pad only. The batch is the slowest grid index.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ort_args.h"
#include "ort_dft.h"

namespace ortk {
namespace {

constexpr int kDftThreads = 256;
constexpr int kDftK = ORT_DFT_TILE_K;   // sum chunk of both stages
constexpr int kDftRows = ORT_DFT_TILE_K;  // stage A: rows j per workgroup (8 per wave)
constexpr int kDftColsA = 64;           // stage A: columns u per workgroup (one per lane)
constexpr int kDftStrip = 8;            // stage B: rows v per workgroup
constexpr int kDftColsB = ORT_DFT_TILE_M;  // stage B: columns u per thread-column step
static_assert(kDftRows == 8 * (kDftThreads / 64), "stage A: 8 rows per wave");
static_assert(kDftK * kDftStrip == kDftThreads, "stage B: one twiddle per thread and chunk");
static_assert(kDftColsB == kDftThreads, "stage B: one thread per column of a step");

struct DftArgs {
  const double* amp;  // [batch][n][n]
  const double* opd;  // [batch][n][n]
  double* t;          // [batch][n][m][2]
  double* out;        // [batch][m][m]
  int64_t n, m;
  double pad;
  int64_t ipad;       // ort::dft_int_pad(pad)
  int32_t tiles_j, tiles_u;  // stage A: tiles per pupil along j and u
  int32_t strips_v, tiles_ub;  // stage B: strips along v, column tiles along u
};

__global__ __launch_bounds__(kDftThreads) void dft_rows_kernel(const DftArgs a) {
  __shared__ double2 gs[kDftK][kDftRows];   // g[k][j]
  __shared__ double2 ws[kDftK][kDftColsA];  // W(u, k)
  const int tx = threadIdx.x, lane = tx & 63, wave = tx >> 6;
  int64_t b = blockIdx.x;
  const int64_t tu = b % a.tiles_u;
  b /= a.tiles_u;
  const int64_t tj = b % a.tiles_j;
  const int64_t batch = b / a.tiles_j;
  const int64_t j0 = tj * kDftRows, u0 = tu * kDftColsA;
  const int64_t hn = a.n / 2, hm = a.m / 2;
  const double* amp = a.amp + batch * a.n * a.n;
  const double* opd = a.opd + batch * a.n * a.n;
  double sr[8], si[8];
  for (int r = 0; r < 8; ++r) sr[r] = si[r] = 0.0;
  for (int64_t k0 = 0; k0 < a.n; k0 += kDftK) {
    const int kc = a.n - k0 < kDftK ? (int)(a.n - k0) : kDftK;
    for (int e = tx; e < kDftK * kDftRows; e += kDftThreads) {
      const int kk = e % kDftK, jj = e / kDftK;
      double2 g = {0.0, 0.0};
      if (kk < kc && j0 + jj < a.n) {
        const int64_t at = (j0 + jj) * a.n + k0 + kk;
        ort::dft_pupil(amp[at], opd[at], g.x, g.y);
      }
      gs[kk][jj] = g;
    }
    for (int e = tx; e < kDftK * kDftColsA; e += kDftThreads) {
      const int kk = e / kDftColsA, uu = e % kDftColsA;
      double2 w = {0.0, 0.0};
      if (kk < kc && u0 + uu < a.m)
        ort::dft_twiddle(u0 + uu - hm, k0 + kk - hn, a.pad, a.ipad, w.x, w.y);
      ws[kk][uu] = w;
    }
    __syncthreads();
    for (int kk = 0; kk < kc; ++kk) {
      const double2 w = ws[kk][lane];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const double2 g = gs[kk][wave * 8 + r];
        ort::dft_mac(g.x, g.y, w.x, w.y, sr[r], si[r]);
      }
    }
    __syncthreads();
  }
  const int64_t u = u0 + lane;
  if (u >= a.m) return;
  for (int r = 0; r < 8; ++r) {
    const int64_t j = j0 + wave * 8 + r;
    if (j < a.n) {
      double2* o = (double2*)a.t + (batch * a.n + j) * a.m + u;
      *o = double2{sr[r], si[r]};
    }
  }
}

__global__ __launch_bounds__(kDftThreads) void dft_cols_kernel(const DftArgs a) {
  __shared__ double2 ws[kDftK][kDftStrip];  // W(v, j)
  const int tx = threadIdx.x;
  int64_t b = blockIdx.x;
  const int64_t tu = b % a.tiles_ub;
  b /= a.tiles_ub;
  const int64_t sv = b % a.strips_v;
  const int64_t batch = b / a.strips_v;
  const int64_t v0 = sv * kDftStrip, u0 = tu * (2 * kDftColsB);
  const int64_t hn = a.n / 2, hm = a.m / 2;
  const int64_t ua = u0 + tx, ub = ua + kDftColsB;
  const bool ina = ua < a.m, inb = ub < a.m;
  const bool two = u0 + kDftColsB < a.m;  // the workgroup has a second column step
  const double2* t = (const double2*)a.t + batch * a.n * a.m;
  double ar[kDftStrip], ai[kDftStrip], br[kDftStrip], bi[kDftStrip];
  for (int r = 0; r < kDftStrip; ++r) ar[r] = ai[r] = br[r] = bi[r] = 0.0;
  for (int64_t j0 = 0; j0 < a.n; j0 += kDftK) {
    const int jc = a.n - j0 < kDftK ? (int)(a.n - j0) : kDftK;
    {
      const int jj = tx / kDftStrip, vv = tx % kDftStrip;
      double2 w = {0.0, 0.0};
      if (jj < jc && v0 + vv < a.m)
        ort::dft_twiddle(v0 + vv - hm, j0 + jj - hn, a.pad, a.ipad, w.x, w.y);
      ws[jj][vv] = w;
    }
    __syncthreads();
    for (int jj = 0; jj < jc; ++jj) {
      const double2* row = t + (j0 + jj) * a.m;
      const double2 zero = {0.0, 0.0};
      const double2 ta = ina ? row[ua] : zero;
      const double2 tb = inb ? row[ub] : zero;
#pragma unroll
      for (int r = 0; r < kDftStrip; ++r) {
        const double2 w = ws[jj][r];
        ort::dft_mac(w.x, w.y, ta.x, ta.y, ar[r], ai[r]);
        if (two) ort::dft_mac(w.x, w.y, tb.x, tb.y, br[r], bi[r]);
      }
    }
    __syncthreads();
  }
  for (int r = 0; r < kDftStrip; ++r) {
    const int64_t v = v0 + r;
    if (v >= a.m) break;
    double* o = a.out + (batch * a.m + v) * a.m;
    if (ina) o[ua] = ar[r] * ar[r] + ai[r] * ai[r];
    if (inb) o[ub] = br[r] * br[r] + bi[r] * bi[r];
  }
}

int64_t ceil_div(int64_t x, int64_t y) { return (x + y - 1) / y; }

}  // namespace
}  // namespace ortk

using namespace ortk;

extern "C" {

int64_t ort_dft_workspace_size(int64_t batch, int64_t n, int64_t m) {
  if (dft_check(nullptr, nullptr, 0, n, m, 1.0, nullptr) != ORT_OK || batch < 0 ||
      batch > INT64_MAX / 16 / ORT_DFT_MAX_SIZE / ORT_DFT_MAX_SIZE)
    return ORT_ERR_ARG;
  return batch * n * m * 2 * (int64_t)sizeof(double);
}

int ort_dft_psf(const double* amp, const double* opd_waves, int64_t batch, int64_t n, int64_t m,
                double pad, double* out, void* workspace, int64_t workspace_size, void* stream) {
  const int rc = dft_check(amp, opd_waves, batch, n, m, pad, out);
  if (rc != ORT_OK) return rc;
  const int64_t need = ort_dft_workspace_size(batch, n, m);
  if (need < 0 || workspace_size < need || (need > 0 && !workspace)) return ORT_ERR_ARG;
  if (batch == 0 || m == 0) return ORT_OK;
  DftArgs a{};
  a.amp = amp;
  a.opd = opd_waves;
  a.t = (double*)workspace;
  a.out = out;
  a.n = n;
  a.m = m;
  a.pad = pad;
  a.ipad = ort::dft_int_pad(pad);
  a.tiles_j = (int32_t)ceil_div(n, kDftRows);
  a.tiles_u = (int32_t)ceil_div(m, kDftColsA);
  a.strips_v = (int32_t)ceil_div(m, kDftStrip);
  a.tiles_ub = (int32_t)ceil_div(m, 2 * kDftColsB);
  const int64_t grid_a = batch * a.tiles_j * a.tiles_u;
  const int64_t grid_b = batch * a.strips_v * a.tiles_ub;
  if (grid_a > 0x7fffffff || grid_b > 0x7fffffff) return ORT_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dft_rows_kernel, dim3((unsigned)grid_a), dim3(kDftThreads), 0, s, a);
  hipLaunchKernelGGL(dft_cols_kernel, dim3((unsigned)grid_b), dim3(kDftThreads), 0, s, a);
  return hipGetLastError() == hipSuccess ? ORT_OK : ORT_ERR_LAUNCH;
}

}  // extern "C"
