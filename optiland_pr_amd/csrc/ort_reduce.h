// ort_reduce.h -- every cross-lane and cross-wave step of the kernels, and the one rule of
// the deterministic sums: lanes by wave_sum, then the block's waves added in index order
// onto 0.0, so a reduction over fixed chunks is bit-identical run to run. A leaf header: the
// HIP runtime and nothing of this project.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ortk {

constexpr int kRedThreads = 256;  // threads per block of the analysis kernels

// Sum over the 64 lanes of a wave. With the whole wave active: DPP row operations
// (VALU moves, no LDS round trip per step): quad_perm xor 1 and xor 2, row_half_mirror,
// row_mirror (a row of 16 summed in every lane), row_bcast15 / row_bcast31 (rows
// accumulated into lane 63), then lane 63 read into a scalar. Otherwise the xor
// butterfly through ds_bpermute. Either way a fixed order: deterministic run to run.
template <int CTRL, int ROW_MASK>
__device__ inline double dpp_step(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, ROW_MASK, 0xf,
                                             false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}
__device__ inline double wave_sum(double v) {
  if (__builtin_amdgcn_read_exec() == ~0ull) {
    v += dpp_step<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
    v += dpp_step<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
    v += dpp_step<0x141, 0xf>(v);  // row_half_mirror
    v += dpp_step<0x140, 0xf>(v);  // row_mirror
    v += dpp_step<0x142, 0xa>(v);  // row_bcast15 -> rows 1, 3
    v += dpp_step<0x143, 0xc>(v);  // row_bcast31 -> rows 2, 3
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), 63);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
  }
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// every lane gets the sum of its group of eight lanes (wave_sum's first three steps)
__device__ inline double group8_sum(double v) {
  if (__builtin_amdgcn_read_exec() == ~0ull) {
    v += dpp_step<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
    v += dpp_step<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
    v += dpp_step<0x141, 0xf>(v);  // row_half_mirror: lane i <- lane 7 - i of its 8
    return v;
  }
  for (int o = 1; o < 8; o <<= 1) v += __shfl_xor(v, o, 64);  // the same sums, same order
  return v;
}
__device__ inline double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = ::fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ inline int wave_max_i32(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ inline uint64_t wave_and_u64(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) v &= __shfl_xor(v, o, 64);
  return v;
}

// The lead form of the block sum, for a kernel whose totals only one thread (or one per
// column) needs: the wave sums of NV values, stored by lane 0 of each wave to [wave * NV + k]
// of the form's own LDS, then one barrier; block_sum_at on the returned rows then gives a
// thread column k's total. One call per kernel (the rows are not guarded for reuse).
template <int NV, int NT = kRedThreads>
__device__ inline const double* block_sum_lead(double (&v)[NV]) {
  __shared__ double lds[NT / 64 * NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    v[k] = wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0) lds[(threadIdx.x >> 6) * NV + k] = v[k];
  }
  __syncthreads();
  return lds;
}
// waves 0 .. NT / 64 - 1 of column k in index order onto 0.0 (so a -0.0 total comes out +0.0)
template <int NV, int NT = kRedThreads>
__device__ inline double block_sum_at(const double* lds, int k) {
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) s += lds[w * NV + k];
  return s;
}

// block-wide sums of NV values (lanes by wave_sum, then waves 0..NT/64-1 in order);
// every thread gets the totals. lds: >= NT / 64 * NV doubles; safe to call back to back.
template <int NV, int NT = kRedThreads>
__device__ inline void block_sum(double (&v)[NV], double* lds) {
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) lds[w * NV + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = block_sum_at<NV, NT>(lds, k);
}

// column sums of rows part[0 .. n) of NV doubles, each thread striding over rows in
// index order, then block_sum
template <int NV>
__device__ inline void reduce_rows_n(const double* part, int n, double (&v)[NV], double* lds) {
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = 0.0;
  for (int c = threadIdx.x; c < n; c += kRedThreads)
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += part[c * NV + k];
  block_sum<NV>(v, lds);
}

// The rms spot size from the F_RMS rows (ort_rms_finish, and the second workgroup of
// ort_newton_finish_rms): one workgroup of NT threads, each holding up to ROWS rows in
// registers (rows past NT * ROWS re-read in the second sum). The counts and sums in index
// order give the centroid (mx, my); then M2 = sum over rows of [M2_b + n_b ((sx_b / n_b -
// mx)^2 + (sy_b / n_b - my)^2)] (a row with n_b = 0 adds nothing: Chan et al.'s pairwise
// update), rms = sqrt(M2 / n); stats as ort_rms_spot's row (n, mean x, mean y, rms) with the
// geometric radius, which this pass has no data for, NaN. lds: >= NT / 64 * 3 doubles.
__device__ inline double rms_row_m2(const double* p, double mx, double my) {
  const double nb = p[0];
  if (!(nb > 0.0)) return 0.0;
  const double dx = p[1] / nb - mx, dy = p[2] / nb - my;
  return p[3] + nb * (dx * dx + dy * dy);
}

constexpr int kRmsFinThreads = 256;  // the one workgroup shape of both finish launches
constexpr int kRmsFinRows = 16;

template <int NT, int ROWS>
__device__ inline void rms_finish_block(const double* part, int n_rows, double* stats,
                                        double* rms, double* lds) {
  double row[ROWS][4];
#pragma unroll
  for (int k = 0; k < ROWS; ++k) {
    const int c = threadIdx.x + k * NT;
#pragma unroll
    for (int f = 0; f < 4; ++f) row[k][f] = c < n_rows ? part[(int64_t)c * 4 + f] : 0.0;
  }
  double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < ROWS; ++k) {
    v[0] += row[k][0];
    v[1] += row[k][1];
    v[2] += row[k][2];
  }
  for (int c = threadIdx.x + ROWS * NT; c < n_rows; c += NT) {
    v[0] += part[(int64_t)c * 4 + 0];
    v[1] += part[(int64_t)c * 4 + 1];
    v[2] += part[(int64_t)c * 4 + 2];
  }
  block_sum<3, NT>(v, lds);
  const double mx = v[1] / v[0], my = v[2] / v[0];
  double m[1] = {0.0};
#pragma unroll
  for (int k = 0; k < ROWS; ++k) m[0] += rms_row_m2(row[k], mx, my);
  for (int c = threadIdx.x + ROWS * NT; c < n_rows; c += NT)
    m[0] += rms_row_m2(part + (int64_t)c * 4, mx, my);
  block_sum<1, NT>(m, lds);
  if (threadIdx.x == 0) {
    const double r = ::sqrt(m[0] / v[0]);
    stats[0] = v[0];
    stats[1] = mx;
    stats[2] = my;
    stats[3] = r;
    stats[4] = __builtin_nan("");
    if (rms) *rms = r;
  }
}

}  // namespace ortk
