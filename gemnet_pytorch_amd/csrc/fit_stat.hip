// The statistic of the scale-factor fit (include/gemnet_hip.h, gn_col_var_f32).
//
// Reference (gemnet/model/layers/scaling.py:143-147): AutoScaleFit.observe adds rows * mean_c Var_c(x) of the reference
// input and of the scaled output of a layer, where the reference input of the two bilinear sums is the GATHERED array
// x[id_expand] ((T,C) triplet rows / (Q,C) quadruplet rows: tens of millions of rows of a periodic GemNet-Q batch, formed only
// to be looked at).  Here the rows are read through the index and never written:
//   acc[slot] += w * 1/C sum_c Var_c,   Var_c = unbiased variance over q < n of x[idx ? idx[q] : q, c]
// in ONE pass over memory and float64 throughout:
//   * shifted sums: the shift s_c is the first row itself (x[idx[0], c]), d = (double)x - s_c is exact, and
//     Var_c = (sum d^2 - (sum d)^2 / n) / (n - 1).  The shift lies inside the column's own spread, so the subtraction cancels
//     at most the few digits of (mean - s)^2 / Var, whatever the ratio of the mean to the spread; equal rows give d = 0 and an
//     exact zero.
//   * layout: C / 4 lanes per row (one float4 each: a row is one contiguous 4 C-byte read, 256 / (C/4) rows per block and
//     trip, four trips in flight per thread), every thread keeps sum d and sum d^2 of its four columns in registers.
//   * no atomics: a FIXED grid (a function of n and C only) of blocks over contiguous row ranges; the threads of a block
//     meet in LDS and are added in row-slot order; block b writes its 2 C partial sums to ws[b]; a second, one-block launch
//     adds the partials in block order, forms the variances and updates the accumulator slot.  Two calls on the same input give
//     the same bits.
// Nothing is read back: the accumulator lives on the device until AutoScaleFit.fit() reads it.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int UNROLL = 4;

__device__ __forceinline__ void add_row(const float4 v, const double s0, const double s1, const double s2, const double s3,
                                        double (&a)[8]) {
  const double d0 = (double)v.x - s0, d1 = (double)v.y - s1, d2 = (double)v.z - s2, d3 = (double)v.w - s3;
  a[0] += d0;
  a[1] += d1;
  a[2] += d2;
  a[3] += d3;
  a[4] = fma(d0, d0, a[4]);
  a[5] = fma(d1, d1, a[5]);
  a[6] = fma(d2, d2, a[6]);
  a[7] = fma(d3, d3, a[7]);
}

// L = C / 4 lanes per row; block b owns rows [b * chunk, min(n, (b + 1) * chunk)).  ws (gridDim.x, 2, C) doubles.
__global__ __launch_bounds__(THREADS) void col_var_partial_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx,
                                                                  double* __restrict__ ws, const int64_t n_src, const int64_t n,
                                                                  const int64_t chunk, const int L) {
  __shared__ double red[THREADS * 8];
  const int C = 4 * L;
  const int rows_per_trip = THREADS / L;
  const int slot = threadIdx.x / L, lane = threadIdx.x % L;
  const int64_t first = idx ? (int64_t)idx[0] : 0;
  const bool first_ok = first >= 0 && first < n_src;
  const float4 s = first_ok ? *reinterpret_cast<const float4*>(x + first * C + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
  const double s0 = s.x, s1 = s.y, s2 = s.z, s3 = s.w;
  double a[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
  const int64_t beg = (int64_t)blockIdx.x * chunk;
  const int64_t end = beg + chunk < n ? beg + chunk : n;
  int64_t q = beg + slot;
  // (an index outside [0, n_src) reads nothing and counts as a copy of the first row: d = 0)
  for (; q + (int64_t)(UNROLL - 1) * rows_per_trip < end; q += (int64_t)UNROLL * rows_per_trip) {
    int64_t r[UNROLL];
    float4 v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) r[u] = idx ? (int64_t)idx[q + (int64_t)u * rows_per_trip] : q + (int64_t)u * rows_per_trip;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
      v[u] = (r[u] >= 0 && r[u] < n_src) ? *reinterpret_cast<const float4*>(x + r[u] * C + 4 * lane) : s;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) add_row(v[u], s0, s1, s2, s3, a);
  }
  for (; q < end; q += rows_per_trip) {
    const int64_t r = idx ? (int64_t)idx[q] : q;
    const float4 v = (r >= 0 && r < n_src) ? *reinterpret_cast<const float4*>(x + r * C + 4 * lane) : s;
    add_row(v, s0, s1, s2, s3, a);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) red[k * THREADS + threadIdx.x] = a[k];
  __syncthreads();
  // the L threads of row slot 0 add the slots in order (a fixed order: the result does not depend on the schedule)
  if (slot == 0) {
    const int slots = THREADS / L;
    for (int k = 0; k < 8; ++k) {
      double t = red[k * THREADS + lane];
      for (int j = 1; j < slots; ++j) t += red[k * THREADS + j * L + lane];
      // k < 4: sum d of column 4 lane + k; k >= 4: sum d^2 of column 4 lane + k - 4
      ws[(int64_t)blockIdx.x * 2 * C + (k < 4 ? 0 : C) + 4 * lane + (k & 3)] = t;
    }
  }
}

// One block: thread t < 2 C * K adds the partials j = t % (2 C) of the blocks b = k, k + K, ... (k = t / (2 C)), the K sub-sums
// meet in LDS in order; then the variances, their mean and the accumulator.
__global__ __launch_bounds__(THREADS) void col_var_final_kernel(const double* __restrict__ ws, double* __restrict__ acc,
                                                                const int blocks, const int64_t n, const int C, const int slot,
                                                                const double w) {
  __shared__ double part[THREADS];
  __shared__ double var[128];
  const int W = 2 * C;
  const int K = THREADS / W;
  const int j = threadIdx.x % W, k = threadIdx.x / W;
  double t = 0.;
  if (k < K)
    for (int b = k; b < blocks; b += K) t += ws[(int64_t)b * W + j];
  part[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x < W) {
    double sum = part[threadIdx.x];
    for (int kk = 1; kk < K; ++kk) sum += part[kk * W + threadIdx.x];
    part[threadIdx.x] = sum;
  }
  __syncthreads();
  if (threadIdx.x < C) {
    const double s1 = part[threadIdx.x], s2 = part[C + threadIdx.x];
    const double v = (s2 - s1 * s1 / (double)n) / (double)(n - 1);
    var[threadIdx.x] = v > 0. ? v : 0.;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = 0.;
    for (int c = 0; c < C; ++c) sum += var[c];
    acc[slot] += w * (sum / (double)C);
  }
}

}  // namespace

extern "C" int gn_col_var_f32(const float* x, const int32_t* idx, double* ws, double* acc, int64_t n_src, int64_t n, int C,
                              int slot, double w, void* stream) {
  if (!(C == 8 || C == 16 || C == 32 || C == 64 || C == 128) || n < 2 || n_src < 1 || slot < 0 ||
      n_src >= ((int64_t)1 << 31) || (!idx && n > n_src) || (reinterpret_cast<uintptr_t>(x) & 15) != 0)
    return (int)hipErrorInvalidValue;
  const int L = C / 4;
  const int64_t rows_per_trip = THREADS / L;
  // a fixed grid: a function of n and C only (at least 2 * UNROLL trips per block while there are rows for it)
  int64_t blocks = (n + rows_per_trip * 2 * UNROLL - 1) / (rows_per_trip * 2 * UNROLL);
  if (blocks > GN_COL_VAR_MAX_BLOCKS) blocks = GN_COL_VAR_MAX_BLOCKS;
  const int64_t chunk = (n + blocks - 1) / blocks;
  blocks = (n + chunk - 1) / chunk;          // no block without rows
  hipLaunchKernelGGL(col_var_partial_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, static_cast<hipStream_t>(stream), x, idx,
                     ws, n_src, n, chunk, L);
  GN_LAUNCH_CHECK();
  hipLaunchKernelGGL(col_var_final_kernel, dim3(1), dim3(THREADS), 0, static_cast<hipStream_t>(stream), ws, acc, (int)blocks, n,
                     C, slot, w);
  GN_LAUNCH_CHECK();
  return 0;
}
