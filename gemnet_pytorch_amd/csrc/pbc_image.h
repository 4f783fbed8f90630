// Image search shared by the periodic index builds (pbc.hip: edges within the cutoff; pbc_index_q.hip: interaction edges
// within int_cutoff): the image range of a pair, the distance test rounded in the positions' dtype, the single-block scan
// that sizes every ragged output, and the lookup of the forward edges of a pair.  Conventions in include/gemnet_hip.h.
#pragma once
#include "common.h"

namespace {

template <typename T> struct RNp;
template <> struct RNp<float> {
  static __device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
  static __device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
  static __device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }
  static __device__ __forceinline__ float sqrt(float a) { return __fsqrt_rn(a); }
};
template <> struct RNp<double> {
  static __device__ __forceinline__ double mul(double a, double b) { return __dmul_rn(a, b); }
  static __device__ __forceinline__ double add(double a, double b) { return __dadd_rn(a, b); }
  static __device__ __forceinline__ double sub(double a, double b) { return __dsub_rn(a, b); }
  static __device__ __forceinline__ double sqrt(double a) { return __dsqrt_rn(a); }
};

struct Range { int lo[3], hi[3]; };

// image range of the pair (i, j) of structure m
template <typename T>
__device__ Range image_range(const T* __restrict__ R, const T* __restrict__ cell, const uint8_t* __restrict__ pbc, int m, int i,
                             int j, double cutoff) {
  const T* C = cell + 9 * (int64_t)m;
  double c[3][3];
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) c[r][k] = (double)C[3 * r + k];
  // cofactors: row k of cof = a_l x a_m (l, m the other two lattice vectors)
  double cof[3][3];
  for (int k = 0; k < 3; ++k) {
    const int l = (k + 1) % 3, n = (k + 2) % 3;
    cof[k][0] = c[l][1] * c[n][2] - c[l][2] * c[n][1];
    cof[k][1] = c[l][2] * c[n][0] - c[l][0] * c[n][2];
    cof[k][2] = c[l][0] * c[n][1] - c[l][1] * c[n][0];
  }
  const double det = c[0][0] * cof[0][0] + c[0][1] * cof[0][1] + c[0][2] * cof[0][2];
  double d0[3];
  for (int k = 0; k < 3; ++k) d0[k] = (double)R[3 * (int64_t)j + k] - (double)R[3 * (int64_t)i + k];
  Range rg;
  for (int k = 0; k < 3; ++k) {
    rg.lo[k] = rg.hi[k] = 0;
    if (!pbc[3 * m + k]) continue;
    // f_k = d0 . cof[k] / det (inverse of the row-vector cell); h_k = |det| / |cof[k]|
    const double nc = sqrt(cof[k][0] * cof[k][0] + cof[k][1] * cof[k][1] + cof[k][2] * cof[k][2]);
    const double f = (d0[0] * cof[k][0] + d0[1] * cof[k][1] + d0[2] * cof[k][2]) / det;
    const double w = cutoff * nc / fabs(det);
    double lo = floor(-f - w), hi = ceil(-f + w);
    lo = lo < -(double)(1 << 20) ? -(double)(1 << 20) : lo;
    hi = hi > (double)(1 << 20) ? (double)(1 << 20) : hi;
    rg.lo[k] = (int)lo;
    rg.hi[k] = (int)hi;
  }
  return rg;
}

__device__ __forceinline__ bool lex_positive(int n0, int n1, int n2) {
  return n0 > 0 || (n0 == 0 && (n1 > 0 || (n1 == 0 && n2 > 0)));
}

// |R_i - (R_j + n cell)| <= cutoff, rounded in T like the molecular builder (n = 0: exactly its distance)
template <typename T>
__device__ __forceinline__ bool within(const T* __restrict__ R, const T* __restrict__ C, int i, int j, int n0, int n1, int n2,
                                       T cutoff) {
  T d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const T sh = RNp<T>::add(RNp<T>::add(RNp<T>::mul((T)n0, C[k]), RNp<T>::mul((T)n1, C[3 + k])), RNp<T>::mul((T)n2, C[6 + k]));
    d[k] = RNp<T>::sub(R[3 * (int64_t)i + k], RNp<T>::add(R[3 * (int64_t)j + k], sh));
  }
  const T s = RNp<T>::add(RNp<T>::add(RNp<T>::mul(d[0], d[0]), RNp<T>::mul(d[1], d[1])), RNp<T>::mul(d[2], d[2]));
  return RNp<T>::sqrt(s) <= cutoff;
}

// single-block exclusive scan of n int64 (in may alias nothing); out[n] = total
__global__ __launch_bounds__(1024) void pbc_scan_kernel(const int64_t* __restrict__ in, int64_t* __restrict__ out, int64_t n) {
  __shared__ int64_t wsum[16];
  __shared__ int64_t carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int64_t base = 0; base < n; base += 1024) {
    const int64_t i = base + tid;
    const int64_t v = i < n ? in[i] : 0;
    int64_t s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t t = __shfl_up(s, o, 64);
      if (lane >= o) s += t;
    }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    int64_t woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    const int64_t carry = carry_s;
    if (i < n) out[i] = carry + woff + s - v;
    __syncthreads();
    if (tid == 1023) carry_s = carry + woff + s;
    __syncthreads();
  }
  if (tid == 0) out[n] = carry_s;
}

// forward edges of atom i with source atom a: [lo, hi) of id_c inside i's range (sorted by j)
__device__ __forceinline__ void src_range(const int32_t* __restrict__ id_c, int64_t b, int64_t e, int a, int64_t& lo,
                                          int64_t& hi) {
  int64_t l = b, h = e;
  while (l < h) { const int64_t md = (l + h) >> 1; if (id_c[md] < a) l = md + 1; else h = md; }
  lo = l;
  h = e;
  while (l < h) { const int64_t md = (l + h) >> 1; if (id_c[md] <= a) l = md + 1; else h = md; }
  hi = l;
}

// inclusive scan of one int per lane over the wave
__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// interaction edges (a, b, *) inside a's range [lo0, hi0) of int_b (sorted by b)
__device__ __forceinline__ void int_range(const int32_t* __restrict__ int_b, int64_t lo0, int64_t hi0, int b, int64_t& lo,
                                          int64_t& hi) {
  int64_t l = lo0, h = hi0;
  while (l < h) { const int64_t md = (l + h) >> 1; if (int_b[md] < b) l = md + 1; else h = md; }
  lo = l;
  h = hi0;
  while (l < h) { const int64_t md = (l + h) >> 1; if (int_b[md] <= b) l = md + 1; else h = md; }
  hi = l;
}

}  // namespace
