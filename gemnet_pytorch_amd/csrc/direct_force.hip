// The force head of the direct-force GemNet (include/gemnet_hip.h, gn_direct_force_f32).
//
// Reference (gemnet.py:580-596): the per-edge force magnitudes of the K output blocks are summed, with coupled forces
// averaged over the two directions of every undirected edge (scatter-mean over id_undir + gather), multiplied with the unit
// edge vector and scattered onto the target atoms:
//   c[e,t]   = sum_k terms[k,e,t]                              (K - 1 elementwise adds over (E,T))
//   c[e,t]  <- (c[e,t] + c[id_swap[e],t]) / 2                  (segmented sum + scale + gather)
//   F[a,t,:] = sum_{e in seg(a)} c[e,t] V_e / |V_e|            ((E,T,3) product + segmented sum)
// As separate launches that is K + 4 passes over a few kilobytes.  Here it is ONE: a group of 16 lanes (one row of a wave)
// owns one (atom, target) row of F, lane g of the group walks the positions g, g + 16, ... of the atom's CSR segment, forms c
// for its edge from both directions in registers (no (E,T) or (E,T,3) array exists), and the 16 partial sums meet in a fixed
// xor butterfly.
// No atomics, no LDS; every row of F is written exactly once, rows of atoms without in-edges as exact zeros.  The order of
// addition of a row depends on the length and CSR order of that atom's own segment only: the result is bit-reproducible and does
// not change when edges of OTHER atoms are appended (the pad edges of padded.py end in dummy atoms).
// Typical in-degree 10-30: one or two trips per lane; a segment of any length works (the trip count grows).
#include "common.h"

namespace {

constexpr int GROUP = 16;              // lanes per (atom, target) row: one row of a wave
constexpr int THREADS = 256;
constexpr int ROWS_PER_BLOCK = THREADS / GROUP;

__global__ __launch_bounds__(THREADS) void direct_force_kernel(const float* __restrict__ terms, const float* __restrict__ V,
                                                               const int32_t* __restrict__ id_swap,
                                                               const int32_t* __restrict__ perm,
                                                               const int32_t* __restrict__ seg_off, float* __restrict__ F,
                                                               const int64_t n_rows, const int64_t E, const int K, const int T) {
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / GROUP;      // row = a * T + t
  const int g = threadIdx.x % GROUP;
  // (a group past the last row keeps running with an empty segment: every lane of the wave takes part in the shuffles below)
  const bool live = row < n_rows;
  const int64_t a = live ? row / T : 0;
  const int t = live ? (int)(row - a * T) : 0;
  const int beg = live ? seg_off[a] : 0, end = live ? seg_off[a + 1] : 0;
  const int64_t plane = E * T;
  float fx = 0.f, fy = 0.f, fz = 0.f;
  for (int p = beg + g; p < end; p += GROUP) {
    const int64_t e = perm ? perm[p] : p;
    float c = terms[e * T + t];
    for (int k = 1; k < K; ++k) c += terms[k * plane + e * T + t];
    if (id_swap) {
      int64_t s = id_swap[e];
      if (s < 0 || s >= E) s = e;      // (an index outside the list never becomes an address: such an edge is its own partner)
      float cs = terms[s * T + t];
      for (int k = 1; k < K; ++k) cs += terms[k * plane + s * T + t];
      c = 0.5f * (c + cs);
    }
    const float vx = V[3 * e], vy = V[3 * e + 1], vz = V[3 * e + 2];
    const float d = sqrtf(vx * vx + vy * vy + vz * vz);
    fx += c * (vx / d);
    fy += c * (vy / d);
    fz += c * (vz / d);
  }
#pragma unroll
  for (int w = GROUP / 2; w >= 1; w >>= 1) {      // xor butterfly inside the 16-lane row: the same sum in every lane
    fx += __shfl_xor(fx, w, GN_WAVE);
    fy += __shfl_xor(fy, w, GN_WAVE);
    fz += __shfl_xor(fz, w, GN_WAVE);
  }
  if (live && g < 3) F[row * 3 + g] = g == 0 ? fx : (g == 1 ? fy : fz);
}

// The adjoint of the head (gn_direct_force_bwd_f32): d/dterms[k] is the same (E,T) array for every k,
//   h[e,t] = < gF[id_a[e],t,:], V_e / |V_e| >,   g[e,t] = h[e,t]  or, coupled,  (h[e,t] + h[id_swap[e],t]) / 2.
// Gather form: one thread owns one (e,t), reads the cotangent row of the edge's target atom (and of its partner's), and writes
// g[e,t] exactly once.  No atomics, no LDS; an edge's result depends on itself and its partner only, so rows are bit-reproducible
// and unchanged by pad edges appended behind the list.  h is ONE inlined routine with its contraction pinned by explicit fmaf, used
// for the edge and for its partner: the two threads of a pair add the same two numbers, so g[e] == g[id_swap[e]] bit for bit (the
// adjoint's form of "coupled forces sum to zero").  No index becomes an address: a partner outside [0, E) is the edge itself (as in
// the forward; with an involution this is the exact transpose), a target atom outside [0, n_atoms) contributes h = 0.
__device__ __forceinline__ float edge_cotangent(const float* __restrict__ gF, const float* __restrict__ V,
                                                const int32_t* __restrict__ id_a, const int64_t e, const int t, const int T,
                                                const int64_t n_atoms) {
  const int64_t a = id_a[e];
  if (a < 0 || a >= n_atoms) return 0.f;
  const float vx = V[3 * e], vy = V[3 * e + 1], vz = V[3 * e + 2];
  const float d = sqrtf(fmaf(vz, vz, fmaf(vy, vy, vx * vx)));
  const float* __restrict__ row = gF + (a * T + t) * 3;
  return fmaf(row[2], vz / d, fmaf(row[1], vy / d, row[0] * (vx / d)));
}

__global__ __launch_bounds__(THREADS) void direct_force_bwd_kernel(const float* __restrict__ gF, const float* __restrict__ V,
                                                                   const int32_t* __restrict__ id_swap,
                                                                   const int32_t* __restrict__ id_a, float* __restrict__ g,
                                                                   const int64_t n_atoms, const int64_t E, const int T) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;      // i = e * T + t
  if (i >= E * T) return;
  const int64_t e = i / T;
  const int t = (int)(i - e * T);
  float h = edge_cotangent(gF, V, id_a, e, t, T, n_atoms);
  if (id_swap) {
    int64_t s = id_swap[e];
    if (s < 0 || s >= E) s = e;
    h = 0.5f * (h + edge_cotangent(gF, V, id_a, s, t, T, n_atoms));
  }
  g[i] = h;
}

}  // namespace

extern "C" int gn_direct_force_f32(const float* terms, const float* V, const int32_t* id_swap, const int32_t* perm,
                                   const int32_t* seg_off, float* F, int64_t n_atoms, int64_t n_edges, int K, int T,
                                   void* stream) {
  if (K < 1 || K > GN_DIRECT_FORCE_MAX_BLOCKS || T < 1 || T > GN_DIRECT_FORCE_MAX_TARGETS || n_edges < 0 ||
      n_edges >= ((int64_t)1 << 31))
    return (int)hipErrorInvalidValue;
  if (n_atoms <= 0) return 0;
  const int64_t n_rows = n_atoms * T;
  const int64_t blocks = (n_rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  if (blocks >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(direct_force_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, static_cast<hipStream_t>(stream), terms, V,
                     id_swap, perm, seg_off, F, n_rows, n_edges, K, T);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_direct_force_bwd_f32(const float* gF, const float* V, const int32_t* id_swap, const int32_t* id_a, float* g,
                                       int64_t n_atoms, int64_t n_edges, int T, void* stream) {
  if (T < 1 || T > GN_DIRECT_FORCE_MAX_TARGETS || n_edges < 0 || n_edges >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
  if (n_edges == 0) return 0;
  const int64_t blocks = (n_edges * T + THREADS - 1) / THREADS;      // < 2^26
  hipLaunchKernelGGL(direct_force_bwd_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, static_cast<hipStream_t>(stream), gF, V,
                     id_swap, id_a, g, n_atoms, n_edges, T);
  GN_LAUNCH_CHECK();
  return 0;
}
