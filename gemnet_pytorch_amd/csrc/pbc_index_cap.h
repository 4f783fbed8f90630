// Kernels shared by the capacity forms of the periodic index builds (pbc_index.hip: gn_pbc_index_padded_t; pbc_index_qp.hip:
// gn_pbc_qindex_padded): cell check, wave-per-atom pair search, in-edge lists, triplets.  Every kernel reads its counts from
// device memory and compares them with the capacity that bounds its arrays before it indexes with them.
#pragma once
#include "common.h"
#include "pbc_image.h"

namespace {

constexpr int kMaxImages = 64;        // pbc.MAX_IMAGES: images per axis and side
constexpr int kGeo = 16;              // doubles per structure: cof[9], det, w[3]


// |R_i - (R_j + n cell)| <= cutoff with every operation rounded in float32: `within<float>` of pbc.hip on registers
__device__ __forceinline__ bool within_f32(const float* ri, const float* rj, const float* C, int n0, int n1, int n2, float cutoff) {
  float d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float sh = __fadd_rn(__fadd_rn(__fmul_rn((float)n0, C[k]), __fmul_rn((float)n1, C[3 + k])), __fmul_rn((float)n2, C[6 + k]));
    d[k] = __fsub_rn(ri[k], __fadd_rn(rj[k], sh));
  }
  const float s = __fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2]));
  return __fsqrt_rn(s) <= cutoff;
}

// one wave: per structure the cofactors / determinant / cutoff over height of image_range (pbc.hip), and the checks of
// PeriodicGraphBuilder.check_cell: 64 non-finite or |det| < 1e-12, 32 more than kMaxImages images per side on a periodic axis
__global__ __launch_bounds__(64) void pbx_cell_kernel(const float* __restrict__ cell, const uint8_t* __restrict__ pbc, int B,
                                                      double cutoff, double* __restrict__ geo, int32_t* __restrict__ cellerr) {
  int err = 0;
  for (int b = threadIdx.x; b < B; b += 64) {
    const float* C = cell + 9 * (int64_t)b;
    double c[3][3];
    bool finite = true;
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k) {
        c[r][k] = (double)C[3 * r + k];
        finite = finite && isfinite(c[r][k]);
      }
    double cof[3][3];
    for (int k = 0; k < 3; ++k) {
      const int l = (k + 1) % 3, n = (k + 2) % 3;
      cof[k][0] = c[l][1] * c[n][2] - c[l][2] * c[n][1];
      cof[k][1] = c[l][2] * c[n][0] - c[l][0] * c[n][2];
      cof[k][2] = c[l][0] * c[n][1] - c[l][1] * c[n][0];
    }
    const double det = c[0][0] * cof[0][0] + c[0][1] * cof[0][1] + c[0][2] * cof[0][2];
    double* g = geo + kGeo * (int64_t)b;
    for (int k = 0; k < 3; ++k)
      for (int q = 0; q < 3; ++q) g[3 * k + q] = cof[k][q];
    g[9] = det;
    if (!finite || !isfinite(det) || fabs(det) < 1e-12) {
      err |= 64;
      g[10] = g[11] = g[12] = 0.0;
      continue;
    }
    for (int k = 0; k < 3; ++k) {
      const double nc = sqrt(cof[k][0] * cof[k][0] + cof[k][1] * cof[k][1] + cof[k][2] * cof[k][2]);
      const double w = cutoff * nc / fabs(det);
      g[10 + k] = w;
      if (pbc[3 * b + k] && !(ceil(w) <= (double)kMaxImages)) err |= 32;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) err |= __shfl_xor(err, o, 64);
  if (threadIdx.x == 0) cellerr[0] = err;
}

// one wave per atom i: its canonical forward pairs (i, j >= i, n); count (kFill == false) or fill into the staging arrays
template <bool kFill>
__global__ __launch_bounds__(256) void pbx_pairs_kernel(const float* __restrict__ R, const float* __restrict__ cell,
                                                        const uint8_t* __restrict__ pbc, const int32_t* __restrict__ mol_off,
                                                        const int32_t* __restrict__ atom_mol, int A, float cutoff,
                                                        const double* __restrict__ geo, const int32_t* __restrict__ cellerr,
                                                        int64_t* __restrict__ cnt, const int64_t* __restrict__ off, int e_cap,
                                                        int32_t* __restrict__ s_a, int32_t* __restrict__ s_c,
                                                        int32_t* __restrict__ s_undir, int32_t* __restrict__ s_swap,
                                                        int32_t* __restrict__ s_offs, int m_fill) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= A) return;                                         // (wave-uniform: i is the wave's atom)
  // m_fill: the structure of the filler atoms of an atom capacity (gn_pbc_index_padded_tv; -1: none) — they have no pair,
  // wherever they sit and whatever the cutoff (wave-uniform: the structure is the wave's atom's)
  if (cellerr[0] || atom_mol[i] == m_fill) {
    if (!kFill && lane == 0) cnt[i] = 0;
    return;
  }
  int64_t H = 0;
  if (kFill) {
    H = off[A];
    if (2 * H > (int64_t)e_cap) return;                       // does not fit: nothing is written, `decide` reports it
  }
  const int m = atom_mol[i];
  const int a1 = mol_off[m + 1];
  float C[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) C[k] = cell[9 * (int64_t)m + k];
  const double* g = geo + kGeo * (int64_t)m;
  const double det = g[9];
  const float ri[3] = {R[3 * (int64_t)i], R[3 * (int64_t)i + 1], R[3 * (int64_t)i + 2]};
  int64_t run = kFill ? off[i] : 0;
  for (int j0 = i; j0 < a1; j0 += 64) {
    const int j = j0 + lane;
    int lo[3] = {0, 0, 0}, wd[3] = {0, 0, 0};
    float rj[3] = {0.f, 0.f, 0.f};
    int c = 0;
    uint64_t hits = 0;
    bool masked = false;
    if (j < a1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) rj[k] = R[3 * (int64_t)j + k];
      const double d0[3] = {(double)rj[0] - (double)ri[0], (double)rj[1] - (double)ri[1], (double)rj[2] - (double)ri[2]};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        wd[k] = 1;
        if (!pbc[3 * m + k]) continue;
        // image_range of pbc.hip: f_k = d0 . cof[k] / det, n_k in [floor(-f_k - w_k), ceil(-f_k + w_k)]
        const double f = (d0[0] * g[3 * k] + d0[1] * g[3 * k + 1] + d0[2] * g[3 * k + 2]) / det;
        const double l = floor(-f - g[10 + k]), h = ceil(-f + g[10 + k]);
        // a valid cell has w_k <= kMaxImages: anything wider (or NaN) comes from non-finite positions -> no images
        if (!(h - l <= (double)(2 * kMaxImages + 2)) || !(fabs(l) <= (double)(1 << 20))) { wd[k] = 0; continue; }
        lo[k] = (int)l;
        wd[k] = (int)h - (int)l + 1;
      }
      const int nimg = wd[0] * wd[1] * wd[2];
      masked = nimg <= 64;
      int q = 0;
      for (int n0 = lo[0]; n0 < lo[0] + wd[0]; ++n0)
        for (int n1 = lo[1]; n1 < lo[1] + wd[1]; ++n1)
          for (int n2 = lo[2]; n2 < lo[2] + wd[2]; ++n2, ++q) {
            if (j == i && !lex_positive(n0, n1, n2)) continue;
            if (!within_f32(ri, rj, C, n0, n1, n2, cutoff)) continue;
            if (masked) hits |= 1ull << q;
            ++c;
          }
    }
    const int incl = wave_scan_incl(c, lane);
    const int total = __shfl(incl, 63, 64);
    if (kFill && c > 0) {
      int64_t e = run + (incl - c);
      auto put = [&](int n0, int n1, int n2) {
        if (e >= H) return;                                   // (cannot happen: the count pass saw the same numbers)
        const int64_t s = e + H;
        s_a[e] = i; s_c[e] = j;
        s_a[s] = j; s_c[s] = i;
        s_undir[e] = (int32_t)e; s_undir[s] = (int32_t)e;
        s_swap[e] = (int32_t)s; s_swap[s] = (int32_t)e;
        s_offs[3 * e] = n0; s_offs[3 * e + 1] = n1; s_offs[3 * e + 2] = n2;
        s_offs[3 * s] = -n0; s_offs[3 * s + 1] = -n1; s_offs[3 * s + 2] = -n2;
        ++e;
      };
      if (masked) {
        const int w12 = wd[1] * wd[2];
        while (hits) {
          const int q = __builtin_ctzll(hits);
          hits &= hits - 1;
          const int n0 = q / w12, rem = q - n0 * w12, n1 = rem / wd[2];
          put(lo[0] + n0, lo[1] + n1, lo[2] + rem - n1 * wd[2]);
        }
      } else {
        for (int n0 = lo[0]; n0 < lo[0] + wd[0]; ++n0)
          for (int n1 = lo[1]; n1 < lo[1] + wd[1]; ++n1)
            for (int n2 = lo[2]; n2 < lo[2] + wd[2]; ++n2) {
              if (j == i && !lex_positive(n0, n1, n2)) continue;
              if (within_f32(ri, rj, C, n0, n1, n2, cutoff)) put(n0, n1, n2);
            }
      }
    }
    run += total;
  }
  if (!kFill && lane == 0) cnt[i] = run;
}


// one wave per atom a: its in-degree (kList == false) or its incoming edges in ascending id — the forward edges of a, then the
// swapped twins of the forward edges (i, a, n), i <= a, lanes over i and a wave scan keeping ascending i (= ascending id)
template <bool kList>
__global__ __launch_bounds__(256) void pbx_in_kernel(const int32_t* __restrict__ mol_off, const int32_t* __restrict__ atom_mol,
                                                     int A, const int64_t* __restrict__ off, const int32_t* __restrict__ s_c,
                                                     int e_cap, const int32_t* __restrict__ cellerr, int64_t* __restrict__ deg,
                                                     const int64_t* __restrict__ in_ptr, int32_t* __restrict__ in_edge,
                                                     int m_fill) {
  const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (a >= A) return;
  const int64_t H = off[A];
  // (the staging arrays were not written | a filler atom of structure m_fill: degree 0, as in pbx_pairs_kernel)
  if (cellerr[0] || 2 * H > (int64_t)e_cap || atom_mol[a] == m_fill) {
    if (!kList && lane == 0) deg[a] = 0;
    return;
  }
  const int a0 = mol_off[atom_mol[a]];
  int64_t k = kList ? in_ptr[a] : 0;
  const int64_t f0 = off[a], nf = off[a + 1] - f0;
  if (kList)
    for (int64_t q = lane; q < nf; q += 64) in_edge[k + q] = (int32_t)(f0 + q);
  k += nf;
  for (int i0 = a0; i0 <= a; i0 += 64) {
    const int i = i0 + lane;
    int64_t lo = 0, hi = 0;
    if (i <= a) src_range(s_c, off[i], off[i + 1], a, lo, hi);
    const int c = (int)(hi - lo);
    const int incl = wave_scan_incl(c, lane);
    if (kList)
      for (int q = 0; q < c; ++q) in_edge[k + (incl - c) + q] = (int32_t)(lo + q + H);
    k += __shfl(incl, 63, 64);
  }
  if (!kList && lane == 0) deg[a] = k;
}

// triplets per reduce edge over the e_cap rows; rows behind E (and every row of a build that does not fit) count zero
__global__ void pbx_cnt3_kernel(const int32_t* __restrict__ s_a, const int64_t* __restrict__ deg, const int64_t* __restrict__ off,
                                int A, int e_cap, const int32_t* __restrict__ cellerr, int64_t* __restrict__ cnt3) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= e_cap) return;
  const int64_t E = 2 * off[A];
  const bool ok = !cellerr[0] && E <= (int64_t)e_cap && r < E;
  cnt3[r] = ok ? deg[s_a[r]] - 1 : 0;
}

// one block: all counts against their capacities, the padding rules of padded.py (_fill), the in-degree bound; state[] as
// documented in include/gemnet_hip.h
__global__ __launch_bounds__(256) void pbx_decide_kernel(const int64_t* __restrict__ off, const int64_t* __restrict__ off3,
                                                         const int64_t* __restrict__ deg, int A, int e_cap, int t_cap, int G,
                                                         int deg_bound, const int32_t* __restrict__ cellerr,
                                                         int32_t* __restrict__ state, int layout_gate) {
  // layout_gate: the layout kernel of the same step (pbc_index.hip, gn_pbc_layout) refused the sizes — state[3] holds its bit 128 and stays
  // as it is, so that trip / commit write nothing (block-uniform: every thread reads the same word)
  if (layout_gate && (state[3] & 128)) return;
  __shared__ int64_t mx_s[256];
  int64_t mx = 0;
  for (int a = threadIdx.x; a < A; a += 256) mx = deg[a] > mx ? deg[a] : mx;
  mx_s[threadIdx.x] = mx;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (threadIdx.x < w && mx_s[threadIdx.x + w] > mx_s[threadIdx.x]) mx_s[threadIdx.x] = mx_s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  mx = mx_s[0];
  int err = cellerr[0];
  int64_t E = 0, T = 0;
  if (!err) {
    E = 2 * off[A];
    if (E > (int64_t)e_cap) {
      err |= 1;
    } else {
      T = off3[e_cap];
      if (T > (int64_t)t_cap) err |= 2;
    }
  }
  if (!err) {
    const int64_t ep = e_cap - E, tp = t_cap - T;
    const int bound = deg_bound > 2 ? deg_bound : 2;
    if ((tp > 0 && ep < 4) || (tp & 1)) err |= 4;
    // largest in-degree of a dummy atom, exactly (padded.py, pad_in_degree of a periodic runner): atom a of a group takes
    // BOTH forward edges of every quad the group holds; the quads cycle over the groups, an odd last pair opens a new quad
    const int64_t qf = ep / 4, rem = (ep / 2) & 1;
    const int64_t pad_deg = qf % G ? 2 * (qf / G + 1) : 2 * (qf / G) + rem;
    if (pad_deg > bound) err |= 8;
    if (mx > (int64_t)deg_bound) err |= 16;
  }
  state[0] |= err;
  state[1] = (int32_t)(E > 0x7fffffff ? 0x7fffffff : E);
  state[2] = (int32_t)(T > 0x7fffffff ? 0x7fffffff : T);
  state[3] = err;
  state[4] = (int32_t)(mx > 0x7fffffff ? 0x7fffffff : mx);
}

// 16 lanes per reduce edge r: the incoming edges x != r of its target atom, ascending (the list is ascending and holds r once)
__global__ __launch_bounds__(256) void pbx_trip_kernel(const int32_t* __restrict__ s_a, const int64_t* __restrict__ off, int A,
                                                       const int64_t* __restrict__ in_ptr, const int32_t* __restrict__ in_edge,
                                                       const int64_t* __restrict__ off3, int e_cap, int t_cap,
                                                       const int32_t* __restrict__ state, int32_t* __restrict__ red,
                                                       int32_t* __restrict__ exp) {
  if (state[3]) return;
  const int r = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 4), sub = threadIdx.x & 15;
  if (r >= e_cap || r >= 2 * off[A]) return;
  const int a = s_a[r];
  const int64_t o0 = off3[r], p0 = in_ptr[a];
  const int d = (int)(in_ptr[a + 1] - p0);
  for (int q = sub; q < d; q += 16) {
    const int32_t x = in_edge[p0 + q];
    if (x == r) continue;
    const int64_t o = o0 + q - (x > r ? 1 : 0);
    if (o >= (int64_t)t_cap) continue;                        // (cannot happen: T <= t_cap was decided)
    red[o] = r;
    exp[o] = x;
  }
}

}  // namespace
