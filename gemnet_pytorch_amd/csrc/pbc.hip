// Periodic cells for GemNet-T (first-order path): the image neighbour list, edge / triplet geometry fused with the basis
// evaluation from SHIFTED edge vectors, and the per-structure strain derivative (stress).
//
// Neighbour list (gn_pbc_index_*): the reference builds edges inside one molecule only (data_container.py:244-316).  With a
// cell, atom c of edge c -> a sits in the image given by the integer offset n (cell_offsets[e]):
//   V_e = R[a] - (R[c] + n cell_b)
// Canonical forward half: pairs (i, j, n) with i < j, or i == j and n lexicographically positive, ordered by (i, j, n) with n
// enumerated lexicographically (n0 outer); edge e of the forward half has id_a = i, id_c = j, offset n; edge e + H has id_a = j,
// id_c = i, offset -n (id_swap = e +- H, id_undir = e mod H).  Without images this is exactly the molecular builder's order.
// Image range per pair and axis: the fractional difference f of R_j - R_i and the cell's perpendicular heights h give
// n_k in [floor(-f_k - c/h_k), ceil(-f_k + c/h_k)] (triclinic cells, cells below 2 cutoff, unwrapped positions); non-periodic
// axes use n_k = 0.  Distances are evaluated like the molecular builder (index_gpu.hip): every operation rounded in R's dtype.
// Triplets: reduce edge r = (c -> a, n_c), expand edges x = (b -> a, n_b) with x != r (edge identity, not atom identity: an
// atom forms triplets with its own images), ascending edge id inside a reduce segment.
// Count pass + exclusive scan (int64) + fill pass; one thread per atom / edge writes its own rows: deterministic, no atomics.
//
// Geometry: the molecular kernels (geometry.hip) recompute vectors from atom positions; here the (E,3) edge vectors are
// materialised once per evaluation (gn_pbc_edge_vec_f32) and the basis kernels read them: the triplet angle c <- a -> b uses
// u = -V[reduce edge], v = -V[expand edge].  Every adjoint returns a per-EDGE vector gradient dE/dV; forces are its
// edge -> atom segmented sums (the shift does not depend on R) and the stress is sum_e V_e (x) dE/dV_e per structure.
#include "common.h"
#include "basis_math.h"
#include "pbc_image.h"

namespace {

// (image_range, within, lex_positive, pbc_scan_kernel, src_range: pbc_image.h, shared with the quadruplet build)

// one thread per atom i: walks its canonical pairs (i, j >= i, n); count (write == false) or fill
template <typename T, bool kFill>
__global__ void pbc_pairs_kernel(const T* __restrict__ R, const T* __restrict__ cell, const uint8_t* __restrict__ pbc,
                                 const int32_t* __restrict__ mol_off, const int32_t* __restrict__ atom_mol, int A, T cutoff,
                                 int64_t* __restrict__ cnt, const int64_t* __restrict__ off, int64_t H,
                                 int32_t* __restrict__ id_a, int32_t* __restrict__ id_c, int32_t* __restrict__ id_undir,
                                 int32_t* __restrict__ id_swap, int32_t* __restrict__ offs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A) return;
  const int m = atom_mol[i];
  const int a1 = mol_off[m + 1];
  const T* C = cell + 9 * (int64_t)m;
  int64_t e = kFill ? off[i] : 0;
  for (int j = i; j < a1; ++j) {
    const Range rg = image_range<T>(R, cell, pbc, m, i, j, (double)cutoff);
    for (int n0 = rg.lo[0]; n0 <= rg.hi[0]; ++n0)
      for (int n1 = rg.lo[1]; n1 <= rg.hi[1]; ++n1)
        for (int n2 = rg.lo[2]; n2 <= rg.hi[2]; ++n2) {
          if (j == i && !lex_positive(n0, n1, n2)) continue;
          if (!within<T>(R, C, i, j, n0, n1, n2, cutoff)) continue;
          if (kFill) {
            const int64_t s = e + H;
            id_a[e] = i; id_c[e] = j;
            id_a[s] = j; id_c[s] = i;
            id_undir[e] = (int32_t)e; id_undir[s] = (int32_t)e;
            id_swap[e] = (int32_t)s; id_swap[s] = (int32_t)e;
            offs[3 * e] = n0; offs[3 * e + 1] = n1; offs[3 * e + 2] = n2;
            offs[3 * s] = -n0; offs[3 * s + 1] = -n1; offs[3 * s + 2] = -n2;
          }
          ++e;
        }
  }
  if (!kFill) cnt[i] = e;
}

// in-degree of atom a (kList == false) or its incoming edges in ascending id: forward edges of a, then the swapped twins of the
// forward edges (i, a, n), i <= a, in ascending forward id
template <bool kList>
__global__ void pbc_in_kernel(const int32_t* __restrict__ mol_off, const int32_t* __restrict__ atom_mol, int A,
                              const int64_t* __restrict__ off, const int32_t* __restrict__ id_c, int64_t H,
                              int64_t* __restrict__ deg, const int64_t* __restrict__ in_ptr, int32_t* __restrict__ in_edge) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= A) return;
  const int a0 = mol_off[atom_mol[a]];
  int64_t k = kList ? in_ptr[a] : 0;
  for (int64_t e = off[a]; e < off[a + 1]; ++e) {
    if (kList) in_edge[k] = (int32_t)e;
    ++k;
  }
  for (int i = a0; i <= a; ++i) {
    int64_t lo, hi;
    src_range(id_c, off[i], off[i + 1], a, lo, hi);
    for (int64_t e = lo; e < hi; ++e) {
      if (kList) in_edge[k] = (int32_t)(e + H);
      ++k;
    }
  }
  if (!kList) deg[a] = k;
}

__global__ void pbc_cnt3_kernel(const int32_t* __restrict__ id_a, const int64_t* __restrict__ deg, int64_t E,
                                int64_t* __restrict__ cnt3) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r < E) cnt3[r] = deg[id_a[r]] - 1;
}

__global__ void pbc_trip_kernel(const int32_t* __restrict__ id_a, int64_t E, const int64_t* __restrict__ in_ptr,
                                const int32_t* __restrict__ in_edge, const int64_t* __restrict__ off3, int32_t* __restrict__ red,
                                int32_t* __restrict__ exp, int32_t* __restrict__ kidx) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= E) return;
  const int a = id_a[r];
  const int64_t o0 = off3[r];
  int64_t o = o0;
  for (int64_t p = in_ptr[a]; p < in_ptr[a + 1]; ++p) {
    const int32_t x = in_edge[p];
    if (x == (int32_t)r) continue;
    red[o] = (int32_t)r;
    exp[o] = x;
    if (kidx) kidx[o] = (int32_t)(o - o0);
    ++o;
  }
}

__global__ void pbc_batch_seg_kernel(const int32_t* __restrict__ atom_mol, int A, int32_t* __restrict__ batch_seg) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a < A) batch_seg[a] = atom_mol[a];
}

// ---- geometry ---------------------------------------------------------------------------------------------------------------
__global__ void pbc_edge_vec_kernel(const float* __restrict__ R, const int32_t* __restrict__ id_c,
                                    const int32_t* __restrict__ id_a, const int32_t* __restrict__ batch_seg,
                                    const float* __restrict__ cell, const int32_t* __restrict__ offs, float* __restrict__ V,
                                    int64_t E) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int a = id_a[e], c = id_c[e];
    const float* C = cell + 9 * (int64_t)batch_seg[a];
    const float n0 = (float)offs[3 * e], n1 = (float)offs[3 * e + 1], n2 = (float)offs[3 * e + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float sh = __fadd_rn(__fadd_rn(__fmul_rn(n0, C[k]), __fmul_rn(n1, C[3 + k])), __fmul_rn(n2, C[6 + k]));
      V[3 * e + k] = R[3 * (int64_t)a + k] - (R[3 * (int64_t)c + k] + sh);
    }
  }
}

// D[e] = |V[e]|; rbf[e,n]; rad[e,l,n]: edge_basis_fwd_kernel (geometry.hip) with the vector read instead of recomputed
__global__ void edge_basis_vec_fwd_kernel(const float* __restrict__ V, const float* __restrict__ freq,
                                          const float* __restrict__ z, const double* __restrict__ nrm, float* __restrict__ D,
                                          float* __restrict__ rbf, float* __restrict__ rad, int64_t E, int NR, int S,
                                          double cutoff, int p) {
  const int sub = threadIdx.x & 15;
  const int nfun = NR + S * NR;
  for (int64_t e = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 4; e < E; e += ((int64_t)gridDim.x * blockDim.x) >> 4) {
    const float vx = V[3 * e], vy = V[3 * e + 1], vz = V[3 * e + 2];
    const float d = sqrtf(vx * vx + vy * vy + vz * vz);
    if (sub == 0) D[e] = d;
    for (int j = sub; j < nfun; j += 16) {
      if (j < NR) {
        if (rbf) rbf[e * NR + j] = (float)bessel_rbf_eval((double)d, (double)freq[j], cutoff, p, 0, 0);
      } else {
        const int lr = j - NR;
        rad[e * S * NR + lr] = (float)sph_radial_eval((double)d, (double)z[lr], nrm[lr], lr / NR, cutoff, p, 0);
      }
    }
  }
}

// W[e,:] = dE/dV_e = gD V / d (gD as in edge_basis_bwd_kernel: fixed-order 16-lane sum)
__global__ void edge_basis_vec_bwd_kernel(const float* __restrict__ g_D, const float* __restrict__ g_rbf,
                                          const float* __restrict__ g_rad, const float* __restrict__ V,
                                          const float* __restrict__ freq, const float* __restrict__ z,
                                          const double* __restrict__ nrm, float* __restrict__ Wout, int64_t E, int NR, int S,
                                          double cutoff, int p) {
  const int sub = threadIdx.x & 15;
  const int64_t e = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 4;
  const bool ok = e < E;
  float vx = 0.f, vy = 0.f, vz = 0.f, d = 1.f;
  double g = 0.0;
  if (ok) {
    vx = V[3 * e]; vy = V[3 * e + 1]; vz = V[3 * e + 2];
    d = sqrtf(vx * vx + vy * vy + vz * vz);
    const int nfun = NR + S * NR;
    for (int j = sub; j < nfun; j += 16) {
      if (j < NR) {
        if (g_rbf) g += (double)g_rbf[e * NR + j] * bessel_rbf_eval((double)d, (double)freq[j], cutoff, p, 1, 0);
      } else if (g_rad) {
        const int lr = j - NR;
        g += (double)g_rad[e * S * NR + lr] * sph_radial_eval((double)d, (double)z[lr], nrm[lr], lr / NR, cutoff, p, 1);
      }
    }
  }
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) g += __shfl_xor(g, m, 16);
  if (ok && sub == 0) {
    if (g_D) g += (double)g_D[e];
    const float sc = (float)(g / (double)d);
    Wout[3 * e] = sc * vx; Wout[3 * e + 1] = sc * vy; Wout[3 * e + 2] = sc * vz;
  }
}

struct AngV { float ux, uy, uz, vx, vy, vz, wx, wy, wz, x, y; bool clamped; };

// u = -V[r] (a -> image of c), v = -V[x] (a -> image of b); same arithmetic as angle_of (geometry.hip)
__device__ __forceinline__ AngV angle_of_edges(const float* __restrict__ V, int r, int x) {
  AngV g;
  g.ux = -V[3 * (int64_t)r]; g.uy = -V[3 * (int64_t)r + 1]; g.uz = -V[3 * (int64_t)r + 2];
  g.vx = -V[3 * (int64_t)x]; g.vy = -V[3 * (int64_t)x + 1]; g.vz = -V[3 * (int64_t)x + 2];
  g.x = g.ux * g.vx + g.uy * g.vy + g.uz * g.vz;
  g.wx = g.uy * g.vz - g.uz * g.vy;
  g.wy = g.uz * g.vx - g.ux * g.vz;
  g.wz = g.ux * g.vy - g.uy * g.vx;
  const float yn = sqrtf(g.wx * g.wx + g.wy * g.wy + g.wz * g.wz);
  g.clamped = yn < 1e-9f;
  g.y = g.clamped ? 1e-9f : yn;
  return g;
}

__global__ void trip_basis_vec_fwd_kernel(const float* __restrict__ V, const int32_t* __restrict__ red,
                                          const int32_t* __restrict__ exp, float* __restrict__ Y, float* __restrict__ theta,
                                          int64_t T, int S) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    const AngV g = angle_of_edges(V, red[t], exp[t]);
    const float th = atan2f(g.y, g.x);
    if (theta) theta[t] = th;
    ylm0_row((double)th, S, 0, Y + t * S);
  }
}

// Gu[t,:] = dE/du, Gv[t,:] = dE/dv (u = -V[reduce edge], v = -V[expand edge])
__global__ void trip_basis_vec_bwd_kernel(const float* __restrict__ gY, const float* __restrict__ V,
                                          const int32_t* __restrict__ red, const int32_t* __restrict__ exp,
                                          float* __restrict__ Gu, float* __restrict__ Gv, int64_t T, int S) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    const AngV g = angle_of_edges(V, red[t], exp[t]);
    const float th = atan2f(g.y, g.x);
    float dY[8];
    ylm0_row((double)th, S, 1, dY);
    float gth = 0.f;
    for (int l = 0; l < S; ++l) gth += gY[t * S + l] * dY[l];
    const float r2 = g.x * g.x + g.y * g.y;
    const float dx = -g.y / r2 * gth;
    const float dy = g.clamped ? 0.f : g.x / r2 * gth;
    const float iy = g.clamped ? 0.f : 1.0f / g.y;
    const float nx = g.wx * iy, ny = g.wy * iy, nz = g.wz * iy;
    Gu[3 * t] = dx * g.vx + dy * (g.vy * nz - g.vz * ny);
    Gu[3 * t + 1] = dx * g.vy + dy * (g.vz * nx - g.vx * nz);
    Gu[3 * t + 2] = dx * g.vz + dy * (g.vx * ny - g.vy * nx);
    Gv[3 * t] = dx * g.ux + dy * (ny * g.uz - nz * g.uy);
    Gv[3 * t + 1] = dx * g.uy + dy * (nz * g.ux - nx * g.uz);
    Gv[3 * t + 2] = dx * g.uz + dy * (nx * g.uy - ny * g.ux);
  }
}

// one workgroup per structure b: S[b] = scale / |det cell_b| * sum_{e in b} V_e (x) G_e, fixed order (strided per thread in f64,
// then a fixed tree in LDS)
__global__ __launch_bounds__(256) void pbc_stress_kernel(const float* __restrict__ V, const float* __restrict__ G,
                                                         const int32_t* __restrict__ perm, const int32_t* __restrict__ seg,
                                                         const float* __restrict__ cell, float scale, float* __restrict__ S) {
  __shared__ double red_s[9][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  double acc[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) acc[q] = 0.0;
  for (int64_t p = seg[b] + tid; p < seg[b + 1]; p += 256) {
    const int64_t e = perm ? perm[p] : p;
    const double v[3] = {V[3 * e], V[3 * e + 1], V[3 * e + 2]};
    const double g[3] = {G[3 * e], G[3 * e + 1], G[3 * e + 2]};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[3 * i + j] += v[i] * g[j];
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) red_s[q][tid] = acc[q];
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int q = 0; q < 9; ++q) red_s[q][tid] += red_s[q][tid + w];
    }
    __syncthreads();
  }
  if (tid < 9) {
    const float* C = cell + 9 * (int64_t)b;
    const double det = (double)C[0] * ((double)C[4] * C[8] - (double)C[5] * C[7]) -
                       (double)C[1] * ((double)C[3] * C[8] - (double)C[5] * C[6]) +
                       (double)C[2] * ((double)C[3] * C[7] - (double)C[4] * C[6]);
    S[9 * (int64_t)b + tid] = (float)((double)scale * red_s[tid][0] / fabs(det));
  }
}

inline int grid_pbc(int64_t n) {
  int64_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

template <typename T>
int pairs_launch(bool fill, const void* R, const void* cell, const uint8_t* pbc, const int32_t* mol_off, const int32_t* atom_mol,
                 int A, double cutoff, int64_t* cnt, const int64_t* off, int64_t H, int32_t* id_a, int32_t* id_c,
                 int32_t* id_undir, int32_t* id_swap, int32_t* offs, hipStream_t st) {
  const dim3 g((unsigned)((A + 127) / 128)), b(128);
  if (fill)
    hipLaunchKernelGGL((pbc_pairs_kernel<T, true>), g, b, 0, st, (const T*)R, (const T*)cell, pbc, mol_off, atom_mol, A, (T)cutoff,
                       cnt, off, H, id_a, id_c, id_undir, id_swap, offs);
  else
    hipLaunchKernelGGL((pbc_pairs_kernel<T, false>), g, b, 0, st, (const T*)R, (const T*)cell, pbc, mol_off, atom_mol, A,
                       (T)cutoff, cnt, off, H, id_a, id_c, id_undir, id_swap, offs);
  GN_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int gn_pbc_index_count(const void* R, int is_f64, const void* cell, const uint8_t* pbc, const int32_t* mol_off,
                                  const int32_t* atom_mol, int B, int A, double cutoff, int64_t* cnt, int64_t* off_half,
                                  void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (A <= 0 || B <= 0) return 0;
  const int rc = is_f64 ? pairs_launch<double>(false, R, cell, pbc, mol_off, atom_mol, A, cutoff, cnt, nullptr, 0, nullptr,
                                               nullptr, nullptr, nullptr, nullptr, st)
                        : pairs_launch<float>(false, R, cell, pbc, mol_off, atom_mol, A, cutoff, cnt, nullptr, 0, nullptr,
                                              nullptr, nullptr, nullptr, nullptr, st);
  if (rc) return rc;
  hipLaunchKernelGGL(pbc_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, off_half, (int64_t)A);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_pbc_index_fill(const void* R, int is_f64, const void* cell, const uint8_t* pbc, const int32_t* mol_off,
                                 const int32_t* atom_mol, int A, double cutoff, const int64_t* off_half, int64_t H,
                                 int32_t* batch_seg, int32_t* id_a, int32_t* id_c, int32_t* id_undir, int32_t* id_swap,
                                 int32_t* cell_offsets, int64_t* deg, int64_t* in_ptr, int32_t* in_edge, int64_t* cnt3,
                                 int64_t* off3, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (A <= 0) return 0;
  if (2 * H > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(pbc_batch_seg_kernel, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, st, atom_mol, A, batch_seg);
  GN_LAUNCH_CHECK();
  if (H <= 0) return 0;
  const int rc = is_f64 ? pairs_launch<double>(true, R, cell, pbc, mol_off, atom_mol, A, cutoff, nullptr, off_half, H, id_a, id_c,
                                               id_undir, id_swap, cell_offsets, st)
                        : pairs_launch<float>(true, R, cell, pbc, mol_off, atom_mol, A, cutoff, nullptr, off_half, H, id_a, id_c,
                                              id_undir, id_swap, cell_offsets, st);
  if (rc) return rc;
  const dim3 ga((unsigned)((A + 127) / 128)), b(128);
  hipLaunchKernelGGL((pbc_in_kernel<false>), ga, b, 0, st, mol_off, atom_mol, A, off_half, id_c, H, deg, nullptr, nullptr);
  GN_LAUNCH_CHECK();
  hipLaunchKernelGGL(pbc_scan_kernel, dim3(1), dim3(1024), 0, st, deg, in_ptr, (int64_t)A);
  GN_LAUNCH_CHECK();
  hipLaunchKernelGGL((pbc_in_kernel<true>), ga, b, 0, st, mol_off, atom_mol, A, off_half, id_c, H, nullptr, in_ptr, in_edge);
  GN_LAUNCH_CHECK();
  const int64_t E = 2 * H;
  hipLaunchKernelGGL(pbc_cnt3_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, id_a, deg, E, cnt3);
  GN_LAUNCH_CHECK();
  hipLaunchKernelGGL(pbc_scan_kernel, dim3(1), dim3(1024), 0, st, cnt3, off3, E);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_pbc_index_trip(const int32_t* id_a, int64_t E, const int64_t* in_ptr, const int32_t* in_edge,
                                 const int64_t* off3, int32_t* id3_reduce_ca, int32_t* id3_expand_ba, int32_t* Kidx3,
                                 void* stream) {
  if (E <= 0) return 0;
  hipLaunchKernelGGL(pbc_trip_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), id_a, E,
                     in_ptr, in_edge, off3, id3_reduce_ca, id3_expand_ba, Kidx3);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_pbc_edge_vec_f32(const float* R, const int32_t* id_c, const int32_t* id_a, const int32_t* batch_seg,
                                   const float* cell, const int32_t* cell_offsets, float* V, int64_t E, void* stream) {
  if (E <= 0) return 0;
  hipLaunchKernelGGL(pbc_edge_vec_kernel, dim3(grid_pbc(E)), dim3(256), 0, static_cast<hipStream_t>(stream), R, id_c, id_a,
                     batch_seg, cell, cell_offsets, V, E);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_edge_basis_vec_fwd_f32(const float* V, const float* freq, const float* z, const double* nrm, float* D,
                                         float* rbf, float* rad, int64_t E, int NR, int S, float cutoff, int p, void* stream) {
  if (E <= 0) return 0;
  if (p < 2 || S > 8) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(edge_basis_vec_fwd_kernel, dim3(grid_pbc(E * 16)), dim3(256), 0, static_cast<hipStream_t>(stream), V, freq, z,
                     nrm, D, rbf, rad, E, NR, S, (double)cutoff, p);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_edge_basis_vec_bwd_f32(const float* g_D, const float* g_rbf, const float* g_rad, const float* V,
                                         const float* freq, const float* z, const double* nrm, float* W, int64_t E, int NR,
                                         int S, float cutoff, int p, void* stream) {
  if (E <= 0) return 0;
  if (p < 2 || S > 8) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(edge_basis_vec_bwd_kernel, dim3((unsigned)((E * 16 + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), g_D, g_rbf, g_rad, V, freq, z, nrm, W, E, NR, S, (double)cutoff, p);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_trip_basis_vec_fwd_f32(const float* V, const int32_t* red, const int32_t* exp, float* Y, float* theta,
                                         int64_t T, int S, void* stream) {
  if (T <= 0) return 0;
  if (S > 8) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(trip_basis_vec_fwd_kernel, dim3(grid_pbc(T)), dim3(256), 0, static_cast<hipStream_t>(stream), V, red, exp, Y,
                     theta, T, S);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_trip_basis_vec_bwd_f32(const float* gY, const float* V, const int32_t* red, const int32_t* exp, float* Gu,
                                         float* Gv, int64_t T, int S, void* stream) {
  if (T <= 0) return 0;
  if (S > 8) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(trip_basis_vec_bwd_kernel, dim3(grid_pbc(T)), dim3(256), 0, static_cast<hipStream_t>(stream), gY, V, red, exp,
                     Gu, Gv, T, S);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_pbc_stress_f32(const float* V, const float* G, const int32_t* perm, const int32_t* seg_off, const float* cell,
                                 int B, float scale, float* S, void* stream) {
  if (B <= 0) return 0;
  hipLaunchKernelGGL(pbc_stress_kernel, dim3((unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), V, G, perm, seg_off,
                     cell, scale, S);
  GN_LAUNCH_CHECK();
  return 0;
}
