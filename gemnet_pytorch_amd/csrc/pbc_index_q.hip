// Periodic cells for GemNet-Q: the image-aware quadruplet index build on top of the edge list of pbc.hip
// (gn_pbc_qindex_*; conventions in include/gemnet_hip.h).  The reference's get_quadruplets (data_container.py:428-489) with
// every node identified by (atom, image): for a quadruplet c -> a - b <- d, a sits in image 0, c in n_c = cell_offsets[ca],
// b in n_b (the offset of the interaction edge) and d in n_b + cell_offsets[db].
//
// Interaction edges (b -> a, n): every image with |R_a - (R_b + n cell)| <= int_cutoff except (b == a, n == 0), both
// directions, ordered by (a, b, n) with n lexicographic.  The distance of a pair is evaluated once, on its canonical forward
// form (a < b, or a == b and n lexicographically positive; the other direction tests (b, a, -n)), so the two directions of a
// pair cannot disagree by a rounding; without images that is the molecular builder's test, bit for bit.
// Incoming edges of an atom for the intermediate triplets: ordered by (source atom, cell offset lexicographic) — the
// molecular builder's source-atom order (scipy's CSR column order) extended by the image.  The in-degrees are those of
// gn_pbc_index_fill, so its in_ptr is reused.
// Quadruplets: ordered by (reduce edge c -> a, expand edge d -> b, interaction edge).  Forward edge ids are ordered by their
// target atom and swapped ids by the forward order of their twins, so one wavefront per reduce edge walks the forward edges
// of its structure twice (ids e, then e + H), looks the interaction edges a - b of each candidate up by bisection, counts the
// survivors of the three node tests per lane and places them with a wave scan: the canonical order without a sort and
// without atomics.  Without images this is the molecular builder's order, array for array.
// Count pass + single-block exclusive scan (int64) + fill pass, sizes read back by the caller in between.
#include "common.h"
#include "pbc_image.h"

namespace {

// (b -> a, n) within the cutoff, evaluated on the canonical forward form of the pair
template <typename T>
__device__ __forceinline__ bool int_within(const T* __restrict__ R, const T* __restrict__ C, int a, int b, int n0, int n1, int n2,
                                           T cutoff) {
  if (a < b || (a == b && lex_positive(n0, n1, n2))) return within<T>(R, C, a, b, n0, n1, n2, cutoff);
  return within<T>(R, C, b, a, -n0, -n1, -n2, cutoff);
}

// one thread per target atom a: its interaction edges (a, b, n); count or fill
template <typename T, bool kFill>
__global__ void pbq_int_kernel(const T* __restrict__ R, const T* __restrict__ cell, const uint8_t* __restrict__ pbc,
                               const int32_t* __restrict__ mol_off, const int32_t* __restrict__ atom_mol, int A, T cutoff,
                               int64_t* __restrict__ cnt, const int64_t* __restrict__ off_int, int64_t n_int,
                               int32_t* __restrict__ int_a, int32_t* __restrict__ int_b, int32_t* __restrict__ int_offs) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= A) return;
  const int m = atom_mol[a];
  const int a0 = mol_off[m], a1 = mol_off[m + 1];
  const T* C = cell + 9 * (int64_t)m;
  int64_t k = kFill ? off_int[a] : 0;
  for (int b = a0; b < a1; ++b) {
    const Range rg = image_range<T>(R, cell, pbc, m, a, b, (double)cutoff);
    for (int n0 = rg.lo[0]; n0 <= rg.hi[0]; ++n0)
      for (int n1 = rg.lo[1]; n1 <= rg.hi[1]; ++n1)
        for (int n2 = rg.lo[2]; n2 <= rg.hi[2]; ++n2) {
          if (b == a && n0 == 0 && n1 == 0 && n2 == 0) continue;
          if (!int_within<T>(R, C, a, b, n0, n1, n2, cutoff)) continue;
          if (kFill && k < n_int) {
            int_a[k] = a;
            int_b[k] = b;
            int_offs[3 * k] = n0; int_offs[3 * k + 1] = n1; int_offs[3 * k + 2] = n2;
          }
          ++k;
        }
  }
  if (!kFill) cnt[a] = k;
}

// one thread per atom a: its incoming edges ordered by (source atom, cell offset) and the position of every edge in that list.
// Sources i < a: the swapped twins of the forward edges (i, a, n), offset -n — descending forward id; i == a: the swapped
// self-image edges (offsets lexicographically negative), then the forward ones; sources j > a: forward edges, ascending.
__global__ void pbq_in_src_kernel(const int32_t* __restrict__ mol_off, const int32_t* __restrict__ atom_mol, int A,
                                  const int64_t* __restrict__ off, const int32_t* __restrict__ id_c, int64_t H,
                                  const int64_t* __restrict__ in_ptr, int32_t* __restrict__ in_src,
                                  int32_t* __restrict__ pos_src) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= A) return;
  const int a0 = mol_off[atom_mol[a]];
  const int64_t p0 = in_ptr[a], p1 = in_ptr[a + 1];
  int64_t p = p0;
  auto put = [&](int64_t e) {
    if (p >= p1) return;                                      // (cannot happen: gn_pbc_index_fill counted the same edges)
    in_src[p] = (int32_t)e;
    pos_src[e] = (int32_t)(p - p0);
    ++p;
  };
  int64_t lo, hi;
  for (int i = a0; i < a; ++i) {
    src_range(id_c, off[i], off[i + 1], a, lo, hi);
    for (int64_t e = hi - 1; e >= lo; --e) put(e + H);
  }
  src_range(id_c, off[a], off[a + 1], a, lo, hi);
  for (int64_t e = hi - 1; e >= lo; --e) put(e + H);
  for (int64_t e = lo; e < off[a + 1]; ++e) put(e);
}

__global__ void pbq_cnt_intm_kernel(const int32_t* __restrict__ int_a, const int32_t* __restrict__ int_b,
                                    const int64_t* __restrict__ in_ptr, int64_t n_int, int64_t* __restrict__ cnt_ca,
                                    int64_t* __restrict__ cnt_db) {
  const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (k >= n_int) return;
  const int a = int_a[k], b = int_b[k];
  cnt_ca[k] = in_ptr[a + 1] - in_ptr[a];
  cnt_db[k] = in_ptr[b + 1] - in_ptr[b];
}

__global__ void pbq_intm_kernel(const int32_t* __restrict__ int_a, const int32_t* __restrict__ int_b, int64_t n_int,
                                const int64_t* __restrict__ in_ptr, const int32_t* __restrict__ in_src,
                                const int64_t* __restrict__ off_ca, const int64_t* __restrict__ off_db, int64_t n_ca,
                                int64_t n_db, int32_t* __restrict__ red_intm_ca, int32_t* __restrict__ red_intm_ab,
                                int32_t* __restrict__ exp_intm_db, int32_t* __restrict__ exp_intm_ab) {
  const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (k >= n_int) return;
  const int a = int_a[k], b = int_b[k];
  int64_t q = off_ca[k];
  for (int64_t p = in_ptr[a]; p < in_ptr[a + 1] && q < n_ca; ++p, ++q) { red_intm_ca[q] = in_src[p]; red_intm_ab[q] = (int32_t)k; }
  q = off_db[k];
  for (int64_t p = in_ptr[b]; p < in_ptr[b + 1] && q < n_db; ++p, ++q) { exp_intm_db[q] = in_src[p]; exp_intm_ab[q] = (int32_t)k; }
}

struct QuadOut {
  int32_t *red_ca, *exp_db, *red_cab, *exp_abd, *kidx;
};

// one wavefront per reduce edge r = (c -> a, n_c): count its quadruplets (kFill == false) or write them
template <bool kFill>
__global__ __launch_bounds__(256) void pbq_quad_kernel(const int32_t* __restrict__ mol_off, const int32_t* __restrict__ atom_mol,
                                                       const int32_t* __restrict__ id_a, const int32_t* __restrict__ id_c,
                                                       const int32_t* __restrict__ offs, const int64_t* __restrict__ off,
                                                       int64_t H, const int64_t* __restrict__ off_int,
                                                       const int32_t* __restrict__ int_b, const int32_t* __restrict__ int_offs,
                                                       const int32_t* __restrict__ pos_src, const int64_t* __restrict__ off_ca,
                                                       const int64_t* __restrict__ off_db, int64_t* __restrict__ cnt4,
                                                       const int64_t* __restrict__ off4, int64_t Q, QuadOut out) {
  const int64_t r = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= 2 * H) return;                                     // (wave-uniform)
  const int a = id_a[r], c = id_c[r];
  const int nc0 = offs[3 * r], nc1 = offs[3 * r + 1], nc2 = offs[3 * r + 2];
  const int m = atom_mol[a];
  const int64_t f0 = off[mol_off[m]], f1 = off[mol_off[m + 1]];   // the forward edges of a's structure
  const int64_t i0 = off_int[a], i1 = off_int[a + 1];
  const int pr = kFill ? pos_src[r] : 0;
  const int64_t o0 = kFill ? off4[r] : 0;
  int64_t o = o0;
  for (int phase = 0; phase < 2; ++phase) {
    for (int64_t e0 = f0; e0 < f1; e0 += 64) {
      const int64_t e = e0 + lane;
      int cnt = 0, b = 0, d = 0, nd0 = 0, nd1 = 0, nd2 = 0;
      int64_t x = 0, klo = 0, khi = 0;
      if (e < f1) {
        x = phase ? e + H : e;                                // expand edge d -> b
        b = id_a[x];
        d = id_c[x];
        nd0 = offs[3 * x]; nd1 = offs[3 * x + 1]; nd2 = offs[3 * x + 2];
        int_range(int_b, i0, i1, b, klo, khi);
      }
      // (c, n_c) != (b, n_b), (a, 0) != (d, n_b + n_db), (c, n_c) != (d, n_b + n_db)
      auto keep = [&](int64_t k) {
        const int nb0 = int_offs[3 * k], nb1 = int_offs[3 * k + 1], nb2 = int_offs[3 * k + 2];
        const int q0 = nb0 + nd0, q1 = nb1 + nd1, q2 = nb2 + nd2;
        if (c == b && nc0 == nb0 && nc1 == nb1 && nc2 == nb2) return false;
        if (a == d && q0 == 0 && q1 == 0 && q2 == 0) return false;
        if (c == d && nc0 == q0 && nc1 == q1 && nc2 == q2) return false;
        return true;
      };
      for (int64_t k = klo; k < khi; ++k) cnt += keep(k) ? 1 : 0;
      const int incl = wave_scan_incl(cnt, lane);
      if (kFill && cnt > 0) {
        int64_t w = o + (incl - cnt);
        const int px = pos_src[x];
        for (int64_t k = klo; k < khi; ++k) {
          if (!keep(k)) continue;
          if (w < Q) {                                        // (always: the count pass saw the same numbers)
            out.red_ca[w] = (int32_t)r;
            out.exp_db[w] = (int32_t)x;
            out.red_cab[w] = (int32_t)(off_ca[k] + pr);
            out.exp_abd[w] = (int32_t)(off_db[k] + px);
            out.kidx[w] = (int32_t)(w - o0);
          }
          ++w;
        }
      }
      o += __shfl(incl, 63, 64);
    }
  }
  if (!kFill && lane == 0) cnt4[r] = o;
}

template <typename T>
int int_launch(bool fill, const void* R, const void* cell, const uint8_t* pbc, const int32_t* mol_off, const int32_t* atom_mol,
               int A, double cutoff, int64_t* cnt, const int64_t* off_int, int64_t n_int, int32_t* int_a, int32_t* int_b,
               int32_t* int_offs, hipStream_t st) {
  const dim3 g((unsigned)((A + 63) / 64)), b(64);
  if (fill)
    hipLaunchKernelGGL((pbq_int_kernel<T, true>), g, b, 0, st, (const T*)R, (const T*)cell, pbc, mol_off, atom_mol, A, (T)cutoff,
                       cnt, off_int, n_int, int_a, int_b, int_offs);
  else
    hipLaunchKernelGGL((pbq_int_kernel<T, false>), g, b, 0, st, (const T*)R, (const T*)cell, pbc, mol_off, atom_mol, A, (T)cutoff,
                       cnt, off_int, n_int, int_a, int_b, int_offs);
  GN_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int gn_pbc_qindex_count(const void* R, int is_f64, const void* cell, const uint8_t* pbc, const int32_t* mol_off,
                                   const int32_t* atom_mol, int B, int A, double int_cutoff, int64_t* cnt, int64_t* off_int,
                                   void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (A <= 0 || B <= 0) return 0;
  const int rc = is_f64 ? int_launch<double>(false, R, cell, pbc, mol_off, atom_mol, A, int_cutoff, cnt, nullptr, 0, nullptr,
                                             nullptr, nullptr, st)
                        : int_launch<float>(false, R, cell, pbc, mol_off, atom_mol, A, int_cutoff, cnt, nullptr, 0, nullptr,
                                            nullptr, nullptr, st);
  if (rc) return rc;
  hipLaunchKernelGGL(pbc_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, off_int, (int64_t)A);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_pbc_qindex_int(const void* R, int is_f64, const void* cell, const uint8_t* pbc, const int32_t* mol_off,
                                 const int32_t* atom_mol, int A, double int_cutoff, const int64_t* off_int, int64_t n_int,
                                 const int64_t* off_half, int64_t H, const int32_t* id_a, const int32_t* id_c,
                                 const int32_t* cell_offsets, const int64_t* in_ptr, int32_t* int_a, int32_t* int_b,
                                 int32_t* int_cell_offsets, int32_t* in_src, int32_t* pos_src, int64_t* cnt_ca, int64_t* off_ca,
                                 int64_t* cnt_db, int64_t* off_db, int64_t* cnt4, int64_t* off4, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (A <= 0) return 0;
  if (n_int < 0 || H < 0 || n_int > 0x7fffffffLL || 2 * H > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (n_int > 0) {
    const int rc = is_f64 ? int_launch<double>(true, R, cell, pbc, mol_off, atom_mol, A, int_cutoff, nullptr, off_int, n_int,
                                               int_a, int_b, int_cell_offsets, st)
                          : int_launch<float>(true, R, cell, pbc, mol_off, atom_mol, A, int_cutoff, nullptr, off_int, n_int,
                                              int_a, int_b, int_cell_offsets, st);
    if (rc) return rc;
  }
  if (H > 0) {
    hipLaunchKernelGGL(pbq_in_src_kernel, dim3((unsigned)((A + 63) / 64)), dim3(64), 0, st, mol_off, atom_mol, A, off_half, id_c,
                       H, in_ptr, in_src, pos_src);
    GN_LAUNCH_CHECK();
  }
  if (n_int > 0) {
    hipLaunchKernelGGL(pbq_cnt_intm_kernel, dim3((unsigned)gn_cdiv(n_int, 256)), dim3(256), 0, st, int_a, int_b, in_ptr, n_int,
                       cnt_ca, cnt_db);
    GN_LAUNCH_CHECK();
    hipLaunchKernelGGL(pbc_scan_kernel, dim3(1), dim3(1024), 0, st, cnt_ca, off_ca, n_int);
    hipLaunchKernelGGL(pbc_scan_kernel, dim3(1), dim3(1024), 0, st, cnt_db, off_db, n_int);
    GN_LAUNCH_CHECK();
  }
  if (H > 0) {
    const int64_t E = 2 * H;
    hipLaunchKernelGGL((pbq_quad_kernel<false>), dim3((unsigned)gn_cdiv(E, 4)), dim3(256), 0, st, mol_off, atom_mol, id_a, id_c,
                       cell_offsets, off_half, H, off_int, int_b, int_cell_offsets, pos_src, off_ca, off_db, cnt4, off4,
                       (int64_t)0, QuadOut{nullptr, nullptr, nullptr, nullptr, nullptr});
    GN_LAUNCH_CHECK();
    hipLaunchKernelGGL(pbc_scan_kernel, dim3(1), dim3(1024), 0, st, cnt4, off4, E);
    GN_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int gn_pbc_qindex_quad(const int32_t* mol_off, const int32_t* atom_mol, int A, const int64_t* off_half, int64_t H,
                                  const int32_t* id_a, const int32_t* id_c, const int32_t* cell_offsets, const int64_t* in_ptr,
                                  const int32_t* in_src, const int32_t* pos_src, const int64_t* off_int, int64_t n_int,
                                  const int32_t* int_a, const int32_t* int_b, const int32_t* int_cell_offsets,
                                  const int64_t* off_ca, const int64_t* off_db, int64_t n_ca, int64_t n_db, const int64_t* off4,
                                  int64_t Q, int32_t* id4_reduce_intm_ca, int32_t* id4_reduce_intm_ab,
                                  int32_t* id4_expand_intm_db, int32_t* id4_expand_intm_ab, int32_t* id4_reduce_ca,
                                  int32_t* id4_expand_db, int32_t* id4_reduce_cab, int32_t* id4_expand_abd, int32_t* Kidx4,
                                  void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (A <= 0 || n_int <= 0 || H <= 0) return 0;
  if (n_int > 0x7fffffffLL || 2 * H > 0x7fffffffLL || n_ca > 0x7fffffffLL || n_db > 0x7fffffffLL || Q > 0x7fffffffLL)
    return (int)hipErrorInvalidValue;
  if (n_ca > 0 || n_db > 0) {
    hipLaunchKernelGGL(pbq_intm_kernel, dim3((unsigned)gn_cdiv(n_int, 256)), dim3(256), 0, st, int_a, int_b, n_int, in_ptr, in_src,
                       off_ca, off_db, n_ca, n_db, id4_reduce_intm_ca, id4_reduce_intm_ab, id4_expand_intm_db,
                       id4_expand_intm_ab);
    GN_LAUNCH_CHECK();
  }
  if (Q > 0) {
    hipLaunchKernelGGL((pbq_quad_kernel<true>), dim3((unsigned)gn_cdiv(2 * H, 4)), dim3(256), 0, st, mol_off, atom_mol, id_a, id_c,
                       cell_offsets, off_half, H, off_int, int_b, int_cell_offsets, pos_src, off_ca, off_db, (int64_t*)nullptr,
                       off4, Q, QuadOut{id4_reduce_ca, id4_expand_db, id4_reduce_cab, id4_expand_abd, Kidx4});
    GN_LAUNCH_CHECK();
  }
  return 0;
}
