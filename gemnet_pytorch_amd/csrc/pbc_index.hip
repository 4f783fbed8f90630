// Capacity form of the periodic image neighbour list (gn_pbc_index_padded_t): the list of csrc/pbc.hip — same canonical order,
// same float32 distance arithmetic — built with NO read-back into capacity-sized arrays, followed by the pad rows of
// gemnet_pytorch_amd/padded.py, so that neighbour list + model are ONE capturable graph (the periodic twin of
// gn_index_gpu_padded_t, index_gpu.hip).  The cell is read from device memory at replay time.
//
// Pair search: one WAVEFRONT per atom i, lanes over the partner atoms j >= i of its structure (64 at a time).  A lane counts the
// images of its own pair inside the cutoff, a wave-level exclusive scan (__shfl_up) places the lanes' runs in ascending j, and
// the lane writes its images in lexicographic n: the canonical (i, j, n) order without a sort and without atomics.  While it
// counts, a lane keeps the hits of its pair as a bit mask when the image box has at most 64 cells (a 3 x 3 x 3 box has 27), so
// that the write phase does not repeat the distance tests.  The per-structure part of the image range (cofactors, determinant,
// cutoff / height) is computed once per call by pbx_cell_kernel, which also checks the cell (error bits 32 and 64).
//
// Order of the launches and what protects the arrays:
//   cell -> pairs<count> -> scan -> pairs<fill> (into STAGING; returns when 2H > e_cap) -> in<count> -> scan -> in<list> -> cnt3
//   -> scan -> decide (one block: every count against its capacity, the padding rules, the in-degree bound; writes state[])
//   -> trip (straight into the model's arrays, only when state[3] == 0) -> commit (edges from staging + all pad rows, ditto).
// Every kernel that indexes with a count checks the capacity that bounds it first; after an error nothing the model reads is
// written, so the arrays keep the previous step's valid contents (gn_index_poison_f32 then turns the outputs into NaN).
//
// Atom capacity (gn_pbc_layout + gn_pbc_index_padded_tv): batches whose structure sizes change from replay to replay.  The
// layout kernels (layout_cap.h, shared with the molecular gn_index_gpu_layout) turn the device-resident sizes N into mol_off / atom_mol / batch_seg / the padded N / the loss mask (one block
// scans the structures, a grid over the atom rows bisects mol_off; error bit 128 and no write when the sizes do not add up to
// n_atoms, hold a zero or exceed a_cap).  The index build then runs the SAME kernels over a_cap atom rows: the atoms between
// the batch and the capacity belong to "structure" n_mol and leave their waves at once with count 0 and degree 0, wherever they
// sit; the real atoms come first, so the canonical order of the real rows is that of the batch on its own.
#include "common.h"
#include "layout_cap.h"
#include "pbc_index_cap.h"

namespace {

struct PadP {
  const int32_t *s_c, *s_a, *s_swap, *s_undir, *s_offs;
  int32_t *id_c, *id_a, *id_swap, *id_undir, *offs, *red, *exp;
};

// edges from staging, then the pad rows of padded.py (_pad_edges / _pad_triplets, triplets-only layout; offsets 0)
__global__ void pbx_commit_pad_kernel(PadP p, int e_cap, int t_cap, int a_cap, int G, const int32_t* __restrict__ state) {
  if (state[3]) return;
  const int64_t E = state[1], T = state[2];
  const int64_t ep = e_cap - E, tp = t_cap - T;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < e_cap; i += nth) {
    if (i < E) {
      p.id_c[i] = p.s_c[i]; p.id_a[i] = p.s_a[i]; p.id_swap[i] = p.s_swap[i]; p.id_undir[i] = p.s_undir[i];
      p.offs[3 * i] = p.s_offs[3 * i]; p.offs[3 * i + 1] = p.s_offs[3 * i + 1]; p.offs[3 * i + 2] = p.s_offs[3 * i + 2];
    } else {
      const int64_t k = i - E, pair = k >> 1;
      const int rev = (int)(k & 1), typ = (int)(pair & 1), grp = (int)((pair >> 1) % G);
      const int a = a_cap + 3 * grp, other = a + 1 + typ;
      p.id_c[i] = rev ? a : other;
      p.id_a[i] = rev ? other : a;
      p.id_swap[i] = (int32_t)(E + (k ^ 1));
      p.id_undir[i] = (int32_t)(E / 2 + pair);
      p.offs[3 * i] = 0; p.offs[3 * i + 1] = 0; p.offs[3 * i + 2] = 0;
    }
  }
  const int64_t n_fwd = 2 * (ep / 4), den = tp > 1 ? tp : 1;
  for (int64_t i = T + tid; i < t_cap; i += nth) {
    const int64_t f = ((i - T) * n_fwd) / den;
    p.red[i] = (int32_t)(E + 2 * f);
    p.exp[i] = (int32_t)(E + 2 * (f ^ 1));
  }
}

inline size_t al64(size_t x) { return (x + 63) & ~(size_t)63; }

struct pbx_ws {
  double* geo;
  int64_t *cnt, *off, *deg, *in_ptr, *cnt3, *off3;
  int32_t *in_edge, *cellerr;
};

size_t pbx_layout(char* base, int A, int e_cap, pbx_ws* w) {
  size_t o = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += al64(bytes); return p; };
  w->geo = (double*)take(8 * (size_t)kGeo * A);               // B <= A structures
  w->cnt = (int64_t*)take(8 * (size_t)A);
  w->off = (int64_t*)take(8 * ((size_t)A + 1));
  w->deg = (int64_t*)take(8 * (size_t)A);
  w->in_ptr = (int64_t*)take(8 * ((size_t)A + 1));
  w->cnt3 = (int64_t*)take(8 * (size_t)e_cap);
  w->off3 = (int64_t*)take(8 * ((size_t)e_cap + 1));
  w->in_edge = (int32_t*)take(4 * (size_t)e_cap);
  w->cellerr = (int32_t*)take(64);
  return o;
}

}  // namespace

extern "C" int64_t gn_pbc_index_ws_bytes(int A, int e_cap) {
  pbx_ws w;
  return (int64_t)pbx_layout(nullptr, A > 0 ? A : 0, e_cap > 0 ? e_cap : 0, &w);
}

namespace {

// the launches of gn_pbc_index_padded_t over A atom rows and B structures.  m_fill / layout_gate: the atom-capacity form
// (gn_pbc_index_padded_tv) — atoms of structure m_fill are fillers without pairs, and a layout the same step refused (bit 128
// in state[3]) lets neither decide nor trip nor commit write; -1 / 0: the fixed layout.
int pbx_run(const float* R, const float* cell, const uint8_t* pbc, const int32_t* mol_off, const int32_t* atom_mol, int B, int A,
            int m_fill, int layout_gate, double cutoff, void* ws, int e_cap, int t_cap, int a_cap, int n_groups, int deg_bound,
            int32_t* staging, int32_t* id_c, int32_t* id_a, int32_t* id_swap, int32_t* id_undir, int32_t* cell_offsets,
            int32_t* id3_reduce_ca, int32_t* id3_expand_ba, int32_t* state, hipStream_t st) {
  pbx_ws w;
  pbx_layout((char*)ws, A, e_cap, &w);
  int32_t *s_a = staging, *s_c = staging + e_cap, *s_undir = staging + 2 * (size_t)e_cap, *s_swap = staging + 3 * (size_t)e_cap,
          *s_offs = staging + 4 * (size_t)e_cap;
  const dim3 gw(gn_cdiv(A, 4)), b256(256), one(1);
  hipLaunchKernelGGL(pbx_cell_kernel, one, dim3(64), 0, st, cell, pbc, B, cutoff, w.geo, w.cellerr);
  hipLaunchKernelGGL((pbx_pairs_kernel<false>), gw, b256, 0, st, R, cell, pbc, mol_off, atom_mol, A, (float)cutoff, w.geo, w.cellerr,
                     w.cnt, w.off, e_cap, s_a, s_c, s_undir, s_swap, s_offs, m_fill);
  hipLaunchKernelGGL(pbc_scan_kernel, one, dim3(1024), 0, st, w.cnt, w.off, (int64_t)A);
  hipLaunchKernelGGL((pbx_pairs_kernel<true>), gw, b256, 0, st, R, cell, pbc, mol_off, atom_mol, A, (float)cutoff, w.geo, w.cellerr,
                     w.cnt, w.off, e_cap, s_a, s_c, s_undir, s_swap, s_offs, m_fill);
  GN_LAUNCH_CHECK();
  hipLaunchKernelGGL((pbx_in_kernel<false>), gw, b256, 0, st, mol_off, atom_mol, A, w.off, s_c, e_cap, w.cellerr, w.deg, w.in_ptr,
                     w.in_edge, m_fill);
  hipLaunchKernelGGL(pbc_scan_kernel, one, dim3(1024), 0, st, w.deg, w.in_ptr, (int64_t)A);
  hipLaunchKernelGGL((pbx_in_kernel<true>), gw, b256, 0, st, mol_off, atom_mol, A, w.off, s_c, e_cap, w.cellerr, w.deg, w.in_ptr,
                     w.in_edge, m_fill);
  hipLaunchKernelGGL(pbx_cnt3_kernel, dim3(gn_cdiv(e_cap, 256)), b256, 0, st, s_a, w.deg, w.off, A, e_cap, w.cellerr, w.cnt3);
  hipLaunchKernelGGL(pbc_scan_kernel, one, dim3(1024), 0, st, w.cnt3, w.off3, (int64_t)e_cap);
  GN_LAUNCH_CHECK();
  hipLaunchKernelGGL(pbx_decide_kernel, one, b256, 0, st, w.off, w.off3, w.deg, A, e_cap, t_cap, n_groups, deg_bound, w.cellerr,
                     state, layout_gate);
  hipLaunchKernelGGL(pbx_trip_kernel, dim3(gn_cdiv((int64_t)e_cap * 16, 256)), b256, 0, st, s_a, w.off, A, w.in_ptr, w.in_edge,
                     w.off3, e_cap, t_cap, state, id3_reduce_ca, id3_expand_ba);
  PadP p{s_c, s_a, s_swap, s_undir, s_offs, id_c, id_a, id_swap, id_undir, cell_offsets, id3_reduce_ca, id3_expand_ba};
  const int64_t work = e_cap > t_cap ? e_cap : t_cap;
  hipLaunchKernelGGL(pbx_commit_pad_kernel, dim3((unsigned)(gn_cdiv(work, 256) < 2048 ? gn_cdiv(work, 256) : 2048)), b256, 0, st, p,
                     e_cap, t_cap, a_cap, n_groups, state);
  GN_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int gn_pbc_index_padded_t(const float* R, const float* cell, const uint8_t* pbc, const int32_t* mol_off,
                                     const int32_t* atom_mol, int B, int A, double cutoff, void* ws, int e_cap, int t_cap,
                                     int a_cap, int n_groups, int deg_bound, int32_t* staging, int32_t* id_c, int32_t* id_a,
                                     int32_t* id_swap, int32_t* id_undir, int32_t* cell_offsets, int32_t* id3_reduce_ca,
                                     int32_t* id3_expand_ba, int32_t* state, void* stream) {
  if (A <= 0 || B <= 0 || B > A || e_cap <= 0 || t_cap <= 0 || n_groups <= 0 || (e_cap & 1) || (t_cap & 1) || a_cap < A)
    return (int)hipErrorInvalidValue;
  return pbx_run(R, cell, pbc, mol_off, atom_mol, B, A, -1, 0, cutoff, ws, e_cap, t_cap, a_cap, n_groups, deg_bound, staging, id_c,
                 id_a, id_swap, id_undir, cell_offsets, id3_reduce_ca, id3_expand_ba, state, static_cast<hipStream_t>(stream));
}

extern "C" int gn_pbc_layout(const int32_t* N, const int32_t* n_atoms, int n_mol, int a_cap, int a_tot, int32_t* mol_off,
                             int32_t* atom_mol, int64_t* batch_seg, int64_t* N_pad, float* mask, int32_t* state, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_mol <= 0 || a_cap < n_mol || a_tot < a_cap) return (int)hipErrorInvalidValue;
  // (layout_cap.h; no bound on one structure's size, no adjacency offsets)
  hipLaunchKernelGGL(cap_layout_scan_kernel, dim3(1), dim3(1024), 0, st, N, n_atoms, n_mol, a_cap, a_tot, 0, mol_off, (int32_t*)nullptr,
                     N_pad, state);
  hipLaunchKernelGGL(cap_layout_atoms_kernel, dim3(gn_cdiv(a_tot, 256)), dim3(256), 0, st, mol_off, n_mol, a_cap, a_tot, state,
                     atom_mol, batch_seg, mask);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_pbc_index_padded_tv(const float* R, const float* cell, const uint8_t* pbc, const int32_t* mol_off,
                                      const int32_t* atom_mol, int n_mol, double cutoff, void* ws, int e_cap, int t_cap, int a_cap,
                                      int n_groups, int deg_bound, int32_t* staging, int32_t* id_c, int32_t* id_a, int32_t* id_swap,
                                      int32_t* id_undir, int32_t* cell_offsets, int32_t* id3_reduce_ca, int32_t* id3_expand_ba,
                                      int32_t* state, void* stream) {
  if (n_mol <= 0 || a_cap < n_mol || e_cap <= 0 || t_cap <= 0 || n_groups <= 0 || (e_cap & 1) || (t_cap & 1))
    return (int)hipErrorInvalidValue;
  // a_cap atom rows; the cell check runs over the n_mol real structures (row n_mol of pbc is never read), atoms of structure
  // n_mol are the fillers
  return pbx_run(R, cell, pbc, mol_off, atom_mol, n_mol, a_cap, n_mol, 1, cutoff, ws, e_cap, t_cap, a_cap, n_groups, deg_bound,
                 staging, id_c, id_a, id_swap, id_undir, cell_offsets, id3_reduce_ca, id3_expand_ba, state,
                 static_cast<hipStream_t>(stream));
}
