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
#include "common.h"

namespace {

constexpr int kMaxImages = 64;        // pbc.MAX_IMAGES: images per axis and side
constexpr int kGeo = 16;              // doubles per structure: cof[9], det, w[3]

__device__ __forceinline__ bool lex_positive(int n0, int n1, int n2) {
  return n0 > 0 || (n0 == 0 && (n1 > 0 || (n1 == 0 && n2 > 0)));
}

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

// inclusive scan of one int per lane over the wave
__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
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
                                                        int32_t* __restrict__ s_offs) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= A) return;                                         // (wave-uniform: i is the wave's atom)
  if (cellerr[0]) {
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

// single-block exclusive scan of n int64; out[n] = total (pbc_scan_kernel of pbc.hip)
__global__ __launch_bounds__(1024) void pbx_scan_kernel(const int64_t* __restrict__ in, int64_t* __restrict__ out, int64_t n) {
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

// one wave per atom a: its in-degree (kList == false) or its incoming edges in ascending id — the forward edges of a, then the
// swapped twins of the forward edges (i, a, n), i <= a, lanes over i and a wave scan keeping ascending i (= ascending id)
template <bool kList>
__global__ __launch_bounds__(256) void pbx_in_kernel(const int32_t* __restrict__ mol_off, const int32_t* __restrict__ atom_mol,
                                                     int A, const int64_t* __restrict__ off, const int32_t* __restrict__ s_c,
                                                     int e_cap, const int32_t* __restrict__ cellerr, int64_t* __restrict__ deg,
                                                     const int64_t* __restrict__ in_ptr, int32_t* __restrict__ in_edge) {
  const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (a >= A) return;
  const int64_t H = off[A];
  if (cellerr[0] || 2 * H > (int64_t)e_cap) {                // the staging arrays were not written
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
                                                         int32_t* __restrict__ state) {
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

extern "C" int gn_pbc_index_padded_t(const float* R, const float* cell, const uint8_t* pbc, const int32_t* mol_off,
                                     const int32_t* atom_mol, int B, int A, double cutoff, void* ws, int e_cap, int t_cap,
                                     int a_cap, int n_groups, int deg_bound, int32_t* staging, int32_t* id_c, int32_t* id_a,
                                     int32_t* id_swap, int32_t* id_undir, int32_t* cell_offsets, int32_t* id3_reduce_ca,
                                     int32_t* id3_expand_ba, int32_t* state, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (A <= 0 || B <= 0 || B > A || e_cap <= 0 || t_cap <= 0 || n_groups <= 0 || (e_cap & 1) || (t_cap & 1) || a_cap < A)
    return (int)hipErrorInvalidValue;
  pbx_ws w;
  pbx_layout((char*)ws, A, e_cap, &w);
  int32_t *s_a = staging, *s_c = staging + e_cap, *s_undir = staging + 2 * (size_t)e_cap, *s_swap = staging + 3 * (size_t)e_cap,
          *s_offs = staging + 4 * (size_t)e_cap;
  const dim3 gw(gn_cdiv(A, 4)), b256(256), one(1);
  hipLaunchKernelGGL(pbx_cell_kernel, one, dim3(64), 0, st, cell, pbc, B, cutoff, w.geo, w.cellerr);
  hipLaunchKernelGGL((pbx_pairs_kernel<false>), gw, b256, 0, st, R, cell, pbc, mol_off, atom_mol, A, (float)cutoff, w.geo, w.cellerr,
                     w.cnt, w.off, e_cap, s_a, s_c, s_undir, s_swap, s_offs);
  hipLaunchKernelGGL(pbx_scan_kernel, one, dim3(1024), 0, st, w.cnt, w.off, (int64_t)A);
  hipLaunchKernelGGL((pbx_pairs_kernel<true>), gw, b256, 0, st, R, cell, pbc, mol_off, atom_mol, A, (float)cutoff, w.geo, w.cellerr,
                     w.cnt, w.off, e_cap, s_a, s_c, s_undir, s_swap, s_offs);
  GN_LAUNCH_CHECK();
  hipLaunchKernelGGL((pbx_in_kernel<false>), gw, b256, 0, st, mol_off, atom_mol, A, w.off, s_c, e_cap, w.cellerr, w.deg, w.in_ptr,
                     w.in_edge);
  hipLaunchKernelGGL(pbx_scan_kernel, one, dim3(1024), 0, st, w.deg, w.in_ptr, (int64_t)A);
  hipLaunchKernelGGL((pbx_in_kernel<true>), gw, b256, 0, st, mol_off, atom_mol, A, w.off, s_c, e_cap, w.cellerr, w.deg, w.in_ptr,
                     w.in_edge);
  hipLaunchKernelGGL(pbx_cnt3_kernel, dim3(gn_cdiv(e_cap, 256)), b256, 0, st, s_a, w.deg, w.off, A, e_cap, w.cellerr, w.cnt3);
  hipLaunchKernelGGL(pbx_scan_kernel, one, dim3(1024), 0, st, w.cnt3, w.off3, (int64_t)e_cap);
  GN_LAUNCH_CHECK();
  hipLaunchKernelGGL(pbx_decide_kernel, one, b256, 0, st, w.off, w.off3, w.deg, A, e_cap, t_cap, n_groups, deg_bound, w.cellerr,
                     state);
  hipLaunchKernelGGL(pbx_trip_kernel, dim3(gn_cdiv((int64_t)e_cap * 16, 256)), b256, 0, st, s_a, w.off, A, w.in_ptr, w.in_edge,
                     w.off3, e_cap, t_cap, state, id3_reduce_ca, id3_expand_ba);
  PadP p{s_c, s_a, s_swap, s_undir, s_offs, id_c, id_a, id_swap, id_undir, cell_offsets, id3_reduce_ca, id3_expand_ba};
  const int64_t work = e_cap > t_cap ? e_cap : t_cap;
  hipLaunchKernelGGL(pbx_commit_pad_kernel, dim3((unsigned)(gn_cdiv(work, 256) < 2048 ? gn_cdiv(work, 256) : 2048)), b256, 0, st, p,
                     e_cap, t_cap, a_cap, n_groups, state);
  GN_LAUNCH_CHECK();
  return 0;
}
