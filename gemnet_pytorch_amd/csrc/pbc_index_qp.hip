// Capacity form of the periodic quadruplet index build (gn_pbc_qindex_padded): the arrays of csrc/pbc.hip + csrc/pbc_index_q.hip
// — same canonical order, same float32 distance arithmetic — built with NO read-back into capacity-sized arrays, followed by
// the pad rows of gemnet_pytorch_amd/padded.py (quadruplet layout), so that index build + GemNet-Q are ONE capturable graph: the
// periodic twin of gn_index_gpu_padded_q (index_gpu.hip), on top of the kernels of gn_pbc_index_padded_t (pbc_index_cap.h).
// Positions and cell are read from device memory at replay time.
//
// Interaction edges: the wave-per-atom pair search of pbc_index_cap.h with int_cutoff gives the canonical forward pairs
// (i, j >= i, n) — every pair tested ONCE, on its forward form — and the list of an atom a ordered by (b, n) is then the in-edge
// list of that pair list by (source atom, offset): sources b < a are the swapped twins of the forward pairs (b, a, n') with
// n = -n' (descending forward id), b == a the swapped self-images followed by the forward ones, b > a the forward pairs of a.
// The same walk over the EDGE list gives the in-edges by (source atom, cell offset) of the intermediate triplets (in_src) and
// the position of every edge in the list of its target (pos_src).  One wavefront per atom, lanes over the source atoms, a wave
// scan keeping the order: no sort, no atomics.
// Quadruplets: one wavefront per reduce edge over the forward edges of its structure, twice (ids e, then e + H), the interaction
// edges a - b of a candidate looked up by bisection, survivors placed with a wave scan (pbq_quad_kernel of pbc_index_q.hip with
// the counts read from device memory); the count pass is the same body.
//
// Order of the launches and what protects the arrays:
//   cell (cutoff), cell (int_cutoff), merge of the two verdicts
//   -> pairs<count> -> scan -> pairs<fill> (edges into STAGING; returns when 2H > e_cap)
//   -> pairs<count> -> scan -> pairs<fill> (interaction pairs into the WORKSPACE; returns when 2Hint > eint_cap)
//   -> in<count> x 2 -> scan x 2 -> in<list> (ascending: triplets) -> src<edges> (in_src, pos_src) -> src<int> (interaction edges
//   into STAGING) -> cnt3, cnt_intm -> scan x 3 -> quad<count> -> scan
//   -> decide (one block: every count against its capacity, the padding rules, the in-degree bounds; writes state[])
//   -> trip, intm, quad<fill> (straight into the model's arrays, only when state[3] == 0)
//   -> commit (edges and interaction edges from staging + the pad rows of all five families, ditto).
// Every kernel that indexes with a count checks the capacity that bounds it first; counts are int64 throughout.  After an error
// nothing the model reads is written, so the arrays keep the previous step's valid contents (gn_index_poison_f32 then turns the
// outputs into NaN).
#include "common.h"
#include "pbc_index_cap.h"

namespace {

// both pair searches stop on either verdict (bit 32 is judged for each cutoff: the larger one decides)
__global__ void pbqp_cellerr_kernel(int32_t* __restrict__ cellerr, int32_t* __restrict__ cellerr_i) {
  if (blockIdx.x || threadIdx.x) return;
  const int e = cellerr[0] | cellerr_i[0];
  cellerr[0] = e;
  cellerr_i[0] = e;
}

// one wave per atom a: the in-edges of a in a forward pair list (off, s_c, s_offs; H = off[A] pairs, 2H <= cap) ordered by
// (source atom, offset lexicographic), written at ptr[a].  kInt == false: the edge ids (in_src) and the position of every edge
// in the list of its target (pos_src).  kInt == true: the interaction edges themselves, (int_a, int_b, int_offs).
template <bool kInt>
__global__ __launch_bounds__(256) void pbqp_src_kernel(const int32_t* __restrict__ mol_off, const int32_t* __restrict__ atom_mol,
                                                       int A, const int64_t* __restrict__ off, const int32_t* __restrict__ s_c,
                                                       const int32_t* __restrict__ s_offs, int cap,
                                                       const int32_t* __restrict__ cellerr, const int64_t* __restrict__ ptr,
                                                       int32_t* __restrict__ in_src, int32_t* __restrict__ pos_src,
                                                       int32_t* __restrict__ int_a, int32_t* __restrict__ int_b,
                                                       int32_t* __restrict__ int_offs) {
  const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (a >= A) return;                                         // (wave-uniform)
  const int64_t H = off[A];
  if (cellerr[0] || 2 * H > (int64_t)cap) return;             // the pair list was not written
  const int a0 = mol_off[atom_mol[a]];
  const int64_t p0 = ptr[a], p1 = ptr[a + 1];
  // p: position in the output, e: forward id of the pair, src: the other atom
  auto put = [&](int64_t p, int64_t e, bool swapped, int src) {
    if (p >= p1 || p >= (int64_t)cap) return;                 // (cannot happen: the in-degrees counted the same pairs)
    if (kInt) {
      int_a[p] = a;
      int_b[p] = src;
#pragma unroll
      for (int k = 0; k < 3; ++k) int_offs[3 * p + k] = swapped ? -s_offs[3 * e + k] : s_offs[3 * e + k];
    } else {
      const int64_t id = swapped ? e + H : e;
      in_src[p] = (int32_t)id;
      pos_src[id] = (int32_t)(p - p0);
    }
  };
  int64_t k = p0;
  for (int i0 = a0; i0 <= a; i0 += 64) {
    const int i = i0 + lane;
    int64_t lo = 0, hi = 0;
    if (i <= a) src_range(s_c, off[i], off[i + 1], a, lo, hi);
    const int c = (int)(hi - lo);
    const int incl = wave_scan_incl(c, lane);
    for (int q = 0; q < c; ++q) put(k + (incl - c) + q, hi - 1 - q, true, i);
    k += __shfl(incl, 63, 64);
  }
  const int64_t f0 = off[a], nf = off[a + 1] - f0;            // the forward pairs of a: self-images first, then j > a
  for (int64_t q = lane; q < nf; q += 64) put(k + q, f0 + q, false, s_c[f0 + q]);
}

// what every kernel in front of `decide` asks before it reads the two staged lists
__device__ __forceinline__ bool lists_fit(const int32_t* __restrict__ cellerr, int64_t H, int64_t Hi, int e_cap, int eint_cap) {
  return !cellerr[0] && 2 * H <= (int64_t)e_cap && 2 * Hi <= (int64_t)eint_cap;
}

// intermediate triplets per interaction edge over the eint_cap rows; rows behind Eint (and every row of a build that does not
// fit) count zero
__global__ void pbqp_cnt_intm_kernel(const int32_t* __restrict__ int_a, const int32_t* __restrict__ int_b,
                                     const int64_t* __restrict__ deg, const int64_t* __restrict__ off,
                                     const int64_t* __restrict__ offi, int A, int e_cap, int eint_cap,
                                     const int32_t* __restrict__ cellerr, int64_t* __restrict__ cnt_ca,
                                     int64_t* __restrict__ cnt_db) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= eint_cap) return;
  const bool ok = lists_fit(cellerr, off[A], offi[A], e_cap, eint_cap) && k < 2 * offi[A];
  cnt_ca[k] = ok ? deg[int_a[k]] : 0;
  cnt_db[k] = ok ? deg[int_b[k]] : 0;
}

struct QuadIn {
  const int32_t *mol_off, *atom_mol, *id_a, *id_c, *offs, *int_b, *int_offs, *pos_src, *cellerr;
  const int64_t *off, *offi, *off_int, *off_ca, *off_db;
};
struct QuadOutP {
  int32_t *red_ca, *exp_db, *red_cab, *exp_abd;
};

// one wavefront per reduce edge r = (c -> a, n_c) of the e_cap rows: count its quadruplets (kFill == false; zero behind E and
// for a build that does not fit) or write them (kFill == true; only after `decide` accepted the step)
template <bool kFill>
__global__ __launch_bounds__(256) void pbqp_quad_kernel(QuadIn in, int A, int e_cap, int eint_cap, int q_cap,
                                                        int64_t* __restrict__ cnt4, const int64_t* __restrict__ off4,
                                                        const int32_t* __restrict__ state, QuadOutP out) {
  const int64_t r = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= (int64_t)e_cap) return;                            // (wave-uniform)
  const int64_t H = in.off[A];
  if (kFill) {
    if (state[3] || r >= 2 * H) return;
  } else if (!lists_fit(in.cellerr, H, in.offi[A], e_cap, eint_cap) || r >= 2 * H) {
    if (lane == 0) cnt4[r] = 0;
    return;
  }
  const int a = in.id_a[r], c = in.id_c[r];
  const int nc0 = in.offs[3 * r], nc1 = in.offs[3 * r + 1], nc2 = in.offs[3 * r + 2];
  const int m = in.atom_mol[a];
  const int64_t f0 = in.off[in.mol_off[m]], f1 = in.off[in.mol_off[m + 1]];   // the forward edges of a's structure
  const int64_t i0 = in.off_int[a], i1 = in.off_int[a + 1];
  const int pr = kFill ? in.pos_src[r] : 0;
  const int64_t o0 = kFill ? off4[r] : 0;
  int64_t o = o0;
  for (int phase = 0; phase < 2; ++phase) {
    for (int64_t e0 = f0; e0 < f1; e0 += 64) {
      const int64_t e = e0 + lane;
      int cnt = 0, b = 0, d = 0, nd0 = 0, nd1 = 0, nd2 = 0;
      int64_t x = 0, klo = 0, khi = 0;
      if (e < f1) {
        x = phase ? e + H : e;                                // expand edge d -> b
        b = in.id_a[x];
        d = in.id_c[x];
        nd0 = in.offs[3 * x]; nd1 = in.offs[3 * x + 1]; nd2 = in.offs[3 * x + 2];
        int_range(in.int_b, i0, i1, b, klo, khi);
      }
      // (c, n_c) != (b, n_b), (a, 0) != (d, n_b + n_db), (c, n_c) != (d, n_b + n_db)
      auto keep = [&](int64_t k) {
        const int nb0 = in.int_offs[3 * k], nb1 = in.int_offs[3 * k + 1], nb2 = in.int_offs[3 * k + 2];
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
        const int px = in.pos_src[x];
        for (int64_t k = klo; k < khi; ++k) {
          if (!keep(k)) continue;
          if (w < (int64_t)q_cap) {                           // (always: Q <= q_cap was decided)
            out.red_ca[w] = (int32_t)r;
            out.exp_db[w] = (int32_t)x;
            out.red_cab[w] = (int32_t)(in.off_ca[k] + pr);
            out.exp_abd[w] = (int32_t)(in.off_db[k] + px);
          }
          ++w;
        }
      }
      o += __shfl(incl, 63, 64);
    }
  }
  if (!kFill && lane == 0) cnt4[r] = o;
}

struct QCapsP { int e, t, eint, i, q, a, G, deg_bound; };

// one block: all counts against their capacities, the padding rules of padded.py (quadruplet layout), the in-degree bounds;
// state[] as documented in include/gemnet_hip.h
__global__ __launch_bounds__(256) void pbqp_decide_kernel(const int64_t* __restrict__ off, const int64_t* __restrict__ offi,
                                                          const int64_t* __restrict__ off3, const int64_t* __restrict__ off_ca,
                                                          const int64_t* __restrict__ off4, const int64_t* __restrict__ deg,
                                                          int A, QCapsP k, const int32_t* __restrict__ cellerr,
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
  int64_t E = 0, T = 0, Ei = 0, I = 0, Q = 0;
  if (!err) {
    E = 2 * off[A];
    Ei = 2 * offi[A];
    if (E > (int64_t)k.e) err |= 1;
    if (Ei > (int64_t)k.eint) err |= 256;
  }
  if (!err) {                                                 // (the counts below are zero when a list was not written)
    T = off3[k.e];
    I = off_ca[k.eint];
    Q = off4[k.e];
    if (T > (int64_t)k.t) err |= 2;
    if (I > (int64_t)k.i) err |= 512;
    if (Q > (int64_t)k.q) err |= 1024;
  }
  if (!err) {
    const int64_t ep = k.e - E, tp = k.t - T, eintp = k.eint - Ei, ip = k.i - I, qp = k.q - Q;
    const int bound = k.deg_bound > 2 ? k.deg_bound : 2;
    if ((tp > 0 && ep < 6) || (tp & 1)) err |= 4;
    if (((tp || ip || qp) && ep < 6) || (ip && eintp < 1) || (qp && ip < 1)) err |= 2048;
    // largest in-degree of a dummy atom (padded.py, pad_in_degree of a quadruplet runner): a unit of six puts two pad edges on
    // atom a and two on atom b of its group; the units cycle over the groups
    const int64_t units = (ep + 5) / 6;
    if (2 * ((units + k.G - 1) / k.G) > bound) err |= 8;
    if (mx > (int64_t)k.deg_bound) err |= 16;
  }
  auto clip = [](int64_t v) { return (int32_t)(v > 0x7fffffff ? 0x7fffffff : v); };
  state[0] |= err;
  state[1] = clip(E);
  state[2] = clip(T);
  state[3] = err;
  state[4] = clip(mx);
  state[5] = clip(Ei);
  state[6] = clip(I);
  state[7] = clip(Q);
}

// one thread per interaction edge k = (b -> a): its two runs of intermediate triplets, the in-edges of a and of b by source
__global__ void pbqp_intm_kernel(const int32_t* __restrict__ int_a, const int32_t* __restrict__ int_b, int eint_cap,
                                 const int64_t* __restrict__ in_ptr, const int32_t* __restrict__ in_src,
                                 const int64_t* __restrict__ off_ca, const int64_t* __restrict__ off_db, int i_cap,
                                 const int32_t* __restrict__ state, int32_t* __restrict__ red_intm_ca,
                                 int32_t* __restrict__ red_intm_ab, int32_t* __restrict__ exp_intm_db,
                                 int32_t* __restrict__ exp_intm_ab) {
  if (state[3]) return;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= eint_cap || k >= state[5]) return;
  const int a = int_a[k], b = int_b[k];
  int64_t q = off_ca[k];
  for (int64_t p = in_ptr[a]; p < in_ptr[a + 1] && q < (int64_t)i_cap; ++p, ++q) { red_intm_ca[q] = in_src[p]; red_intm_ab[q] = k; }
  q = off_db[k];
  for (int64_t p = in_ptr[b]; p < in_ptr[b + 1] && q < (int64_t)i_cap; ++p, ++q) { exp_intm_db[q] = in_src[p]; exp_intm_ab[q] = k; }
}

struct PadQP {
  const int32_t *s_c, *s_a, *s_swap, *s_undir, *s_offs, *s_int_a, *s_int_b, *s_int_offs;
  int32_t *id_c, *id_a, *id_swap, *id_undir, *offs, *red3, *exp3, *int_a, *int_b, *int_offs, *intm_ca, *intm_db, *intm_red_ab,
      *intm_exp_ab, *q_red_ca, *q_exp_db, *q_red_cab, *q_exp_abd;
};

// edges and interaction edges from staging, then the pad rows of padded.py (quadruplet layout: _pad_edges(quad), _pad_triplets
// (quad), _pad_int_edges, _pad_intm, _pad_quads; offsets 0)
__global__ void pbqp_commit_pad_kernel(PadQP p, QCapsP k, const int32_t* __restrict__ state) {
  if (state[3]) return;
  const int64_t E = state[1], T = state[2], Ei = state[5], I = state[6], Q = state[7];
  const int64_t ep = k.e - E, tp = k.t - T, eintp = k.eint - Ei, ip = k.i - I, qp = k.q - Q;
  const int G = k.G;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  // edges: copy + pad (units of six: b->a, a->b, c->a, a->c, d->b, b->d over groups of four dummy atoms)
  for (int64_t i = tid; i < k.e; i += nth) {
    if (i < E) {
      p.id_c[i] = p.s_c[i]; p.id_a[i] = p.s_a[i]; p.id_swap[i] = p.s_swap[i]; p.id_undir[i] = p.s_undir[i];
      p.offs[3 * i] = p.s_offs[3 * i]; p.offs[3 * i + 1] = p.s_offs[3 * i + 1]; p.offs[3 * i + 2] = p.s_offs[3 * i + 2];
    } else {
      const int64_t kk = i - E, pair = kk >> 1;
      const int rev = (int)(kk & 1), typ = (int)(pair % 3), grp = (int)((pair / 3) % G);
      const int a = k.a + 4 * grp;
      const int src = typ == 2 ? a + 3 : a + 1 + typ, dst = typ == 2 ? a + 1 : a;
      p.id_c[i] = rev ? dst : src;
      p.id_a[i] = rev ? src : dst;
      p.id_swap[i] = (int32_t)(E + (kk ^ 1));
      p.id_undir[i] = (int32_t)(E / 2 + pair);
      p.offs[3 * i] = 0; p.offs[3 * i + 1] = 0; p.offs[3 * i + 2] = 0;
    }
  }
  // pad triplets: the forward edges b->a, c->a (offsets 0 and 2) of the complete units
  {
    const int64_t nf = 2 * (ep / 6), den = tp > 1 ? tp : 1;
    for (int64_t j = tid; j < tp; j += nth) {
      const int64_t sidx = (j * nf) / den, u = sidx >> 1, w = sidx & 1;
      p.red3[T + j] = (int32_t)(E + 6 * u + 2 * w);
      p.exp3[T + j] = (int32_t)(E + 6 * u + 2 * (1 - w));
    }
  }
  // interaction edges: copy + pad (pairs b->a, a->b cycling over the groups)
  for (int64_t i = tid; i < k.eint; i += nth) {
    if (i < Ei) {
      p.int_a[i] = p.s_int_a[i]; p.int_b[i] = p.s_int_b[i];
      p.int_offs[3 * i] = p.s_int_offs[3 * i]; p.int_offs[3 * i + 1] = p.s_int_offs[3 * i + 1];
      p.int_offs[3 * i + 2] = p.s_int_offs[3 * i + 2];
    } else {
      const int64_t kk = i - Ei, pr = kk >> 1;
      const int rev = (int)(kk & 1), a = k.a + 4 * (int)(pr % G);
      p.int_b[i] = rev ? a : a + 1;
      p.int_a[i] = rev ? a + 1 : a;
      p.int_offs[3 * i] = 0; p.int_offs[3 * i + 1] = 0; p.int_offs[3 * i + 2] = 0;
    }
  }
  // pad intermediate triplets / quadruplets
  const int64_t n_ab = (eintp + 1) / 2, n_units = ep / 6 > 1 ? ep / 6 : 1, iden = ip > 1 ? ip : 1;
  auto intm_unit = [&](int64_t i, int64_t& pp) {     // unit of pad intermediate triplet i, and its interaction-edge pair
    pp = (i * n_ab) / iden;
    const int64_t g = pp % G;
    return g < n_units ? g : pp % n_units;
  };
  for (int64_t i = tid; i < ip; i += nth) {
    int64_t pp;
    const int64_t u = intm_unit(i, pp);
    p.intm_ca[I + i] = (int32_t)(E + 6 * u + 2);
    p.intm_db[I + i] = (int32_t)(E + 6 * u + 4);
    p.intm_red_ab[I + i] = (int32_t)(Ei + 2 * pp);
    p.intm_exp_ab[I + i] = (int32_t)(Ei + 2 * pp);
  }
  {
    const int64_t qden = qp > 1 ? qp : 1, imod = ip > 1 ? ip : 1;
    for (int64_t q = tid; q < qp; q += nth) {
      const int64_t u = (q * n_units) / qden, im = q % imod;
      int64_t pp;
      const int64_t ui = intm_unit(im, pp);
      p.q_red_ca[Q + q] = (int32_t)(E + 6 * u + 2);
      p.q_exp_abd[Q + q] = (int32_t)(I + im);
      p.q_red_cab[Q + q] = (int32_t)(I + im);
      p.q_exp_db[Q + q] = (int32_t)(E + 6 * ui + 4);
    }
  }
}

inline size_t al64(size_t x) { return (x + 63) & ~(size_t)63; }

struct pbqp_ws {
  double *geo, *geo_i;
  int64_t *cnt, *off, *cnti, *offi, *deg, *in_ptr, *ideg, *off_int, *cnt3, *off3, *cnt4, *off4, *cnt_ca, *off_ca, *cnt_db, *off_db;
  int32_t *in_edge, *in_src, *pos_src, *p_a, *p_c, *p_undir, *p_swap, *p_offs, *cellerr, *cellerr_i;
};

size_t pbqp_layout(char* base, int A, int e_cap, int eint_cap, pbqp_ws* w) {
  size_t o = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += al64(bytes); return p; };
  const size_t a = (size_t)A, e = (size_t)e_cap, ei = (size_t)eint_cap;
  w->geo = (double*)take(8 * (size_t)kGeo * a);               // B <= A structures
  w->geo_i = (double*)take(8 * (size_t)kGeo * a);
  w->cnt = (int64_t*)take(8 * a);
  w->off = (int64_t*)take(8 * (a + 1));
  w->cnti = (int64_t*)take(8 * a);
  w->offi = (int64_t*)take(8 * (a + 1));
  w->deg = (int64_t*)take(8 * a);
  w->in_ptr = (int64_t*)take(8 * (a + 1));
  w->ideg = (int64_t*)take(8 * a);
  w->off_int = (int64_t*)take(8 * (a + 1));
  w->cnt3 = (int64_t*)take(8 * e);
  w->off3 = (int64_t*)take(8 * (e + 1));
  w->cnt4 = (int64_t*)take(8 * e);
  w->off4 = (int64_t*)take(8 * (e + 1));
  w->cnt_ca = (int64_t*)take(8 * ei);
  w->off_ca = (int64_t*)take(8 * (ei + 1));
  w->cnt_db = (int64_t*)take(8 * ei);
  w->off_db = (int64_t*)take(8 * (ei + 1));
  w->in_edge = (int32_t*)take(4 * e);
  w->in_src = (int32_t*)take(4 * e);
  w->pos_src = (int32_t*)take(4 * e);
  w->p_a = (int32_t*)take(4 * ei);
  w->p_c = (int32_t*)take(4 * ei);
  w->p_undir = (int32_t*)take(4 * ei);
  w->p_swap = (int32_t*)take(4 * ei);
  w->p_offs = (int32_t*)take(12 * ei);
  w->cellerr = (int32_t*)take(64);
  w->cellerr_i = (int32_t*)take(64);
  return o;
}

}  // namespace

extern "C" int64_t gn_pbc_qindex_ws_bytes(int A, int e_cap, int eint_cap, void* /*stream: nothing is launched*/) {
  pbqp_ws w;
  return (int64_t)pbqp_layout(nullptr, A > 0 ? A : 0, e_cap > 0 ? e_cap : 0, eint_cap > 0 ? eint_cap : 0, &w);
}

extern "C" int gn_pbc_qindex_padded(const float* R, const float* cell, const uint8_t* pbc, const int32_t* mol_off,
                                    const int32_t* atom_mol, int B, int A, double cutoff, double int_cutoff, void* ws, int e_cap,
                                    int t_cap, int eint_cap, int i_cap, int q_cap, int a_cap, int n_groups, int deg_bound,
                                    int32_t* staging, int32_t* const* arrays, int32_t* state, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (A <= 0 || B <= 0 || B > A || n_groups <= 0 || e_cap <= 0 || t_cap <= 0 || eint_cap <= 0 || i_cap <= 0 || q_cap <= 0 ||
      (e_cap & 1) || (t_cap & 1) || a_cap < A || !arrays)
    return (int)hipErrorInvalidValue;
  pbqp_ws w;
  pbqp_layout((char*)ws, A, e_cap, eint_cap, &w);
  const size_t e = (size_t)e_cap, ei = (size_t)eint_cap;
  int32_t *s_a = staging, *s_c = staging + e, *s_undir = staging + 2 * e, *s_swap = staging + 3 * e, *s_offs = staging + 4 * e,
          *s_int_a = staging + 7 * e, *s_int_b = staging + 7 * e + ei, *s_int_offs = staging + 7 * e + 2 * ei;
  // arrays: id_c, id_a, id_swap, id_undir, id3_reduce_ca, id3_expand_ba, id4_int_a, id4_int_b, id4_reduce_intm_ca,
  //         id4_expand_intm_db, id4_reduce_intm_ab, id4_expand_intm_ab, id4_reduce_ca, id4_expand_db, id4_reduce_cab, id4_expand_abd,
  //         cell_offsets, int_cell_offsets
  const dim3 gw(gn_cdiv(A, 4)), b256(256), one(1), ge(gn_cdiv(e_cap, 256)), gei(gn_cdiv(eint_cap, 256)), gq(gn_cdiv(e_cap, 4));
  hipLaunchKernelGGL(pbx_cell_kernel, one, dim3(64), 0, st, cell, pbc, B, cutoff, w.geo, w.cellerr);
  hipLaunchKernelGGL(pbx_cell_kernel, one, dim3(64), 0, st, cell, pbc, B, int_cutoff, w.geo_i, w.cellerr_i);
  hipLaunchKernelGGL(pbqp_cellerr_kernel, one, dim3(64), 0, st, w.cellerr, w.cellerr_i);
  // the edge list (staging) and the interaction pairs (workspace): count -> scan -> fill
  hipLaunchKernelGGL((pbx_pairs_kernel<false>), gw, b256, 0, st, R, cell, pbc, mol_off, atom_mol, A, (float)cutoff, w.geo, w.cellerr,
                     w.cnt, w.off, e_cap, s_a, s_c, s_undir, s_swap, s_offs, -1);
  hipLaunchKernelGGL(pbc_scan_kernel, one, dim3(1024), 0, st, w.cnt, w.off, (int64_t)A);
  hipLaunchKernelGGL((pbx_pairs_kernel<true>), gw, b256, 0, st, R, cell, pbc, mol_off, atom_mol, A, (float)cutoff, w.geo, w.cellerr,
                     w.cnt, w.off, e_cap, s_a, s_c, s_undir, s_swap, s_offs, -1);
  hipLaunchKernelGGL((pbx_pairs_kernel<false>), gw, b256, 0, st, R, cell, pbc, mol_off, atom_mol, A, (float)int_cutoff, w.geo_i,
                     w.cellerr_i, w.cnti, w.offi, eint_cap, w.p_a, w.p_c, w.p_undir, w.p_swap, w.p_offs, -1);
  hipLaunchKernelGGL(pbc_scan_kernel, one, dim3(1024), 0, st, w.cnti, w.offi, (int64_t)A);
  hipLaunchKernelGGL((pbx_pairs_kernel<true>), gw, b256, 0, st, R, cell, pbc, mol_off, atom_mol, A, (float)int_cutoff, w.geo_i,
                     w.cellerr_i, w.cnti, w.offi, eint_cap, w.p_a, w.p_c, w.p_undir, w.p_swap, w.p_offs, -1);
  GN_LAUNCH_CHECK();
  // in-degrees of both lists, the three in-edge orders
  hipLaunchKernelGGL((pbx_in_kernel<false>), gw, b256, 0, st, mol_off, atom_mol, A, w.off, s_c, e_cap, w.cellerr, w.deg, w.in_ptr,
                     w.in_edge, -1);
  hipLaunchKernelGGL((pbx_in_kernel<false>), gw, b256, 0, st, mol_off, atom_mol, A, w.offi, w.p_c, eint_cap, w.cellerr_i, w.ideg,
                     w.off_int, (int32_t*)nullptr, -1);
  hipLaunchKernelGGL(pbc_scan_kernel, one, dim3(1024), 0, st, w.deg, w.in_ptr, (int64_t)A);
  hipLaunchKernelGGL(pbc_scan_kernel, one, dim3(1024), 0, st, w.ideg, w.off_int, (int64_t)A);
  hipLaunchKernelGGL((pbx_in_kernel<true>), gw, b256, 0, st, mol_off, atom_mol, A, w.off, s_c, e_cap, w.cellerr, w.deg, w.in_ptr,
                     w.in_edge, -1);
  hipLaunchKernelGGL((pbqp_src_kernel<false>), gw, b256, 0, st, mol_off, atom_mol, A, w.off, s_c, s_offs, e_cap, w.cellerr, w.in_ptr,
                     w.in_src, w.pos_src, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
  hipLaunchKernelGGL((pbqp_src_kernel<true>), gw, b256, 0, st, mol_off, atom_mol, A, w.offi, w.p_c, w.p_offs, eint_cap, w.cellerr_i,
                     w.off_int, (int32_t*)nullptr, (int32_t*)nullptr, s_int_a, s_int_b, s_int_offs);
  GN_LAUNCH_CHECK();
  // counts of the three large families
  hipLaunchKernelGGL(pbx_cnt3_kernel, ge, b256, 0, st, s_a, w.deg, w.off, A, e_cap, w.cellerr, w.cnt3);
  hipLaunchKernelGGL(pbqp_cnt_intm_kernel, gei, b256, 0, st, s_int_a, s_int_b, w.deg, w.off, w.offi, A, e_cap, eint_cap, w.cellerr,
                     w.cnt_ca, w.cnt_db);
  hipLaunchKernelGGL(pbc_scan_kernel, one, dim3(1024), 0, st, w.cnt3, w.off3, (int64_t)e_cap);
  hipLaunchKernelGGL(pbc_scan_kernel, one, dim3(1024), 0, st, w.cnt_ca, w.off_ca, (int64_t)eint_cap);
  hipLaunchKernelGGL(pbc_scan_kernel, one, dim3(1024), 0, st, w.cnt_db, w.off_db, (int64_t)eint_cap);
  const QuadIn qin{mol_off, atom_mol, s_a, s_c, s_offs, s_int_b, s_int_offs, w.pos_src, w.cellerr, w.off, w.offi, w.off_int, w.off_ca,
                   w.off_db};
  hipLaunchKernelGGL((pbqp_quad_kernel<false>), gq, b256, 0, st, qin, A, e_cap, eint_cap, q_cap, w.cnt4, w.off4,
                     (const int32_t*)state, QuadOutP{nullptr, nullptr, nullptr, nullptr});
  hipLaunchKernelGGL(pbc_scan_kernel, one, dim3(1024), 0, st, w.cnt4, w.off4, (int64_t)e_cap);
  GN_LAUNCH_CHECK();
  const QCapsP k{e_cap, t_cap, eint_cap, i_cap, q_cap, a_cap, n_groups, deg_bound};
  hipLaunchKernelGGL(pbqp_decide_kernel, one, b256, 0, st, w.off, w.offi, w.off3, w.off_ca, w.off4, w.deg, A, k, w.cellerr, state);
  // the writers of the large families: straight into the model's arrays, or nothing at all
  hipLaunchKernelGGL(pbx_trip_kernel, dim3(gn_cdiv((int64_t)e_cap * 16, 256)), b256, 0, st, s_a, w.off, A, w.in_ptr, w.in_edge,
                     w.off3, e_cap, t_cap, (const int32_t*)state, arrays[4], arrays[5]);
  hipLaunchKernelGGL(pbqp_intm_kernel, gei, b256, 0, st, s_int_a, s_int_b, eint_cap, w.in_ptr, w.in_src, w.off_ca, w.off_db, i_cap,
                     (const int32_t*)state, arrays[8], arrays[10], arrays[9], arrays[11]);
  hipLaunchKernelGGL((pbqp_quad_kernel<true>), gq, b256, 0, st, qin, A, e_cap, eint_cap, q_cap, (int64_t*)nullptr, w.off4,
                     (const int32_t*)state, QuadOutP{arrays[12], arrays[13], arrays[14], arrays[15]});
  GN_LAUNCH_CHECK();
  const PadQP p{s_c, s_a, s_swap, s_undir, s_offs, s_int_a, s_int_b, s_int_offs, arrays[0], arrays[1], arrays[2], arrays[3],
                arrays[16], arrays[4], arrays[5], arrays[6], arrays[7], arrays[17], arrays[8], arrays[9], arrays[10], arrays[11],
                arrays[12], arrays[13], arrays[14], arrays[15]};
  const int64_t work = [&] { int64_t m = e_cap; for (int64_t v : {(int64_t)t_cap, (int64_t)eint_cap, (int64_t)i_cap, (int64_t)q_cap}) m = v > m ? v : m; return m; }();
  hipLaunchKernelGGL(pbqp_commit_pad_kernel, dim3((unsigned)(gn_cdiv(work, 256) < 2048 ? gn_cdiv(work, 256) : 2048)), b256, 0, st, p, k,
                     (const int32_t*)state);
  GN_LAUNCH_CHECK();
  return 0;
}
