// Radial head of the first-order (inference) forward of GemNet-T in one kernel, and its adjoint in one kernel.
//
// Per edge the model needs the NR Bessel functions and the S NR spherical-Bessel radial functions of the distance only as
// the operands of four tiny frozen projections (gemnet.py:158-204: mlp_rbf3, mlp_rbf_h, mlp_rbf_out (NR -> 16) and the
// circular-basis down projection mlp_cbf3, (S, NR) -> (S, 16), efficient.py:41-57).  geometry.hip writes the 48 values
// (rbf, rad3) and four GEMM launches read them again: 160 outputs of a 6-term dot product each, in tile kernels built for
// K >= 32.  Here the 48 values stay in LDS and the lanes that evaluated them also project them, so rad3 never exists;
// the adjoint folds the four transposed projections and the sum of the rbf gradients into the derivative kernel.
//
// Basis values: the same f64 functions and the same cast as edge_basis_fwd_kernel (bit-identical).  Projections: one fp32
// FMA chain over r per output, in the order r = 0..NR-1.  An edge's results depend on nothing but that edge (no grid-
// stride, fixed lane roles, fixed reduction order), so runs at another E or grid give the same rows bit for bit.
//
// Weights arrive concatenated, wcat (10, NR, 16): rows k = 0, 1, 2 hold W_rbf3^T, W_rbf_h^T, W_rbf_out^T and k = 3 + s
// holds W_cbf3[s] — [k][r][i] is contiguous in i for the forward (lane = column) and for the adjoint (lane = (k, r) row).
#include "common.h"
#include "basis_math.h"

namespace {

constexpr int RH_NR = 6, RH_S = 7, RH_NI = 16;
constexpr int RH_NFUN = RH_NR + RH_S * RH_NR;   // 48 basis functions per edge
constexpr int RH_NOUT = 3 + RH_S;               // 10 projected rows of 16 columns per edge

// 16 lanes per edge, three f64 evaluations each (j = sub, sub + 16, sub + 32), 16 edges per block.  48 lanes with one
// evaluation each measured the same stand-alone and 0.8 % slower in the step (profiles/radial_head_timeline.txt).
constexpr int RH_LPE = 16, RH_BLOCK = 256, RH_EPB = RH_BLOCK / RH_LPE;

__device__ __forceinline__ float rh_distance(const float* __restrict__ R, int c, int a, float& vx, float& vy, float& vz) {
  const float* Ra = R + 3 * (int64_t)a;
  const float* Rc = R + 3 * (int64_t)c;
  // same f32 arithmetic as edge_basis_fwd_kernel: V = Ra - Rc; D = sqrt(sum(V^2))
  vx = Ra[0] - Rc[0]; vy = Ra[1] - Rc[1]; vz = Ra[2] - Rc[2];
  return sqrtf(vx * vx + vy * vy + vz * vz);
}

__global__ void __launch_bounds__(RH_BLOCK)
radial_head_fwd_kernel(const float* __restrict__ R, const int32_t* __restrict__ id_c, const int32_t* __restrict__ id_a,
                       const float* __restrict__ freq, const float* __restrict__ z, const double* __restrict__ nrm,
                       const float* __restrict__ wcat, float* __restrict__ rbf, float* __restrict__ rbf3,
                       float* __restrict__ rbf_h, float* __restrict__ rbf_out, float* __restrict__ rbf_W1, int64_t E,
                       double cutoff, int p) {
  __shared__ float vals[RH_EPB][RH_NFUN];
  const int el = threadIdx.x / RH_LPE, sub = threadIdx.x % RH_LPE;
  const int64_t e = blockIdx.x * (int64_t)RH_EPB + el;
  const bool ok = e < E;
  if (ok) {
    float vx, vy, vz;
    const float d = rh_distance(R, id_c[e], id_a[e], vx, vy, vz);
    for (int j = sub; j < RH_NFUN; j += RH_LPE) {
      float v;
      if (j < RH_NR) {
        v = (float)bessel_rbf_eval((double)d, (double)freq[j], cutoff, p, 0, 0);
        rbf[e * RH_NR + j] = v;
      } else {
        const int lr = j - RH_NR;
        v = (float)sph_radial_eval((double)d, (double)z[lr], nrm[lr], lr / RH_NR, cutoff, p, 0);
      }
      vals[el][j] = v;
    }
  }
  __syncthreads();
  if (!ok) return;
  // lane -> column i of the ten output rows: out[k][i] = sum_r b_k[r] wcat[k][r][i]
  static_assert(RH_LPE == RH_NI, "one lane per output column");
  const int i = sub;
#pragma unroll
  for (int k = 0; k < RH_NOUT; ++k) {
    const float* b = k < 3 ? vals[el] : vals[el] + RH_NR + (k - 3) * RH_NR;
    const float* w = wcat + k * (RH_NR * RH_NI) + i;
    float acc = b[0] * w[0];
#pragma unroll
    for (int r = 1; r < RH_NR; ++r) acc = fmaf(b[r], w[r * RH_NI], acc);
    if (k >= 3) rbf_W1[(e * RH_S + (k - 3)) * RH_NI + i] = acc;
    else (k == 0 ? rbf3 : (k == 1 ? rbf_h : rbf_out))[e * RH_NI + i] = acc;
  }
}

// sum_i w[i] g[i], i < 16, in the order i = 0..15 (both rows 16-byte aligned)
__device__ __forceinline__ float rh_dot16(const float* __restrict__ w, const float* __restrict__ g) {
  float acc = 0.f;
#pragma unroll
  for (int q = 0; q < RH_NI / 4; ++q) {
    const float4 a = reinterpret_cast<const float4*>(w)[q];
    const float4 b = reinterpret_cast<const float4*>(g)[q];
    acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc); acc = fmaf(a.z, b.z, acc); acc = fmaf(a.w, b.w, acc);
  }
  return acc;
}

// W[e,:] = (sum_j c_j f_j'(d) / d) V  with  c_r = g_rbf[r] + sum_i (W_rbf3[i,r] g_rbf3[i] + W_rbf_h[i,r] g_rbf_h[i] +
// W_rbf_out[i,r] g_rbf_out[i])  and  c_{s,r} = sum_i W_cbf3[s,r,i] g_rbf_W1[s,i]  (any cotangent may be null).
// Lane j forms c_j (fp32), multiplies with the f64 derivative, and the first lane of the edge adds the 16 partial sums
// in lane order.
__global__ void __launch_bounds__(RH_BLOCK)
radial_head_bwd_kernel(const float* __restrict__ g_rbf, const float* __restrict__ g_rbf3, const float* __restrict__ g_rbf_h,
                       const float* __restrict__ g_rbf_out, const float* __restrict__ g_rbf_W1, const float* __restrict__ R,
                       const int32_t* __restrict__ id_c, const int32_t* __restrict__ id_a, const float* __restrict__ freq,
                       const float* __restrict__ z, const double* __restrict__ nrm, const float* __restrict__ wcat,
                       float* __restrict__ Wout, int64_t E, double cutoff, int p) {
  __shared__ double part[RH_EPB][RH_LPE];
  const int el = threadIdx.x / RH_LPE, sub = threadIdx.x % RH_LPE;
  const int64_t e = blockIdx.x * (int64_t)RH_EPB + el;
  const bool ok = e < E;
  float vx = 0.f, vy = 0.f, vz = 0.f, d = 1.f;
  double g = 0.0;
  if (ok) {
    d = rh_distance(R, id_c[e], id_a[e], vx, vy, vz);
    const bool any_rbf = g_rbf || g_rbf3 || g_rbf_h || g_rbf_out;
    for (int j = sub; j < RH_NFUN; j += RH_LPE) {
      if (j < RH_NR) {
        if (!any_rbf) continue;
        float c = g_rbf ? g_rbf[e * RH_NR + j] : 0.f;
        if (g_rbf3) c += rh_dot16(wcat + (0 * RH_NR + j) * RH_NI, g_rbf3 + e * RH_NI);
        if (g_rbf_h) c += rh_dot16(wcat + (1 * RH_NR + j) * RH_NI, g_rbf_h + e * RH_NI);
        if (g_rbf_out) c += rh_dot16(wcat + (2 * RH_NR + j) * RH_NI, g_rbf_out + e * RH_NI);
        g += (double)c * bessel_rbf_eval((double)d, (double)freq[j], cutoff, p, 1, 0);
      } else if (g_rbf_W1) {
        const int lr = j - RH_NR, s = lr / RH_NR;
        const float c = rh_dot16(wcat + (3 * RH_NR + lr) * RH_NI, g_rbf_W1 + (e * RH_S + s) * RH_NI);
        g += (double)c * sph_radial_eval((double)d, (double)z[lr], nrm[lr], s, cutoff, p, 1);
      }
    }
  }
  part[el][sub] = g;
  __syncthreads();
  if (ok && sub == 0) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < RH_LPE; ++q) t += part[el][q];
    const float sc = (float)(t / (double)d);
    Wout[3 * e] = sc * vx; Wout[3 * e + 1] = sc * vy; Wout[3 * e + 2] = sc * vz;
  }
}

// ---- the edge embedding inside the two launches --------------------------------------------------------------------------
// m0 = ssilu(rbf W_r + (emb W_c^T)[Z[id_c]] + (emb W_a^T)[Z[id_a]]) (embedding_block.py:60-75 with frozen weights): the six
// rbf values are in `vals`, the two atom terms are rows of 93-row tables, so the Dense is a 6-term FMA chain per output and
// two row reads.  Order of gemm_smallk + its epilogue: fma over r = 0..5 from zero, + T_c row, + T_a row, activation — m0 is
// bit-identical to that launch.  d0 = ssilu'(z0) comes from the same sigmoid (gn_ssilu_pair) and replaces the stored z0.
// A lane owns the float4 columns sub and sub + 16 of the 32 of a row: the 16 lanes of an edge store 256 contiguous bytes.
constexpr int RH_NE = 128, RH_NE4 = RH_NE / 4;
constexpr int RH_PITCH4 = RH_NE4 + 1;        // LDS row pitch of the adjoint's staged rows, in float4

__global__ void __launch_bounds__(RH_BLOCK)
radial_head_emb_fwd_kernel(const float* __restrict__ R, const int32_t* __restrict__ id_c, const int32_t* __restrict__ id_a,
                           const float* __restrict__ freq, const float* __restrict__ z, const double* __restrict__ nrm,
                           const float* __restrict__ wcat, const int32_t* __restrict__ zrow, const float4* __restrict__ Tc,
                           const float4* __restrict__ Ta, const float4* __restrict__ Wr, float* __restrict__ rbf,
                           float* __restrict__ rbf3, float* __restrict__ rbf_h, float* __restrict__ rbf_out,
                           float* __restrict__ rbf_W1, float4* __restrict__ m0, float4* __restrict__ d0, int64_t E,
                           double cutoff, int p) {
  __shared__ float vals[RH_EPB][RH_NFUN];
  __shared__ float4 wr[RH_NR * RH_NE4];
  const int el = threadIdx.x / RH_LPE, sub = threadIdx.x % RH_LPE;
  const int64_t e = blockIdx.x * (int64_t)RH_EPB + el;
  const bool ok = e < E;
  if (threadIdx.x < RH_NR * RH_NE4) wr[threadIdx.x] = Wr[threadIdx.x];
  int c = 0, a = 0;
  if (ok) {
    float vx, vy, vz;
    c = id_c[e]; a = id_a[e];
    const float d = rh_distance(R, c, a, vx, vy, vz);
    for (int j = sub; j < RH_NFUN; j += RH_LPE) {
      float v;
      if (j < RH_NR) {
        v = (float)bessel_rbf_eval((double)d, (double)freq[j], cutoff, p, 0, 0);
        if (rbf) rbf[e * RH_NR + j] = v;
      } else {
        const int lr = j - RH_NR;
        v = (float)sph_radial_eval((double)d, (double)z[lr], nrm[lr], lr / RH_NR, cutoff, p, 0);
      }
      vals[el][j] = v;
    }
  }
  __syncthreads();
  if (!ok) return;
  const int i = sub;
#pragma unroll
  for (int k = 0; k < RH_NOUT; ++k) {
    const float* b = k < 3 ? vals[el] : vals[el] + RH_NR + (k - 3) * RH_NR;
    const float* w = wcat + k * (RH_NR * RH_NI) + i;
    float acc = b[0] * w[0];
#pragma unroll
    for (int r = 1; r < RH_NR; ++r) acc = fmaf(b[r], w[r * RH_NI], acc);
    if (k >= 3) rbf_W1[(e * RH_S + (k - 3)) * RH_NI + i] = acc;
    else (k == 0 ? rbf3 : (k == 1 ? rbf_h : rbf_out))[e * RH_NI + i] = acc;
  }
  const float4* tc = Tc + (int64_t)zrow[c] * RH_NE4;
  const float4* ta = Ta + (int64_t)zrow[a] * RH_NE4;
  const float* b = vals[el];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int q = sub + h * RH_LPE;
    const float4 g1 = tc[q], g2 = ta[q];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int r = 0; r < RH_NR; ++r) {
      const float4 w = wr[r * RH_NE4 + q];
      v.x = fmaf(b[r], w.x, v.x); v.y = fmaf(b[r], w.y, v.y); v.z = fmaf(b[r], w.z, v.z); v.w = fmaf(b[r], w.w, v.w);
    }
    v.x += g1.x; v.y += g1.y; v.z += g1.z; v.w += g1.w;
    v.x += g2.x; v.y += g2.y; v.z += g2.z; v.w += g2.w;
    float4 dv;
    gn_ssilu_pair(v.x, v.x, dv.x); gn_ssilu_pair(v.y, v.y, dv.y); gn_ssilu_pair(v.z, v.z, dv.z); gn_ssilu_pair(v.w, v.w, dv.w);
    m0[e * RH_NE4 + q] = v;
    d0[e * RH_NE4 + q] = dv;
  }
}

// radial_head_bwd_kernel with the adjoint of the embedding Dense folded in: lane j < NR adds
// sum_i (ga[e,i] + gb[e,i]) d0[e,i] W_r[j,i] (fp32, i = 0..127 in order) to its c_j.  The 16 lanes of an edge stage the row
// t = (ga + gb) d0 in LDS once (float4, coalesced); the six lanes then read it as broadcasts.  With ga = gb = null nothing
// of this runs and W is the old kernel's, bit for bit.
__global__ void __launch_bounds__(RH_BLOCK)
radial_head_emb_bwd_kernel(const float* __restrict__ g_rbf, const float* __restrict__ g_rbf3, const float* __restrict__ g_rbf_h,
                           const float* __restrict__ g_rbf_out, const float* __restrict__ g_rbf_W1,
                           const float4* __restrict__ ga, const float4* __restrict__ gb, const float4* __restrict__ d0,
                           const float4* __restrict__ Wr, const float* __restrict__ R, const int32_t* __restrict__ id_c,
                           const int32_t* __restrict__ id_a, const float* __restrict__ freq, const float* __restrict__ z,
                           const double* __restrict__ nrm, const float* __restrict__ wcat, float* __restrict__ Wout, int64_t E,
                           double cutoff, int p) {
  __shared__ double part[RH_EPB][RH_LPE];
  __shared__ float4 trow[RH_EPB][RH_PITCH4];
  __shared__ float4 wr[RH_NR][RH_PITCH4];
  const int el = threadIdx.x / RH_LPE, sub = threadIdx.x % RH_LPE;
  const int64_t e = blockIdx.x * (int64_t)RH_EPB + el;
  const bool ok = e < E;
  const bool emb = ga || gb;
  if (emb) {
    if (threadIdx.x < RH_NR * RH_NE4) wr[threadIdx.x / RH_NE4][threadIdx.x % RH_NE4] = Wr[threadIdx.x];
    if (ok) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int q = sub + h * RH_LPE;
        float4 g = ga ? ga[e * RH_NE4 + q] : gb[e * RH_NE4 + q];
        if (ga && gb) { const float4 u = gb[e * RH_NE4 + q]; g.x += u.x; g.y += u.y; g.z += u.z; g.w += u.w; }
        const float4 dv = d0[e * RH_NE4 + q];
        trow[el][q] = make_float4(g.x * dv.x, g.y * dv.y, g.z * dv.z, g.w * dv.w);
      }
    }
    __syncthreads();
  }
  float vx = 0.f, vy = 0.f, vz = 0.f, d = 1.f;
  double g = 0.0;
  if (ok) {
    d = rh_distance(R, id_c[e], id_a[e], vx, vy, vz);
    const bool any_rbf = g_rbf || g_rbf3 || g_rbf_h || g_rbf_out || emb;
    for (int j = sub; j < RH_NFUN; j += RH_LPE) {
      if (j < RH_NR) {
        if (!any_rbf) continue;
        float c = g_rbf ? g_rbf[e * RH_NR + j] : 0.f;
        if (g_rbf3) c += rh_dot16(wcat + (0 * RH_NR + j) * RH_NI, g_rbf3 + e * RH_NI);
        if (g_rbf_h) c += rh_dot16(wcat + (1 * RH_NR + j) * RH_NI, g_rbf_h + e * RH_NI);
        if (g_rbf_out) c += rh_dot16(wcat + (2 * RH_NR + j) * RH_NI, g_rbf_out + e * RH_NI);
        if (emb) {
          float s = 0.f;
#pragma unroll 8
          for (int q = 0; q < RH_NE4; ++q) {
            const float4 t = trow[el][q], w = wr[j][q];
            s = fmaf(t.x, w.x, s); s = fmaf(t.y, w.y, s); s = fmaf(t.z, w.z, s); s = fmaf(t.w, w.w, s);
          }
          c += s;
        }
        g += (double)c * bessel_rbf_eval((double)d, (double)freq[j], cutoff, p, 1, 0);
      } else if (g_rbf_W1) {
        const int lr = j - RH_NR, s = lr / RH_NR;
        const float c = rh_dot16(wcat + (3 * RH_NR + lr) * RH_NI, g_rbf_W1 + (e * RH_S + s) * RH_NI);
        g += (double)c * sph_radial_eval((double)d, (double)z[lr], nrm[lr], s, cutoff, p, 1);
      }
    }
  }
  part[el][sub] = g;
  __syncthreads();
  if (ok && sub == 0) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < RH_LPE; ++q) t += part[el][q];
    const float sc = (float)(t / (double)d);
    Wout[3 * e] = sc * vx; Wout[3 * e + 1] = sc * vy; Wout[3 * e + 2] = sc * vz;
  }
}

inline bool rh_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline bool rh_shape_ok(int64_t E, int NR, int S, int NI, int p) {
  // one block per 16 edges: the grid must fit 2^31 - 1 blocks
  return NR == RH_NR && S == RH_S && NI == RH_NI && p >= 2 && E < ((int64_t)1 << 34);
}

}  // namespace

extern "C" int gn_radial_head_fwd_f32(const float* R, const int32_t* id_c, const int32_t* id_a, const float* freq,
                                      const float* z, const double* nrm, const float* wcat, float* rbf, float* rbf3,
                                      float* rbf_h, float* rbf_out, float* rbf_W1, int64_t E, int NR, int S, int NI,
                                      float cutoff, int p, void* stream) {
  if (E <= 0) return 0;
  if (!rh_shape_ok(E, NR, S, NI, p)) return (int)hipErrorInvalidValue;
  if (!R || !id_c || !id_a || !freq || !z || !nrm || !wcat || !rbf || !rbf3 || !rbf_h || !rbf_out || !rbf_W1)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(radial_head_fwd_kernel, dim3((unsigned)((E + RH_EPB - 1) / RH_EPB)), dim3(RH_BLOCK), 0,
                     static_cast<hipStream_t>(stream), R, id_c, id_a, freq, z, nrm, wcat, rbf, rbf3, rbf_h, rbf_out, rbf_W1, E,
                     (double)cutoff, p);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_radial_head_emb_fwd_f32(const float* R, const int32_t* id_c, const int32_t* id_a, const float* freq,
                                          const float* z, const double* nrm, const float* wcat, const int32_t* zrow,
                                          const float* Tc, const float* Ta, const float* Wr, float* rbf, float* rbf3,
                                          float* rbf_h, float* rbf_out, float* rbf_W1, float* m0, float* d0, int64_t E,
                                          int NR, int S, int NI, int NE, float cutoff, int p, void* stream) {
  if (E <= 0) return 0;
  if (!rh_shape_ok(E, NR, S, NI, p) || NE != RH_NE) return (int)hipErrorInvalidValue;
  if (!R || !id_c || !id_a || !freq || !z || !nrm || !wcat || !zrow || !Tc || !Ta || !Wr || !rbf3 || !rbf_h || !rbf_out ||
      !rbf_W1 || !m0 || !d0)
    return (int)hipErrorInvalidValue;
  // table rows, W_r and the (E,128) outputs move as float4
  if (!rh_aligned(Tc) || !rh_aligned(Ta) || !rh_aligned(Wr) || !rh_aligned(m0) || !rh_aligned(d0))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(radial_head_emb_fwd_kernel, dim3((unsigned)((E + RH_EPB - 1) / RH_EPB)), dim3(RH_BLOCK), 0,
                     static_cast<hipStream_t>(stream), R, id_c, id_a, freq, z, nrm, wcat, zrow,
                     reinterpret_cast<const float4*>(Tc), reinterpret_cast<const float4*>(Ta),
                     reinterpret_cast<const float4*>(Wr), rbf, rbf3, rbf_h, rbf_out, rbf_W1, reinterpret_cast<float4*>(m0),
                     reinterpret_cast<float4*>(d0), E, (double)cutoff, p);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_radial_head_emb_bwd_f32(const float* g_rbf, const float* g_rbf3, const float* g_rbf_h, const float* g_rbf_out,
                                          const float* g_rbf_W1, const float* ga, const float* gb, const float* d0,
                                          const float* Wr, const float* R, const int32_t* id_c, const int32_t* id_a,
                                          const float* freq, const float* z, const double* nrm, const float* wcat, float* W,
                                          int64_t E, int NR, int S, int NI, int NE, float cutoff, int p, void* stream) {
  if (E <= 0) return 0;
  if (!rh_shape_ok(E, NR, S, NI, p) || NE != RH_NE) return (int)hipErrorInvalidValue;
  if (!R || !id_c || !id_a || !freq || !z || !nrm || !wcat || !W) return (int)hipErrorInvalidValue;
  if ((ga || gb) && (!d0 || !Wr)) return (int)hipErrorInvalidValue;
  if (!rh_aligned(wcat) || !rh_aligned(g_rbf3) || !rh_aligned(g_rbf_h) || !rh_aligned(g_rbf_out) || !rh_aligned(g_rbf_W1) ||
      !rh_aligned(ga) || !rh_aligned(gb) || !rh_aligned(d0) || !rh_aligned(Wr))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(radial_head_emb_bwd_kernel, dim3((unsigned)((E + RH_EPB - 1) / RH_EPB)), dim3(RH_BLOCK), 0,
                     static_cast<hipStream_t>(stream), g_rbf, g_rbf3, g_rbf_h, g_rbf_out, g_rbf_W1,
                     reinterpret_cast<const float4*>(ga), reinterpret_cast<const float4*>(gb),
                     reinterpret_cast<const float4*>(d0), reinterpret_cast<const float4*>(Wr), R, id_c, id_a, freq, z, nrm, wcat,
                     W, E, (double)cutoff, p);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_radial_head_bwd_f32(const float* g_rbf, const float* g_rbf3, const float* g_rbf_h, const float* g_rbf_out,
                                      const float* g_rbf_W1, const float* R, const int32_t* id_c, const int32_t* id_a,
                                      const float* freq, const float* z, const double* nrm, const float* wcat, float* W,
                                      int64_t E, int NR, int S, int NI, float cutoff, int p, void* stream) {
  if (E <= 0) return 0;
  if (!rh_shape_ok(E, NR, S, NI, p)) return (int)hipErrorInvalidValue;
  if (!R || !id_c || !id_a || !freq || !z || !nrm || !wcat || !W) return (int)hipErrorInvalidValue;
  // the 16-column rows are read as float4 (null cotangents are skipped)
  if (!rh_aligned(wcat) || !rh_aligned(g_rbf3) || !rh_aligned(g_rbf_h) || !rh_aligned(g_rbf_out) || !rh_aligned(g_rbf_W1))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(radial_head_bwd_kernel, dim3((unsigned)((E + RH_EPB - 1) / RH_EPB)), dim3(RH_BLOCK), 0,
                     static_cast<hipStream_t>(stream), g_rbf, g_rbf3, g_rbf_h, g_rbf_out, g_rbf_W1, R, id_c, id_a, freq, z, nrm, wcat,
                     W, E, (double)cutoff, p);
  GN_LAUNCH_CHECK();
  return 0;
}
