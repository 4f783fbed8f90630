// Force TRAINING on periodic batches (include/gemnet_hip.h, gn_dist_vec_* / gn_angle_vec_* / gn_pbc_force_stress_adj_f32).
//
// A periodic batch depends on positions and cell only through the edge vectors V (E,3) (csrc/pbc.hip), so the second-order
// graph of the training step — loss.backward() through G = -dE/dV, from which forces and stress are linear — needs the
// distances and triplet angles as twice-differentiable functions of V, and the adjoint of the (G -> F, S) map:
//     distance   D[e]     = |V[e]|
//     angle      theta[t] = atan2(max(|u x v|, 1e-9), u.v),  u = -V[red[t]],  v = -V[exp[t]]   (gn_trip_basis_vec_fwd_f32)
// each as value / first adjoint / tangent kernel, the twins of geometry2.hip on V instead of on atom pairs (same arithmetic,
// the angle adjoint is the shared template of geom_dual.h).  V never takes part in a caller's autograd graph, so no
// second-order terms w.r.t. V exist here.  One thread per edge / triplet, grid-stride; per-triplet terms are reduced per edge
// by gn_segsum_multi_f32 — no atomics, fixed order of addition.
#include "common.h"
#include "geom_dual.h"

namespace {

__global__ void dist_vec_fwd_kernel(const float* __restrict__ V, float* __restrict__ D, int64_t E) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const float vx = V[3 * e], vy = V[3 * e + 1], vz = V[3 * e + 2];
    D[e] = sqrtf(vx * vx + vy * vy + vz * vz);      // dist_fwd_kernel's arithmetic: sqrt(sum(V^2))
  }
}

// W[e] = gD[e] V[e] / |V[e]| = gD dD/dV
__global__ void dist_vec_bwd_kernel(const float* __restrict__ gD, const float* __restrict__ V, float* __restrict__ W, int64_t E) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const float vx = V[3 * e], vy = V[3 * e + 1], vz = V[3 * e + 2];
    const float sc = gD[e] / sqrtf(vx * vx + vy * vy + vz * vz);
    W[3 * e] = sc * vx; W[3 * e + 1] = sc * vy; W[3 * e + 2] = sc * vz;
  }
}

// Ddot[e] = vhat . tV[e]
__global__ void dist_vec_jvp_kernel(const float* __restrict__ V, const float* __restrict__ tV, float* __restrict__ Ddot,
                                    int64_t E) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const float vx = V[3 * e], vy = V[3 * e + 1], vz = V[3 * e + 2];
    const float id = 1.0f / sqrtf(vx * vx + vy * vy + vz * vz);
    Ddot[e] = (vx * id) * tV[3 * e] + (vy * id) * tV[3 * e + 1] + (vz * id) * tV[3 * e + 2];
  }
}

__device__ __forceinline__ void load_uv_vec(const float* __restrict__ V, int64_t r, int64_t x, V3<float>& u, V3<float>& v) {
  u = {-V[3 * r], -V[3 * r + 1], -V[3 * r + 2]};
  v = {-V[3 * x], -V[3 * x + 1], -V[3 * x + 2]};
}

__global__ void angle_vec_fwd_kernel(const float* __restrict__ V, const int32_t* __restrict__ red, const int32_t* __restrict__ exp,
                                     float* __restrict__ theta, int64_t T) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    V3<float> u, v;
    load_uv_vec(V, red[t], exp[t], u, v);
    const V3<float> w = cross(u, v);
    const float yn = sqrtf(dot(w, w));
    theta[t] = atan2f(yn < 1e-9f ? 1e-9f : yn, dot(u, v));
  }
}

// Gu[t] = g dtheta/du, Gv[t] = g dtheta/dv   (dE/dV = -segsum(Gu by reduce edge) - segsum(Gv by expand edge))
__global__ void angle_vec_bwd_kernel(const float* __restrict__ g, const float* __restrict__ V, const int32_t* __restrict__ red,
                                     const int32_t* __restrict__ exp, float* __restrict__ Gu, float* __restrict__ Gv, int64_t T) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    V3<float> u, v, gu, gv;
    load_uv_vec(V, red[t], exp[t], u, v);
    angle_adjoint<float>(u, v, g[t], gu, gv);
    Gu[3 * t] = gu.x; Gu[3 * t + 1] = gu.y; Gu[3 * t + 2] = gu.z;
    Gv[3 * t] = gv.x; Gv[3 * t + 1] = gv.y; Gv[3 * t + 2] = gv.z;
  }
}

// thdot[t] = dtheta/du . du + dtheta/dv . dv  with du = -tV[red[t]], dv = -tV[exp[t]]: the tangent of theta along tV, which is
// the cotangent of the incoming adjoint g in the double backward (the first adjoint is linear in g)
__global__ void angle_vec_jvp_kernel(const float* __restrict__ V, const float* __restrict__ tV, const int32_t* __restrict__ red,
                                     const int32_t* __restrict__ exp, float* __restrict__ thdot, int64_t T) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    V3<float> u, v, du, dv, g1u, g1v;
    load_uv_vec(V, red[t], exp[t], u, v);
    load_uv_vec(tV, red[t], exp[t], du, dv);
    angle_adjoint<float>(u, v, 1.0f, g1u, g1v);
    thdot[t] = dot(g1u, du) + dot(g1v, dv);
  }
}

// gG[e,j] = gF[id_a[e],j] - gF[id_c[e],j] + scale / |det cell_b| sum_i V[e,i] gS[b,i,j],  b = batch_seg[id_a[e]]: the adjoint of
// F = segsum(G, id_a) - segsum(G, id_c) and S[b] = scale / |det cell_b| sum_{e of b} V_e (x) G_e (pbc_stress_kernel: the same f64
// determinant) in one pass over the edges; gS may be null (a loss without a stress term).
__global__ void pbc_force_stress_adj_kernel(const float* __restrict__ gF, const float* __restrict__ gS, const float* __restrict__ V,
                                            const int32_t* __restrict__ id_c, const int32_t* __restrict__ id_a,
                                            const int32_t* __restrict__ batch_seg, const float* __restrict__ cell, float scale,
                                            float* __restrict__ gG, int64_t E) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = id_a[e], c = id_c[e];
    float o[3] = {gF[3 * a] - gF[3 * c], gF[3 * a + 1] - gF[3 * c + 1], gF[3 * a + 2] - gF[3 * c + 2]};
    if (gS) {
      const int64_t b = batch_seg[a];
      const float* C = cell + 9 * b;
      const double det = (double)C[0] * ((double)C[4] * C[8] - (double)C[5] * C[7]) -
                         (double)C[1] * ((double)C[3] * C[8] - (double)C[5] * C[6]) +
                         (double)C[2] * ((double)C[3] * C[7] - (double)C[4] * C[6]);
      const double k = (double)scale / fabs(det);
      const double v[3] = {V[3 * e], V[3 * e + 1], V[3 * e + 2]};
      const float* s = gS + 9 * b;
#pragma unroll
      for (int j = 0; j < 3; ++j) o[j] += (float)(k * (v[0] * s[j] + v[1] * s[3 + j] + v[2] * s[6 + j]));
    }
    gG[3 * e] = o[0]; gG[3 * e + 1] = o[1]; gG[3 * e + 2] = o[2];
  }
}

inline int grid_for_vec(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 65535 ? 65535 : b));
}

}  // namespace

extern "C" int gn_dist_vec_fwd_f32(const float* V, float* D, int64_t E, void* stream) {
  if (E <= 0) return 0;
  hipLaunchKernelGGL(dist_vec_fwd_kernel, dim3(grid_for_vec(E)), dim3(256), 0, static_cast<hipStream_t>(stream), V, D, E);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_dist_vec_bwd_f32(const float* gD, const float* V, float* W, int64_t E, void* stream) {
  if (E <= 0) return 0;
  hipLaunchKernelGGL(dist_vec_bwd_kernel, dim3(grid_for_vec(E)), dim3(256), 0, static_cast<hipStream_t>(stream), gD, V, W, E);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_dist_vec_jvp_f32(const float* V, const float* tV, float* Ddot, int64_t E, void* stream) {
  if (E <= 0) return 0;
  hipLaunchKernelGGL(dist_vec_jvp_kernel, dim3(grid_for_vec(E)), dim3(256), 0, static_cast<hipStream_t>(stream), V, tV, Ddot, E);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_angle_vec_fwd_f32(const float* V, const int32_t* red, const int32_t* exp, float* theta, int64_t T,
                                    void* stream) {
  if (T <= 0) return 0;
  hipLaunchKernelGGL(angle_vec_fwd_kernel, dim3(grid_for_vec(T)), dim3(256), 0, static_cast<hipStream_t>(stream), V, red, exp,
                     theta, T);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_angle_vec_bwd_f32(const float* g, const float* V, const int32_t* red, const int32_t* exp, float* Gu, float* Gv,
                                    int64_t T, void* stream) {
  if (T <= 0) return 0;
  hipLaunchKernelGGL(angle_vec_bwd_kernel, dim3(grid_for_vec(T)), dim3(256), 0, static_cast<hipStream_t>(stream), g, V, red, exp,
                     Gu, Gv, T);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_angle_vec_jvp_f32(const float* V, const float* tV, const float* g, const int32_t* red, const int32_t* exp,
                                    float* thdot, int64_t T, void* stream) {
  if (T <= 0) return 0;
  (void)g;      // (the slot of gn_angle_jvp_f32's g: only its second-order terms read it, and V has none)
  hipLaunchKernelGGL(angle_vec_jvp_kernel, dim3(grid_for_vec(T)), dim3(256), 0, static_cast<hipStream_t>(stream), V, tV, red, exp,
                     thdot, T);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_pbc_force_stress_adj_f32(const float* gF, const float* gS, const float* V, const int32_t* id_c,
                                           const int32_t* id_a, const int32_t* batch_seg, const float* cell, float scale,
                                           float* gG, int64_t E, void* stream) {
  if (E <= 0) return 0;
  hipLaunchKernelGGL(pbc_force_stress_adj_kernel, dim3(grid_for_vec(E)), dim3(256), 0, static_cast<hipStream_t>(stream), gF, gS, V,
                     id_c, id_a, batch_seg, cell, scale, gG, E);
  GN_LAUNCH_CHECK();
  return 0;
}
