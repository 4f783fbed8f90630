// Force TRAINING of GemNet-Q on periodic batches (include/gemnet_hip.h, gn_angle_vec2_* / gn_quad_angles_vec_jvp_f32).
//
// A periodic GemNet-Q batch depends on positions and cell only through the edge vectors V (E,3) and the interaction-edge
// vectors Vint (n_int,3) (csrc/pbc_quad.hip), so the second-order graph of the training step — loss.backward() through
// G = -dE/dV and Gint = -dE/dVint, from which forces and stress are linear — needs the geometry of the quadruplet branch as
// twice-differentiable functions of (V, Vint):
//     a - b <- d angle   theta[t] = atan2(max(|u x v|, 1e-9), u.v),  u = U[iu[t]],  v = -W[iw[t]]   (gn_trip_basis_vec2_fwd_f32)
//                        as value / first adjoint / tangent kernel: the two-array twins of gn_angle_vec_* (csrc/pbc_train.hip),
//                        same arithmetic (the shared angle_adjoint<float> of geom_dual.h)
//     quadruplet angles  value and first adjoint are gn_quad_angles_vec_fwd_f32 / _bwd_f32 (csrc/pbc_quad.hip), unchanged; the
//                        tangent kernel here evaluates the SAME body as that first adjoint (quad_math.h, quad_angles_adj)
//                        with unit cotangents and dots the result with the tangent vectors, so adjoint and tangent take identical
//                        decisions at the degeneracies of a crystal: c - a - b collinear => dPhi = 0; a vanished rejection or a
//                        planar quadruplet => dTheta = 0.
// V and Vint are the private leaves the forces and the stress are taken from and never join a caller's graph, so no second-order
// terms with respect to the vectors exist here.  The distances of the interaction edges are gn_dist_vec_* on Vint and the
// (G, Gint) -> (F, S) adjoint is gn_pbc_force_stress_adj_f32 once per edge family.  One thread per triplet / quadruplet,
// grid-stride; per-triplet adjoint terms are reduced by the caller with the segmented sums of rows.hip — no atomics, fixed order.
#include "common.h"
#include "geom_dual.h"
// quad_math.h and geom_dual.h both call their three-vector V3 (a struct there, a template over the scalar type here): the
// quadruplet math gets a namespace of its own in this translation unit
namespace qm {
#include "quad_math.h"
}

namespace {

__device__ __forceinline__ V3<float> row3(const float* __restrict__ p, int64_t r, float s) {
  return {s * p[3 * r], s * p[3 * r + 1], s * p[3 * r + 2]};
}

__global__ void angle_vec2_fwd_kernel(const float* __restrict__ U, const int32_t* __restrict__ iu, const float* __restrict__ W,
                                      const int32_t* __restrict__ iw, float* __restrict__ theta, int64_t T) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    // on (u, -v) = (U[iu], W[iw]) as loaded: |u x v| = |u x (-v)| and u.v = -(u.(-v)) hold bit for bit, and the products of the
    // cross product are then rounded in the order of gn_angle_fwd_f32 on the same two vectors (with the sign folded into v the
    // compiler contracts the other product of each difference: 1 ulp apart on one row in ten) — without images theta is the
    // molecular kernel's, bit for bit
    const V3<float> u = row3(U, iu[t], 1.0f), nv = row3(W, iw[t], 1.0f);
    const V3<float> w = cross(u, nv);
    const float yn = sqrtf(dot(w, w));
    theta[t] = atan2f(yn < 1e-9f ? 1e-9f : yn, -dot(u, nv));
  }
}

// GU[t] = g dtheta/dU[iu[t]], GW[t] = g dtheta/dW[iw[t]]  (v = -W[iw[t]])
__global__ void angle_vec2_bwd_kernel(const float* __restrict__ g, const float* __restrict__ U, const int32_t* __restrict__ iu,
                                      const float* __restrict__ W, const int32_t* __restrict__ iw, float* __restrict__ GU,
                                      float* __restrict__ GW, int64_t T) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    const V3<float> u = row3(U, iu[t], 1.0f), v = row3(W, iw[t], -1.0f);
    V3<float> gu, gv;
    angle_adjoint<float>(u, v, g[t], gu, gv);
    GU[3 * t] = gu.x; GU[3 * t + 1] = gu.y; GU[3 * t + 2] = gu.z;
    GW[3 * t] = -gv.x; GW[3 * t + 1] = -gv.y; GW[3 * t + 2] = -gv.z;
  }
}

// thdot[t] = dtheta/du . tU[iu[t]] - dtheta/dv . tW[iw[t]]: the tangent of theta along (tU, tW), i.e. the cotangent of the
// incoming adjoint g in the double backward (the first adjoint is linear in g).  A null tangent array counts as zero.
__global__ void angle_vec2_jvp_kernel(const float* __restrict__ U, const int32_t* __restrict__ iu, const float* __restrict__ W,
                                      const int32_t* __restrict__ iw, const float* __restrict__ tU, const float* __restrict__ tW,
                                      float* __restrict__ thdot, int64_t T) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t ru = iu[t], rw = iw[t];
    const V3<float> u = row3(U, ru, 1.0f), v = row3(W, rw, -1.0f);
    const V3<float> zero = {0.f, 0.f, 0.f};
    const V3<float> du = tU ? row3(tU, ru, 1.0f) : zero, dv = tW ? row3(tW, rw, -1.0f) : zero;
    V3<float> g1u, g1v;
    angle_adjoint<float>(u, v, 1.0f, g1u, g1v);
    thdot[t] = dot(g1u, du) + dot(g1v, dv);
  }
}

__device__ __forceinline__ qm::V3 neg3(const float* p) { return {-p[0], -p[1], -p[2]}; }

// tang[q] = (dPhi_cab, dTheta_cabd, 0, 0) along (tV, tVint): quad_angles_jvp_kernel (geometry.hip) on uac = -V[ca],
// uab = -Vint[k], ubd = -V[db], k = intm_ab[abd[q]] (the index reads of quad_angles_vec_bwd_kernel).  Each angle's gradient is
// one evaluation of the first adjoint's body with a unit cotangent in its slot: 16 B written per quadruplet.
__global__ __launch_bounds__(256) void quad_angles_vec_jvp_kernel(const float* __restrict__ V, const float* __restrict__ Vint,
                                                                  const float* __restrict__ tV, const float* __restrict__ tVint,
                                                                  const int32_t* __restrict__ ca, const int32_t* __restrict__ db,
                                                                  const int32_t* __restrict__ abd,
                                                                  const int32_t* __restrict__ intm_ab, float4* __restrict__ tang,
                                                                  int64_t Q) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < Q; q += (int64_t)gridDim.x * 256) {
    const int64_t eca = ca[q], edb = db[q], k = intm_ab[abd[q]];
    const qm::V3 uac = neg3(V + 3 * eca), uab = neg3(Vint + 3 * k), ubd = neg3(V + 3 * edb);
    const qm::V3 zero = {0.f, 0.f, 0.f};
    const qm::V3 dac = tV ? neg3(tV + 3 * eca) : zero, dab = tVint ? neg3(tVint + 3 * k) : zero,
                 dbd = tV ? neg3(tV + 3 * edb) : zero;
    qm::V3 g_ac, g_ab, g_bd;
    qm::quad_angles_adj(uac, uab, ubd, 1.0f, 0.0f, g_ac, g_ab, g_bd);
    const float dphi = qm::dot(g_ac, dac) + qm::dot(g_ab, dab) + qm::dot(g_bd, dbd);
    qm::quad_angles_adj(uac, uab, ubd, 0.0f, 1.0f, g_ac, g_ab, g_bd);
    const float dth = qm::dot(g_ac, dac) + qm::dot(g_ab, dab) + qm::dot(g_bd, dbd);
    tang[q] = make_float4(dphi, dth, 0.f, 0.f);
  }
}

inline int grid_t(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 65535 ? 65535 : b));
}

inline int grid_q(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace

extern "C" int gn_angle_vec2_fwd_f32(const float* U, const int32_t* iu, const float* W, const int32_t* iw, float* theta, int64_t T,
                                     void* stream) {
  if (T <= 0) return 0;
  hipLaunchKernelGGL(angle_vec2_fwd_kernel, dim3(grid_t(T)), dim3(256), 0, static_cast<hipStream_t>(stream), U, iu, W, iw, theta,
                     T);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_angle_vec2_bwd_f32(const float* g, const float* U, const int32_t* iu, const float* W, const int32_t* iw,
                                     float* GU, float* GW, int64_t T, void* stream) {
  if (T <= 0) return 0;
  hipLaunchKernelGGL(angle_vec2_bwd_kernel, dim3(grid_t(T)), dim3(256), 0, static_cast<hipStream_t>(stream), g, U, iu, W, iw, GU,
                     GW, T);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_angle_vec2_jvp_f32(const float* U, const int32_t* iu, const float* W, const int32_t* iw, const float* tU,
                                     const float* tW, float* thdot, int64_t T, void* stream) {
  if (T <= 0) return 0;
  hipLaunchKernelGGL(angle_vec2_jvp_kernel, dim3(grid_t(T)), dim3(256), 0, static_cast<hipStream_t>(stream), U, iu, W, iw, tU, tW,
                     thdot, T);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_quad_angles_vec_jvp_f32(const float* V, const float* Vint, const float* tV, const float* tVint,
                                          const int32_t* q_ca, const int32_t* q_db, const int32_t* q_abd, const int32_t* intm_ab,
                                          float* tang, int64_t Q, void* stream) {
  if (Q <= 0) return 0;
  if ((reinterpret_cast<uintptr_t>(tang) & 15u) != 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(quad_angles_vec_jvp_kernel, dim3(grid_q(Q)), dim3(256), 0, static_cast<hipStream_t>(stream), V, Vint, tV,
                     tVint, q_ca, q_db, q_abd, intm_ab, reinterpret_cast<float4*>(tang), Q);
  GN_LAUNCH_CHECK();
  return 0;
}
