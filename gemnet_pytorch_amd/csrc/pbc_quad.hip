// Periodic cells for GemNet-Q (first-order path): the quadruplet geometry on VECTORS.  A periodic batch reaches the positions
// only through the edge vectors V (E,3) (gn_pbc_edge_vec_f32 over id_c, id_a, cell_offsets) and the interaction-edge vectors
// Vint (n_int,3) (the same kernel over id4_int_b, id4_int_a, int_cell_offsets); for a quadruplet c -> a - b <- d with reduce
// edge ca, interaction edge k = (b -> a) and expand edge db the three difference vectors of quad_math.h are
//   uac = -V[ca],  uab = -Vint[k],  ubd = -V[db]
// (image-aware by construction: every vector carries its shift), and for an intermediate triplet a - b <- d the angle at b is
// between u = Vint[k] (b -> a) and v = -V[db] (b -> d).  k is read through the intermediate triplet: k = intm_ab[abd[q]].
// Every adjoint returns gradients with respect to the VECTORS, per triplet / quadruplet; the caller sums them onto vector
// rows with the segmented sums of rows.hip (fixed order, no atomics), and forces and stress follow from dE/dV and dE/dVint
// exactly as for GemNet-T (pbc.hip).  Same per-quadruplet math as the molecular kernels (geometry.hip), with the reference's clamp
// decision taken relative to the vectors' lengths (quad_math.h, *_rel): in a crystal collinear and planar quadruplets are exact.
#include "common.h"
#include "basis_math.h"
#include "quad_math.h"

namespace {

__device__ __forceinline__ V3 neg3(const float* p) { return {-p[0], -p[1], -p[2]}; }

// Y[t,l] = Y_l0(angle(u, v)), u = U[iu[t]], v = -W[iw[t]]
__global__ void trip_basis_vec2_fwd_kernel(const float* __restrict__ U, const int32_t* __restrict__ iu,
                                           const float* __restrict__ W, const int32_t* __restrict__ iw, float* __restrict__ Y,
                                           int64_t T, int S) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    const float th = angle_uv(v3(U + 3 * (int64_t)iu[t]), neg3(W + 3 * (int64_t)iw[t]));
    ylm0_row((double)th, S, 0, Y + t * S);
  }
}

// GU[t,:] = dE/dU[iu[t]], GW[t,:] = dE/dW[iw[t]] of triplet t given gY[t,:]
__global__ void trip_basis_vec2_bwd_kernel(const float* __restrict__ gY, const float* __restrict__ U,
                                           const int32_t* __restrict__ iu, const float* __restrict__ W,
                                           const int32_t* __restrict__ iw, float* __restrict__ GU, float* __restrict__ GW,
                                           int64_t T, int S) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    const V3 u = v3(U + 3 * (int64_t)iu[t]), v = neg3(W + 3 * (int64_t)iw[t]);
    const float th = angle_uv(u, v);
    float dY[8];
    ylm0_row((double)th, S, 1, dY);
    float gth = 0.f;
    for (int l = 0; l < S; ++l) gth += gY[t * S + l] * dY[l];
    V3 gu, gv;
    angle_uv_bwd(u, v, gth, gu, gv);
    GU[3 * t] = gu.x; GU[3 * t + 1] = gu.y; GU[3 * t + 2] = gu.z;
    GW[3 * t] = -gv.x; GW[3 * t + 1] = -gv.y; GW[3 * t + 2] = -gv.z;
  }
}

struct QuadIdx {
  const int32_t *ca, *db, *abd, *intm_ab;
};

__device__ __forceinline__ void quad_vectors(const float* __restrict__ V, const float* __restrict__ Vint, const QuadIdx& ix,
                                             int64_t q, V3& uac, V3& uab, V3& ubd) {
  uac = neg3(V + 3 * (int64_t)ix.ca[q]);
  uab = neg3(Vint + 3 * (int64_t)ix.intm_ab[ix.abd[q]]);
  ubd = neg3(V + 3 * (int64_t)ix.db[q]);
}

// Gc (Q,3) = dE/dV[ca]; Gbd (Q,8) = [dE/dVint[k] xyz, 0, dE/dV[db] xyz, 0]: the vectors are minus the difference vectors
__device__ __forceinline__ void quad_store(float* __restrict__ Gc, float* __restrict__ Gbd, int64_t q, V3 g_ac, V3 g_ab, V3 g_bd) {
  Gc[3 * q] = -g_ac.x; Gc[3 * q + 1] = -g_ac.y; Gc[3 * q + 2] = -g_ac.z;
  float4* __restrict__ row = reinterpret_cast<float4*>(Gbd + 8 * q);
  row[0] = make_float4(-g_ab.x, -g_ab.y, -g_ab.z, 0.f);
  row[1] = make_float4(-g_bd.x, -g_bd.y, -g_bd.z, 0.f);
}

// Y[q, :] = Y_lm(Phi_cab, Theta_cabd); rows through LDS, coalesced stores (quad_basis_fwd_kernel of geometry.hip)
__global__ __launch_bounds__(256) void quad_basis_vec_fwd_kernel(const float* __restrict__ V, const float* __restrict__ Vint,
                                                                 QuadIdx ix, float* __restrict__ Y, int64_t Q, int S) {
  extern __shared__ float rows[];   // [256][S*S]
  const int SS = S * S;
  for (int64_t q0 = (int64_t)blockIdx.x * 256; q0 < Q; q0 += (int64_t)gridDim.x * 256) {
    const int64_t q = q0 + threadIdx.x;
    if (q < Q) {
      V3 uac, uab, ubd;
      quad_vectors(V, Vint, ix, q, uac, uab, ubd);
      double sn, cs, s1, c1;
      quad_angles_sc(uac, uab, ubd, sn, cs, s1, c1);
      ylm_row_sc(sn, cs, s1, c1, S, rows + threadIdx.x * SS);
    }
    __syncthreads();
    const int64_t n = (Q - q0 < 256 ? Q - q0 : 256) * SS;
    float* __restrict__ dst = Y + q0 * SS;
    for (int64_t i = threadIdx.x; i < n; i += 256) dst[i] = rows[i];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void quad_basis_vec_bwd_kernel(const float* __restrict__ gY, const float* __restrict__ V,
                                                                 const float* __restrict__ Vint, QuadIdx ix,
                                                                 float* __restrict__ Gc, float* __restrict__ Gbd, int64_t Q,
                                                                 int S) {
  extern __shared__ float rows[];   // [256][S*S]
  const int SS = S * S;
  for (int64_t q0 = (int64_t)blockIdx.x * 256; q0 < Q; q0 += (int64_t)gridDim.x * 256) {
    const int64_t n = (Q - q0 < 256 ? Q - q0 : 256) * SS;
    const float* __restrict__ src = gY + q0 * SS;
    for (int64_t i = threadIdx.x; i < n; i += 256) rows[i] = src[i];
    __syncthreads();
    const int64_t q = q0 + threadIdx.x;
    if (q < Q) {
      V3 uac, uab, ubd;
      quad_vectors(V, Vint, ix, q, uac, uab, ubd);
      double sn, cs, s1, c1;
      quad_angles_sc(uac, uab, ubd, sn, cs, s1, c1);
      double g_first, g_second;   // d/d(polar angle = Phi_cab), d/d(azimuth = Theta_cabd)
      ylm_dot_grad_sc(sn, cs, s1, c1, S, rows + threadIdx.x * SS, g_first, g_second);
      V3 g_ac, g_ab, g_bd;
      quad_angles_adj(uac, uab, ubd, (float)g_first, (float)g_second, g_ac, g_ab, g_bd);
      quad_store(Gc, Gbd, q, g_ac, g_ab, g_bd);
    }
    __syncthreads();
  }
}

// angle form: ang[q] = (sin, cos) of Phi_cab and of Theta_cabd (quad_angles_fwd_kernel of geometry.hip)
__global__ __launch_bounds__(256) void quad_angles_vec_fwd_kernel(const float* __restrict__ V, const float* __restrict__ Vint,
                                                                  QuadIdx ix, float4* __restrict__ ang, int64_t Q) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < Q; q += (int64_t)gridDim.x * 256) {
    V3 uac, uab, ubd;
    quad_vectors(V, Vint, ix, q, uac, uab, ubd);
    double sn, cs, s1, c1;
    quad_angles_sc(uac, uab, ubd, sn, cs, s1, c1);
    ang[q] = make_float4((float)sn, (float)cs, (float)s1, (float)c1);
  }
}

// g_ang[q] = (dE/dPhi_cab, dE/dTheta_cabd, -, -)
__global__ __launch_bounds__(256) void quad_angles_vec_bwd_kernel(const float4* __restrict__ g_ang, const float* __restrict__ V,
                                                                  const float* __restrict__ Vint, QuadIdx ix,
                                                                  float* __restrict__ Gc, float* __restrict__ Gbd, int64_t Q) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < Q; q += (int64_t)gridDim.x * 256) {
    V3 uac, uab, ubd;
    quad_vectors(V, Vint, ix, q, uac, uab, ubd);
    const float4 g = g_ang[q];
    V3 g_ac, g_ab, g_bd;
    quad_angles_adj(uac, uab, ubd, g.x, g.y, g_ac, g_ab, g_bd);
    quad_store(Gc, Gbd, q, g_ac, g_ab, g_bd);
  }
}

inline int grid_q(int64_t n) {
  int64_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace

extern "C" int gn_trip_basis_vec2_fwd_f32(const float* U, const int32_t* iu, const float* W, const int32_t* iw, float* Y,
                                          int64_t T, int S, void* stream) {
  if (T <= 0) return 0;
  if (S < 1 || S > 8) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(trip_basis_vec2_fwd_kernel, dim3(grid_q(T)), dim3(256), 0, static_cast<hipStream_t>(stream), U, iu, W, iw, Y,
                     T, S);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_trip_basis_vec2_bwd_f32(const float* gY, const float* U, const int32_t* iu, const float* W, const int32_t* iw,
                                          float* GU, float* GW, int64_t T, int S, void* stream) {
  if (T <= 0) return 0;
  if (S < 1 || S > 8) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(trip_basis_vec2_bwd_kernel, dim3(grid_q(T)), dim3(256), 0, static_cast<hipStream_t>(stream), gY, U, iu, W,
                     iw, GU, GW, T, S);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_quad_basis_vec_fwd_f32(const float* V, const float* Vint, const int32_t* q_ca, const int32_t* q_db,
                                         const int32_t* q_abd, const int32_t* intm_ab, float* Y, int64_t Q, int S,
                                         void* stream) {
  if (Q <= 0) return 0;
  if (S < 1 || S > 7) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(quad_basis_vec_fwd_kernel, dim3(grid_q(Q)), dim3(256), (size_t)256 * S * S * sizeof(float),
                     static_cast<hipStream_t>(stream), V, Vint, QuadIdx{q_ca, q_db, q_abd, intm_ab}, Y, Q, S);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_quad_basis_vec_bwd_f32(const float* gY, const float* V, const float* Vint, const int32_t* q_ca,
                                         const int32_t* q_db, const int32_t* q_abd, const int32_t* intm_ab, float* Gc,
                                         float* Gbd, int64_t Q, int S, void* stream) {
  if (Q <= 0) return 0;
  if (S < 1 || S > 7) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(quad_basis_vec_bwd_kernel, dim3(grid_q(Q)), dim3(256), (size_t)256 * S * S * sizeof(float),
                     static_cast<hipStream_t>(stream), gY, V, Vint, QuadIdx{q_ca, q_db, q_abd, intm_ab}, Gc, Gbd, Q, S);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_quad_angles_vec_fwd_f32(const float* V, const float* Vint, const int32_t* q_ca, const int32_t* q_db,
                                          const int32_t* q_abd, const int32_t* intm_ab, float* ang, int64_t Q, void* stream) {
  if (Q <= 0) return 0;
  hipLaunchKernelGGL(quad_angles_vec_fwd_kernel, dim3(grid_q(Q)), dim3(256), 0, static_cast<hipStream_t>(stream), V, Vint,
                     QuadIdx{q_ca, q_db, q_abd, intm_ab}, reinterpret_cast<float4*>(ang), Q);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_quad_angles_vec_bwd_f32(const float* g_ang, const float* V, const float* Vint, const int32_t* q_ca,
                                          const int32_t* q_db, const int32_t* q_abd, const int32_t* intm_ab, float* Gc,
                                          float* Gbd, int64_t Q, void* stream) {
  if (Q <= 0) return 0;
  hipLaunchKernelGGL(quad_angles_vec_bwd_kernel, dim3(grid_q(Q)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const float4*>(g_ang), V, Vint, QuadIdx{q_ca, q_db, q_abd, intm_ab}, Gc, Gbd, Q);
  GN_LAUNCH_CHECK();
  return 0;
}
