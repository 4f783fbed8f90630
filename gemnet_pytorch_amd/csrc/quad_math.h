// Per-quadruplet geometry of GemNet-Q, c -> a - b <- d (gemnet.py:334-418), on the three difference vectors
//   uac = c - a,  uab = b - a,  ubd = d - b:
// the polar angle Phi_cab = angle(uab, uac) and the azimuth Theta_cabd = angle(reject(uac, uab), reject(ubd, -uab)), and the
// first adjoint onto the three vectors.  Shared by the molecular kernels (geometry.hip: vectors from atom positions) and the
// periodic ones (pbc_quad.hip: vectors from the edge / interaction-edge arrays), so the clamps are stated once.
#pragma once
#include "common.h"

namespace {

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(const float* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// theta = atan2(max(|u x v|, 1e-9), u.v) and, for a given dL/dtheta, dL/du and dL/dv
__device__ __forceinline__ float angle_uv(V3 u, V3 v) {
  const V3 w = cross(u, v);
  const float yn = sqrtf(dot(w, w));
  return atan2f(yn < 1e-9f ? 1e-9f : yn, dot(u, v));
}
// (sin, cos) of that angle without atan2 / sincos: with y = max(|u x v|, 1e-9), x = u.v: sin = y / hypot(x, y),
// cos = x / hypot(x, y)  (exactly the sine and cosine of atan2(y, x))
__device__ __forceinline__ void angle_uv_sc(V3 u, V3 v, double& sn, double& cs) {
  const V3 w = cross(u, v);
  const float yn = sqrtf(dot(w, w));
  const double y = yn < 1e-9f ? 1e-9 : (double)yn;
  const double x = (double)dot(u, v);
  const double ir = 1.0 / sqrt(x * x + y * y);
  sn = y * ir;
  cs = x * ir;
}
__device__ __forceinline__ void angle_uv_bwd(V3 u, V3 v, float gth, V3& gu, V3& gv) {
  const V3 w = cross(u, v);
  const float x = dot(u, v);
  const float yn = sqrtf(dot(w, w));
  const bool clamped = yn < 1e-9f;
  const float y = clamped ? 1e-9f : yn;
  const float r2 = x * x + y * y;
  const float dx = -y / r2 * gth;
  const float dy = clamped ? 0.f : x / r2 * gth;
  const V3 n = (clamped ? 0.f : 1.0f / y) * w;
  gu = dx * v + dy * cross(v, n);
  gv = dx * u + dy * cross(n, u);
}
// r = x - (x.n / n.n) n  (vector_rejection, gemnet.py:313-332) and its adjoint
__device__ __forceinline__ V3 reject(V3 x, V3 n) { return x - (dot(x, n) / dot(n, n)) * n; }
__device__ __forceinline__ void reject_bwd(V3 x, V3 n, V3 gr, V3& gx, V3& gn) {
  const float s = dot(x, n), q = dot(n, n), a = s / q, gn_dot = dot(gr, n);
  gx = gr - (gn_dot / q) * n;
  gn = (-a) * gr - gn_dot * ((1.0f / q) * x - (2.0f * s / (q * q)) * n);
}

// ---- the two angles of one quadruplet and their adjoint: ONE body for molecules and crystals -----------------------------------
// kRel = false: the molecular kernels — the reference's absolute clamp max(|u x v|, 1e-9) inside angle_uv_*, nothing else.
// kRel = true: the periodic kernels.  In a crystal c - a - b or a - b - d can be EXACTLY collinear (an atom and its own images)
// and a quadruplet EXACTLY planar (c -> a and d -> b related by a lattice translation).  There the reference's clamp decides: in
// exact (and fp64) arithmetic the cross product vanishes, the angle sits on the clamp and its gradient is zero — the symmetric
// choice where the unsigned angle has a kink (planar: the one-sided slopes are +-1 / |p|) or the azimuth is not defined
// (collinear: the rejection vanishes and the azimuth is atan2(1e-9, 0) = pi / 2).  In fp32 the same cross product is a rounding
// residue of relative size 1e-7, far above the ABSOLUTE 1e-9: the kernel would differentiate the noise (1 / residue) or pick one
// side of the kink, differently for every translation copy of the same quadruplet.  With kRel the clamp decision is taken
// RELATIVE to the vectors' lengths: sin below kRelSin counts as the exact degeneracy.  The primitives, the formulas and every
// value away from a degeneracy are the same statements for both.
constexpr float kRelSin = 1e-5f;
constexpr float kRelSin2 = kRelSin * kRelSin;

__device__ __forceinline__ bool rel_parallel(V3 u, V3 v) {
  const V3 w = cross(u, v);
  return dot(w, w) <= kRelSin2 * dot(u, u) * dot(v, v);
}
// the rejection p of x has vanished: x is (anti)parallel to the vector it was rejected from
__device__ __forceinline__ bool rel_vanished(V3 p, V3 x) { return dot(p, p) <= kRelSin2 * dot(x, x); }

// (sin, cos) of the polar angle Phi_cab and of the azimuth Theta_cabd of one quadruplet
template <bool kRel>
__device__ __forceinline__ void quad_angles_sc_t(V3 uac, V3 uab, V3 ubd, double& sn, double& cs, double& s1, double& c1) {
  const V3 uba = (-1.0f) * uab;
  angle_uv_sc(uab, uac, sn, cs);
  const V3 p1 = reject(uac, uab), p2 = reject(ubd, uba);
  if (kRel && (rel_vanished(p1, uac) || rel_vanished(p2, ubd))) {
    s1 = 1.0;            // atan2(1e-9, 0): the reference's value of an azimuth that is not defined
    c1 = 0.0;
    return;
  }
  angle_uv_sc(p1, p2, s1, c1);
}

// adjoint: g_phi = dE/dPhi_cab, g_th = dE/dTheta_cabd -> dE/duac, dE/duab, dE/dubd
template <bool kRel>
__device__ __forceinline__ void quad_angles_adj_t(V3 uac, V3 uab, V3 ubd, float g_phi, float g_th, V3& g_ac, V3& g_ab, V3& g_bd) {
  const V3 uba = (-1.0f) * uab;
  const V3 p1 = reject(uac, uab), p2 = reject(ubd, uba);
  V3 gp1, gp2, t1, t2, g_ba;
  if (kRel && rel_parallel(uab, uac)) {
    g_ab = {0.f, 0.f, 0.f};
    g_ac = {0.f, 0.f, 0.f};
  } else {
    angle_uv_bwd(uab, uac, g_phi, g_ab, g_ac);
  }
  if (kRel && (rel_vanished(p1, uac) || rel_vanished(p2, ubd) || rel_parallel(p1, p2))) {   // the azimuth sits on its clamp
    g_bd = {0.f, 0.f, 0.f};
    return;
  }
  angle_uv_bwd(p1, p2, g_th, gp1, gp2);
  reject_bwd(uac, uab, gp1, t1, t2);   // d p1 / d(uac, uab)
  g_ac = g_ac + t1; g_ab = g_ab + t2;
  reject_bwd(ubd, uba, gp2, g_bd, g_ba);
  g_ab = g_ab - g_ba;                   // uba = -uab
}

// the molecular kernels (geometry.hip) ...
__device__ __forceinline__ void quad_angles_sc(V3 uac, V3 uab, V3 ubd, double& sn, double& cs, double& s1, double& c1) {
  quad_angles_sc_t<false>(uac, uab, ubd, sn, cs, s1, c1);
}
__device__ __forceinline__ void quad_angles_adj(V3 uac, V3 uab, V3 ubd, float g_phi, float g_th, V3& g_ac, V3& g_ab, V3& g_bd) {
  quad_angles_adj_t<false>(uac, uab, ubd, g_phi, g_th, g_ac, g_ab, g_bd);
}
// ... and the periodic ones (pbc_quad.hip)
__device__ __forceinline__ void quad_angles_sc_rel(V3 uac, V3 uab, V3 ubd, double& sn, double& cs, double& s1, double& c1) {
  quad_angles_sc_t<true>(uac, uab, ubd, sn, cs, s1, c1);
}
__device__ __forceinline__ void quad_angles_adj_rel(V3 uac, V3 uab, V3 ubd, float g_phi, float g_th, V3& g_ac, V3& g_ab,
                                                    V3& g_bd) {
  quad_angles_adj_t<true>(uac, uab, ubd, g_phi, g_th, g_ac, g_ab, g_bd);
}

}  // namespace
