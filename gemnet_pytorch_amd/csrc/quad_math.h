// Per-quadruplet geometry of GemNet-Q, c -> a - b <- d (gemnet.py:334-418), on the three difference vectors
//   uac = c - a,  uab = b - a,  ubd = d - b:
// the polar angle Phi_cab = angle(uab, uac) and the azimuth Theta_cabd = angle(reject(uac, uab), reject(ubd, -uab)), and the
// first adjoint onto the three vectors.  Shared by the molecular kernels (geometry.hip: vectors from atom positions) and the
// periodic ones (pbc_quad.hip: vectors from the edge / interaction-edge arrays), so the clamps and the decisions at the
// degeneracies are stated once.
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

// ---- the two angles of one quadruplet, their adjoint and their tangent: ONE body for molecules and crystals ------------------
// c - a - b or a - b - d can be EXACTLY collinear and a quadruplet EXACTLY planar: in a crystal an atom and its own images, c -> a
// and d -> b related by a lattice translation; in a molecule CO2, acetylene, ethylene, benzene (planar, and its para atoms
// H - C ... C - H on one line).  There the reference's clamp decides: in exact (and fp64, axis-aligned) arithmetic the cross
// product vanishes, the angle sits on the clamp and its gradient is zero — the symmetric choice where the unsigned angle has a
// kink (planar: the one-sided slopes are +-1 / |p|) or the azimuth is not defined (collinear: the rejection vanishes and the
// azimuth is atan2(1e-9, 0) = pi / 2).  In fp32, and in ANY arithmetic once the structure is not aligned with the axes, the same
// cross product is a rounding residue of relative size 1e-7, far above the ABSOLUTE 1e-9: the kernel would differentiate the
// noise (1 / residue) or pick one side of the kink, differently for every copy of the same quadruplet.  So the clamp decision is
// taken RELATIVE to the vectors' lengths: sin below kRelSin counts as the exact degeneracy.  Away from a degeneracy nothing
// differs from the reference's formulas.  Value, adjoint and tangent read the SAME decisions (quad_decide), so the forces are the
// gradient of the energy and the second-order pass differentiates that same function.
constexpr float kRelSin = GN_REL_SIN;
constexpr float kRelSin2 = kRelSin * kRelSin;

__device__ __forceinline__ bool rel_parallel(V3 u, V3 v) {
  const V3 w = cross(u, v);
  return dot(w, w) <= kRelSin2 * dot(u, u) * dot(v, v);
}
// the rejection p of x has vanished: x is (anti)parallel to the vector it was rejected from
__device__ __forceinline__ bool rel_vanished(V3 p, V3 x) { return dot(p, p) <= kRelSin2 * dot(x, x); }

struct QuadDecision {
  V3 uba, p1, p2;   // -uab and the two rejections
  bool vanished;    // a rejection has vanished: the azimuth is the convention (sin, cos) = (1, 0)
  bool flat;        // c - a - b collinear: the polar angle is a constant
  bool fixed;       // vanished, or the quadruplet is planar: the azimuth sits on its clamp, a constant
};
template <bool kAdjoint>
__device__ __forceinline__ QuadDecision quad_decide(V3 uac, V3 uab, V3 ubd) {
  QuadDecision d;
  d.uba = (-1.0f) * uab;
  d.p1 = reject(uac, uab);
  d.p2 = reject(ubd, d.uba);
  d.vanished = rel_vanished(d.p1, uac) || rel_vanished(d.p2, ubd);
  d.flat = kAdjoint && rel_parallel(uab, uac);          // (the value kernels need `vanished` alone)
  d.fixed = kAdjoint && (d.vanished || rel_parallel(d.p1, d.p2));
  return d;
}

// (sin, cos) of the polar angle Phi_cab and of the azimuth Theta_cabd of one quadruplet
__device__ __forceinline__ void quad_angles_sc(V3 uac, V3 uab, V3 ubd, double& sn, double& cs, double& s1, double& c1) {
  angle_uv_sc(uab, uac, sn, cs);
  const QuadDecision d = quad_decide<false>(uac, uab, ubd);
  if (d.vanished) {
    s1 = 1.0;            // atan2(1e-9, 0): the reference's value of an azimuth that is not defined
    c1 = 0.0;
    return;
  }
  angle_uv_sc(d.p1, d.p2, s1, c1);
}

// adjoint: g_phi = dE/dPhi_cab, g_th = dE/dTheta_cabd -> dE/duac, dE/duab, dE/dubd
__device__ __forceinline__ void quad_angles_adj(V3 uac, V3 uab, V3 ubd, float g_phi, float g_th, V3& g_ac, V3& g_ab, V3& g_bd) {
  const QuadDecision d = quad_decide<true>(uac, uab, ubd);
  V3 gp1, gp2, t1, t2, g_ba;
  if (d.flat) {
    g_ab = {0.f, 0.f, 0.f};
    g_ac = {0.f, 0.f, 0.f};
  } else {
    angle_uv_bwd(uab, uac, g_phi, g_ab, g_ac);
  }
  if (d.fixed) {
    g_bd = {0.f, 0.f, 0.f};
    return;
  }
  angle_uv_bwd(d.p1, d.p2, g_th, gp1, gp2);
  reject_bwd(uac, uab, gp1, t1, t2);   // d p1 / d(uac, uab)
  g_ac = g_ac + t1; g_ab = g_ab + t2;
  reject_bwd(ubd, d.uba, gp2, g_bd, g_ba);
  g_ab = g_ab - g_ba;                   // uba = -uab
}

// tangent: (dPhi_cab, dTheta_cabd) along (dac, dab, dbd) — the closed-form adjoints with unit cotangents, contracted with the
// tangent vectors, under the decisions of the adjoint
__device__ __forceinline__ void quad_angles_tan(V3 uac, V3 uab, V3 ubd, V3 dac, V3 dab, V3 dbd, float& dphi, float& dth) {
  const QuadDecision d = quad_decide<true>(uac, uab, ubd);
  V3 g_ab, g_ac, gp1, gp2, t1, t2, g_bd, g_ba;
  dphi = 0.f;
  dth = 0.f;
  if (!d.flat) {
    angle_uv_bwd(uab, uac, 1.0f, g_ab, g_ac);
    dphi = dot(g_ab, dab) + dot(g_ac, dac);
  }
  if (!d.fixed) {
    angle_uv_bwd(d.p1, d.p2, 1.0f, gp1, gp2);
    reject_bwd(uac, uab, gp1, t1, t2);        // d p1 / d(uac, uab)
    reject_bwd(ubd, d.uba, gp2, g_bd, g_ba);  // d p2 / d(ubd, uba);  d uba = -d uab
    dth = dot(t1, dac) + dot(t2, dab) + dot(g_bd, dbd) - dot(g_ba, dab);
  }
}

}  // namespace
