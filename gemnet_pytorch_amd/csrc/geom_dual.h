// Forward-mode dual numbers and the first adjoint of the neighbour angle as a template over the scalar type: shared by the
// position form (geometry2.hip) and the edge-vector form (pbc_train.hip) of the twice-differentiable training geometry, so that
// the clamp logic of atan2(max(|u x v|, 1e-9), u.v) exists once.
#pragma once
#include "common.h"

namespace {

struct Dual {
  float v, d;
};
__device__ __forceinline__ Dual mk(float v, float d = 0.f) { return {v, d}; }
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dual operator-(Dual a) { return {-a.v, -a.d}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ Dual operator/(Dual a, Dual b) {
  const float q = a.v / b.v;
  return {q, (a.d - q * b.d) / b.v};
}
__device__ __forceinline__ Dual dsqrt(Dual a) {
  const float s = sqrtf(a.v);
  return {s, 0.5f * a.d / s};
}
__device__ __forceinline__ float dsqrt(float a) { return sqrtf(a); }
__device__ __forceinline__ float val(float a) { return a; }
__device__ __forceinline__ float val(Dual a) { return a.v; }
__device__ __forceinline__ void lift(float& o, float v) { o = v; }
__device__ __forceinline__ void lift(Dual& o, float v) { o = {v, 0.f}; }

template <class T>
struct V3 {
  T x, y, z;
};
template <class T>
__device__ __forceinline__ T dot(const V3<T>& a, const V3<T>& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
template <class T>
__device__ __forceinline__ V3<T> cross(const V3<T>& a, const V3<T>& b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// First adjoint of theta(u, v) = atan2(max(|u x v|, 1e-9), u.v):  gu = g dtheta/du, gv = g dtheta/dv  (the clamp has a
// zero gradient through y, gemnet.py:309: torch.max(y, 1e-9)).  Same formulas as trip_basis_bwd_kernel (geometry.hip).
// kRel (the position form, geometry2.hip): the clamp decision relative to the vectors, sin < GN_REL_SIN, as in geometry.hip —
// off the axes the cross product of an exactly collinear triplet is a residue of 1e-7 |u| |v| whose direction is rounding
// noise; y then enters as a constant.  The edge-vector twins (pbc_train.hip, pbc_quad_train.hip) keep the absolute decision.
template <class T, bool kRel = false>
__device__ __forceinline__ void angle_adjoint(const V3<T>& u, const V3<T>& v, const T g, V3<T>& gu, V3<T>& gv) {
  const T x = dot(u, v);
  const V3<T> w = cross(u, v);
  const T w2 = dot(w, w);
  const T yn = dsqrt(w2);
  const bool clamped =
      val(yn) < 1e-9f || (kRel && val(w2) <= (GN_REL_SIN * GN_REL_SIN) * val(dot(u, u)) * val(dot(v, v)));
  T y, zero;
  lift(zero, 0.f);
  lift(y, val(yn) < 1e-9f ? 1e-9f : val(yn));
  if (!clamped) y = yn;
  const T r2 = x * x + y * y;
  const T dx = -(y / r2) * g;
  T dy = zero;
  V3<T> n = {zero, zero, zero};
  if (!clamped) {
    dy = (x / r2) * g;
    n = {w.x / y, w.y / y, w.z / y};
  }
  const V3<T> vn = cross(v, n), nu = cross(n, u);      // d|u x v|/du = v x n,  d|u x v|/dv = n x u
  gu = {dx * v.x + dy * vn.x, dx * v.y + dy * vn.y, dx * v.z + dy * vn.z};
  gv = {dx * u.x + dy * nu.x, dx * u.y + dy * nu.y, dx * u.z + dy * nu.z};
}

}  // namespace
