// Lane mapping experiment for the radial head's adjoint (profiles/radial_emb_timeline.txt section 6):
// a block of 64 edges x 8 waves, wave w evaluates ONE role for its 64 edges (w < 7: the six radial functions of l = w; w = 7:
// the six Bessel rbf), so the order l and the loop bounds of the f64 evaluations are wave-uniform.  The library kernel gives a
// wave 4 edges x 16 lanes with j = sub, sub + 16, sub + 32: rbf and two to four different l per round.
// The per-function factors (c_j fp32, f_j' f64) go through LDS and one lane per edge forms the sum in the library kernel's
// association: sixteen partials q, each over j = q, q + 16, q + 32, added q = 0..15 — W is meant to be bit-identical.
// Not part of the library: built and timed by tools/exp/radial_head_roles.py.
#include "../../gemnet_pytorch_amd/csrc/common.h"
#include "../../gemnet_pytorch_amd/csrc/basis_math.h"

namespace {

constexpr int NR = 6, S = 7, NI = 16, NFUN = NR + S * NR, EPB = 64, BLOCK = 512;

__device__ __forceinline__ float dot16(const float* __restrict__ w, const float* __restrict__ g) {
  float acc = 0.f;
#pragma unroll
  for (int q = 0; q < NI / 4; ++q) {
    const float4 a = reinterpret_cast<const float4*>(w)[q];
    const float4 b = reinterpret_cast<const float4*>(g)[q];
    acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc); acc = fmaf(a.z, b.z, acc); acc = fmaf(a.w, b.w, acc);
  }
  return acc;
}

__global__ void __launch_bounds__(BLOCK)
radial_head_bwd_roles_kernel(const float* __restrict__ g_rbf, const float* __restrict__ g_rbf3, const float* __restrict__ g_rbf_h,
                             const float* __restrict__ g_rbf_out, const float* __restrict__ g_rbf_W1, const float* __restrict__ R,
                             const int32_t* __restrict__ id_c, const int32_t* __restrict__ id_a, const float* __restrict__ freq,
                             const float* __restrict__ z, const double* __restrict__ nrm, const float* __restrict__ wcat,
                             float* __restrict__ Wout, int64_t E, double cutoff, int p) {
  __shared__ double ev[NFUN][EPB];
  __shared__ float cf[NFUN][EPB];
  const int w = threadIdx.x / EPB, el = threadIdx.x % EPB;
  const int64_t e = blockIdx.x * (int64_t)EPB + el;
  const bool ok = e < E;
  float vx = 0.f, vy = 0.f, vz = 0.f, d = 1.f;
  if (ok) {
    const float* Ra = R + 3 * (int64_t)id_a[e];
    const float* Rc = R + 3 * (int64_t)id_c[e];
    vx = Ra[0] - Rc[0]; vy = Ra[1] - Rc[1]; vz = Ra[2] - Rc[2];
    d = sqrtf(vx * vx + vy * vy + vz * vz);
  }
  const bool any_rbf = g_rbf || g_rbf3 || g_rbf_h || g_rbf_out;
#pragma unroll 1
  for (int r = 0; r < NR; ++r) {
    float c = 0.f;
    double f = 0.0;
    int j;
    if (w == S) {
      j = r;
      if (ok && any_rbf) {
        c = g_rbf ? g_rbf[e * NR + r] : 0.f;
        if (g_rbf3) c += dot16(wcat + (0 * NR + r) * NI, g_rbf3 + e * NI);
        if (g_rbf_h) c += dot16(wcat + (1 * NR + r) * NI, g_rbf_h + e * NI);
        if (g_rbf_out) c += dot16(wcat + (2 * NR + r) * NI, g_rbf_out + e * NI);
        f = bessel_rbf_eval((double)d, (double)freq[r], cutoff, p, 1, 0);
      }
    } else {
      const int lr = w * NR + r;
      j = NR + lr;
      if (ok && g_rbf_W1) {
        c = dot16(wcat + (3 * NR + lr) * NI, g_rbf_W1 + (e * S + w) * NI);
        f = sph_radial_eval((double)d, (double)z[lr], nrm[lr], w, cutoff, p, 1);
      }
    }
    cf[j][el] = c;
    ev[j][el] = f;
  }
  __syncthreads();
  if (w == 0 && ok) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      double g = 0.0;
#pragma unroll
      for (int j = q; j < NFUN; j += 16) g += (double)cf[j][el] * ev[j][el];
      t += g;
    }
    const float sc = (float)(t / (double)d);
    Wout[3 * e] = sc * vx; Wout[3 * e + 1] = sc * vy; Wout[3 * e + 2] = sc * vz;
  }
}

}  // namespace

extern "C" int exp_radial_head_bwd_roles(const float* g_rbf, const float* g_rbf3, const float* g_rbf_h, const float* g_rbf_out,
                                         const float* g_rbf_W1, const float* R, const int32_t* id_c, const int32_t* id_a,
                                         const float* freq, const float* z, const double* nrm, const float* wcat, float* W,
                                         int64_t E, float cutoff, int p, void* stream) {
  if (E <= 0) return 0;
  hipLaunchKernelGGL(radial_head_bwd_roles_kernel, dim3((unsigned)((E + EPB - 1) / EPB)), dim3(BLOCK), 0,
                     static_cast<hipStream_t>(stream), g_rbf, g_rbf3, g_rbf_h, g_rbf_out, g_rbf_W1, R, id_c, id_a, freq, z, nrm, wcat,
                     W, E, (double)cutoff, p);
  GN_LAUNCH_CHECK();
  return 0;
}
