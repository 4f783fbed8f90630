// Energy head of the grouped OutputBlocks (include/gemnet_hip.h, gn_energy_head_fwd_f32 / gn_energy_head_bwd_f32).
//
// Reference (atom_update_block.py:168-172, gemnet.py:596-600): every OutputBlock ends in out_energy = Dense(emb_size_atom, 1)
// and the model sums the blocks' energies per atom.  As separate launches that is one N = 1 GEMM per block (each adding the
// running sum in its epilogue) and, in the adjoint, one K = 1 GEMM per block that spreads dE/dE_a over the block's 128
// columns.  With the blocks' final rows stacked (G, A, 128) both are one small pass:
//   forward : one wave per atom; lane l owns columns 2l, 2l+1 of every group's row, a 64-lane xor butterfly folds the dot
//             product, the G dot products are added in block order (the order of the chained epilogues)
//   adjoint : one thread per float4 of the stacked seed g_x[g, a, :] = g_E[a] * w[g]
#include "common.h"

namespace {

constexpr int C = 128;

__global__ __launch_bounds__(256) void energy_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              float* __restrict__ E, int G, int64_t n_atoms) {
  const int lane = threadIdx.x & 63;
  const int64_t a = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (a >= n_atoms) return;
  float sum = 0.f;
  for (int g = 0; g < G; ++g) {
    const float2 xv = *reinterpret_cast<const float2*>(x + ((size_t)g * n_atoms + a) * C + 2 * lane);
    const float2 wv = *reinterpret_cast<const float2*>(w + (size_t)g * C + 2 * lane);
    float d = xv.x * wv.x + xv.y * wv.y;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) d += __shfl_xor(d, o, 64);
    sum = g == 0 ? d : sum + d;
  }
  if (lane == 0) E[a] = sum;
}

__global__ __launch_bounds__(256) void energy_head_bwd_kernel(const float* __restrict__ g_E, const float* __restrict__ w,
                                                              float* __restrict__ g_x, int G, int64_t n_atoms) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // float4 index into (G, n_atoms, C)
  const int64_t total = (int64_t)G * n_atoms * (C / 4);
  if (i >= total) return;
  const int c4 = (int)(i % (C / 4));
  const int64_t ga = i / (C / 4);
  const int g = (int)(ga / n_atoms);
  const int64_t a = ga - (int64_t)g * n_atoms;
  const float ge = g_E[a];
  const float4 wv = *reinterpret_cast<const float4*>(w + (size_t)g * C + 4 * c4);
  *reinterpret_cast<float4*>(g_x + i * 4) = make_float4(ge * wv.x, ge * wv.y, ge * wv.z, ge * wv.w);
}

}  // namespace

extern "C" int gn_energy_head_fwd_f32(const float* x, const float* w, float* E, int G, int64_t n_atoms, int C_, void* stream) {
  if (C_ != C || G <= 0 || G > 8) return (int)hipErrorInvalidValue;
  if (n_atoms <= 0) return 0;
  hipLaunchKernelGGL(energy_head_fwd_kernel, dim3((unsigned)gn_cdiv(n_atoms, 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     x, w, E, G, n_atoms);
  GN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gn_energy_head_bwd_f32(const float* g_E, const float* w, float* g_x, int G, int64_t n_atoms, int C_, void* stream) {
  if (C_ != C || G <= 0 || G > 8) return (int)hipErrorInvalidValue;
  if (n_atoms <= 0) return 0;
  const int64_t total = (int64_t)G * n_atoms * (C / 4);
  hipLaunchKernelGGL(energy_head_bwd_kernel, dim3((unsigned)gn_cdiv(total, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     g_E, w, g_x, G, n_atoms);
  GN_LAUNCH_CHECK();
  return 0;
}
