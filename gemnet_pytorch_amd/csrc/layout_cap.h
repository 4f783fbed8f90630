// The capacity layout from device-resident structure sizes, shared by gn_pbc_layout (pbc_index.hip: periodic structures) and
// gn_index_gpu_layout (index_gpu.hip: molecules, which also need the offsets of their n x n adjacency blocks).
// One block: sum and validity of N first (an invalid layout sets bit 128 and writes no array), then the exclusive scan in rounds
// of 1024 structures with a carry, as pbc_scan_kernel.  No atomics; every launch is sized by the capacities.
#pragma once
#include "common.h"

namespace {

// n_max: capacity of ONE structure (0: no bound — gn_pbc_layout);  sq_off (n_mol + 1, may be NULL): exclusive scan of N_b^2
__global__ __launch_bounds__(1024) void cap_layout_scan_kernel(const int32_t* __restrict__ N, const int32_t* __restrict__ n_atoms,
                                                               int n_mol, int a_cap, int a_tot, int n_max,
                                                               int32_t* __restrict__ mol_off, int32_t* __restrict__ sq_off,
                                                               int64_t* __restrict__ N_pad, int32_t* __restrict__ state) {
  __shared__ int64_t wsum[16];
  __shared__ int64_t wsq[16];
  __shared__ int wbad[16];
  __shared__ int64_t carry_s, carry_sq;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t sum = 0;
  int bad = 0;
  for (int b = tid; b < n_mol; b += 1024) {
    const int32_t v = N[b];
    sum += v;
    bad |= v < 1;
    bad |= n_max > 0 && v > n_max;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    bad |= __shfl_xor(bad, o, 64);
  }
  if (lane == 0) { wsum[wave] = sum; wbad[wave] = bad; }
  if (tid == 0) { carry_s = 0; carry_sq = 0; }
  __syncthreads();
  int64_t total = 0;
  bad = 0;
  for (int w = 0; w < 16; ++w) { total += wsum[w]; bad |= wbad[w]; }
  if (bad || total != (int64_t)n_atoms[0] || total > (int64_t)a_cap) {      // (block-uniform)
    if (tid == 0) { state[0] |= 128; state[3] = 128; }
    return;
  }
  __syncthreads();                                            // wsum is reused by the scan
  for (int base = 0; base < n_mol; base += 1024) {
    const int b = base + tid;
    const int64_t v = b < n_mol ? (int64_t)N[b] : 0;
    const int64_t v2 = v * v;
    int64_t s = v, s2 = v2;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t t = __shfl_up(s, o, 64), t2 = __shfl_up(s2, o, 64);
      if (lane >= o) { s += t; s2 += t2; }
    }
    if (lane == 63) { wsum[wave] = s; wsq[wave] = s2; }
    __syncthreads();
    int64_t woff = 0, woff2 = 0;
    for (int w = 0; w < wave; ++w) { woff += wsum[w]; woff2 += wsq[w]; }
    const int64_t carry = carry_s, carry2 = carry_sq;
    if (b < n_mol) {
      mol_off[b] = (int32_t)(carry + woff + s - v);
      if (sq_off) sq_off[b] = (int32_t)(carry2 + woff2 + s2 - v2);      // <= a_cap * n_max <= 2^31 - 1 (checked on the host)
      N_pad[b] = v;
    }
    __syncthreads();
    if (tid == 1023) { carry_s = carry + woff + s; carry_sq = carry2 + woff2 + s2; }
    __syncthreads();
  }
  if (tid == 0) {
    mol_off[n_mol] = (int32_t)total;                          // the filler atoms [A, a_cap) form "structure" n_mol
    mol_off[n_mol + 1] = a_cap;
    if (sq_off) sq_off[n_mol] = (int32_t)carry_sq;
    N_pad[n_mol] = (int64_t)a_tot - total;                    // fillers + dummy atoms: the dummy molecule of padded.py
    state[3] = 0;
  }
}

// one thread per atom row of a_tot: its structure by bisection in mol_off (strictly ascending over [0, n_mol]: every N_b >= 1)
__global__ __launch_bounds__(256) void cap_layout_atoms_kernel(const int32_t* __restrict__ mol_off, int n_mol, int a_cap, int a_tot,
                                                               const int32_t* __restrict__ state, int32_t* __restrict__ atom_mol,
                                                               int64_t* __restrict__ batch_seg, float* __restrict__ mask) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a_tot || (state[3] & 128)) return;
  int m = n_mol;
  if (i < a_cap) {
    int lo = 0, hi = n_mol + 1;                               // first index in [0, n_mol] with mol_off > i, or n_mol + 1
    while (lo < hi) {
      const int md = (lo + hi) >> 1;
      if (mol_off[md] <= i) lo = md + 1; else hi = md;
    }
    m = lo - 1;
    atom_mol[i] = m;
    mask[i] = i < mol_off[n_mol] ? 1.0f : 0.0f;
  }
  batch_seg[i] = m;
}

}  // namespace
