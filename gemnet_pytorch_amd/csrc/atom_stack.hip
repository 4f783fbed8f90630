// The forward of the atom-row MLP stack as a kernel of its own (include/gemnet_hip.h, gn_atom_stack_fwd_f32), and, in the second
// half of the file, its first-order adjoint (gn_atom_stack_bwd_f32); both also as grouped launches for the stage of the grouped
// OutputBlocks (gn_atom_stack_fwd_grouped_f32 / gn_atom_stack_bwd_grouped_f32: template parameters GR, SEED, RT below).
//
// Why: the stacks that run on ATOM rows (AtomUpdateBlock: Dense + ResidualLayers + the tail projections of the concat layer,
// M = 1 024 rows, 128 -> 128) are 64 workgroups of one 16-row tile each on 256 CUs: pure latency, and the chain
// interpreter (chain2.hip) spends ~5.8 k cycles per GEMM op there for ~1.6 k of matrix-pipe phase — descriptor decode, weights
// requested one op ahead, an epilogue shaped for five row blocks and any operand kind.  Here the program is fixed at compile
// time (L ResidualLayers, T tails, final skip or not) and everything that does not change a value is specialised:
//   * no op table: template parameters and a plain argument struct;
//   * the tile's rows, then the weight fragments of the first AS_AHEAD ops are requested at kernel entry, those of op
//     j + AS_AHEAD when op j's MFMA phase is over (one op is 32 VGPRs per lane);
//   * all eight fragment reads of an op, its LDS residual and its global skip operand are issued before the first MFMA;
//   * the epilogue runs in registers; one barrier per op, none between or behind the tails.
// What is NOT changed is the arithmetic: the activation tile sits in LDS in the two-fp16-plane format of
// chain_split_kernel<1, 2, false, true> (no row scale: the forward is not a linear program), the same swizzle, the same K order
// per accumulator (hh | hl | lh, k-chunks 0..3), the same epilogue expressions in the same order — every output is bit for bit
// what gn_chain_split_f32 writes for the same program (tests/test_gpu_atom_stack.py).
// Weights: the planes gn_pack_weight_split_fmt(..., GN_SPLIT_F16X2) produces; no packing of its own.
#include <type_traits>

#include "common.h"

#include "chain_split.h"

// Bit-equality with chain_split_kernel needs the same roundings, and which multiply-add pairs the compiler contracts depends
// on the code around them: in the interpreter the stages of an epilogue sit in different basic blocks (one uniform branch per
// stage) and nothing is contracted across them, in the straight-line code below everything would be.  So contraction is off for
// this file and the two fused operations the interpreter's code does have are written out (as_fma): the collapse of the
// correction accumulators, and (s + x s) - s (x s) of the activation derivative.
#pragma clang fp contract(off)

// Knock-outs of diagnosis builds (never defined in the product library; tools/atom_stack_bench.py says how they are built):
//   AS_EXP == 1  no weight fetch (zero fragments)      AS_EXP == 2  no activation arithmetic in the epilogue
//   AS_EXP == 3  no MFMAs                              AS_EXP == 4  no barriers between the ops (timing only: the tile races)
#ifndef AS_EXP
#define AS_EXP 0
#endif

#ifndef AS_GROUP_TILES
// 16-row tiles per workgroup of the GROUPED launches (1 or 2).  Measured at G = 5, A = 1 024 (us per launch, forward / adjoint):
// 1 -> 11.4 / 9.5 (320 workgroups, two per CU, every one fetching all 64 KB per op), 2 -> 9.8 / 8.2 (160 workgroups, one per CU,
// half the weight traffic); profiles/out_group_atoms_timeline.txt
#define AS_GROUP_TILES 2
#endif

#ifndef AS_AHEAD
// GEMM ops whose weight fragments are in flight or resident ahead of the running one.  Measured at M = 1 024 (7 GEMMs, us per
// launch): 2 -> 7.52, 3 -> 7.65, 4 -> 7.75, 5 -> 7.91, 7 (everything at entry) -> 8.4: every CU asks the L2 for the same 64 KB per op
// at the same time, and what is requested early only delays the first op's fragments (profiles/atom_stack_timeline.txt).
#define AS_AHEAD 2
#endif

namespace {
using namespace gn_split;

__device__ __forceinline__ float as_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// ssilu(x) and ssilu'(x) from one sigmoid, rounded as gn_ssilu_pair is inside chain_split_kernel:
// xs = x s;  d = fma(-s, xs, s + xs) / 0.6;  y = xs / 0.6
__device__ __forceinline__ void as_ssilu_pair(float x, float& y, float& d) {
  const float s = gn_sigmoid(x), xs = x * s;
  const float t = s + xs;
  d = as_fma(-s, xs, t) * GN_INV_06;
  y = xs * GN_INV_06;
}

constexpr int AS_MAX_GEMMS = 7;    // Dense + 2 x 2 + 2 tails
constexpr int AS_MAX_ROWS = 4096;  // where gn_chain_split_f32 runs 16-row tiles too
constexpr int AS_MAX_GROUPS = 8;   // GN_CHAIN_MAX_GROUPS
constexpr int AS_W_UINT4 = 8 * 4 * 2 * 64;      // one packed 128 x 128 weight: [col tile][k-chunk][plane][lane] uint4 (64 KiB)

struct as_fwd_args {
  const float* x;
  int M;
  const uint4* W[AS_MAX_GEMMS];    // packed planes in program order: W0, (W1, W2) per layer, tails
  float* z[5];                     // ssilu'(z) of the Dense and of both GEMMs of every layer
  float s;                         // ResidualLayer scale
  const float* res2;               // final skip (RES2)
  float beta2;
  float* y;
  float* t[2];                     // tail outputs
  int pitch;                       // grouped launch: rows between the groups' slabs of x, z, y
};

// One template for the single and the grouped launch.  L ResidualLayers, T tails, RES2: the final global skip.
// GR (gn_atom_stack_fwd_grouped_f32): blockIdx.y is the group, whose rows lie P.pitch rows and whose packed weights one weight
// behind those of the group before; a tile never spans two groups (rows >= M are masked as ever).
// RT: 16-row tiles of one workgroup: 1 in the single launch, AS_GROUP_TILES (by default 2 — every weight fragment is fetched once
// for both) in the grouped one; each tile has its own two LDS slots and its own accumulators, a row's
// arithmetic does not know about the other tile.  With GR = false, RT = 1 every [r] below is a scalar and rg, wg are 0.
template <int L, int T, bool RES2, bool GR, int RT>
__global__ __launch_bounds__(NT) void atom_stack_fwd_kernel(const as_fwd_args P) {
  static_assert(L >= 0 && L <= 2 && T >= 0 && T <= 2 && (!RES2 || L > 0), "programs of the atom stack");
  static_assert(!GR || (L >= 1 && T == 0 && !RES2), "programs of the grouped output blocks");
  static_assert(RT == 1 || (GR && RT == 2), "one row tile, or two in the grouped launch");
  constexpr int NM = 1 + 2 * L;              // GEMM ops that write the tile
  constexpr int NG = NM + T;
  constexpr int PLANE = 16 * ROWB;           // bytes of one plane
  constexpr int SLOT = 2 * PLANE;
  constexpr int TILE = 2 * SLOT;             // LDS of one row tile
  __shared__ __attribute__((aligned(16))) unsigned char smem[RT * TILE];
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int l15 = lane & 15;
  const int lg = lane >> 4;
  const int M = P.M;
  const int row0 = (int)blockIdx.x * (16 * RT);
  size_t rg = 0, wg = 0;                     // this group's offset into the row operands (floats) / the weights (uint4)
  if constexpr (GR) {
    rg = (size_t)blockIdx.y * (size_t)P.pitch * SW;
    wg = (size_t)blockIdx.y * AS_W_UINT4;
  }

  // weight fragments: [op][k-chunk][plane]; packed layout [col tile][k-chunk][plane][lane][8 fp16]
  uint4 w[NG][4][2];
  auto wload = [&](auto jc) {
    constexpr int j = decltype(jc)::value;
    if constexpr (j < NG) {
      const uint4* __restrict__ const base = P.W[j] + wg + (size_t)wave * (4 * 2 * 64) + lane;
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int p = 0; p < 2; ++p) w[j][c][p] = AS_EXP == 1 ? make_uint4(0x3c003c00u + lane, 0u, 0u, 0u) : base[(c * 2 + p) * 64];
    }
  };
  // the tile's rows are requested first: returns are in order, and the LOAD below must not wait behind the weight sets
  const int lr = tid >> 5, lc = (tid & 31) << 2;      // 16 rows x 32 float4 = one float4 per thread and tile
  float4 xv[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    xv[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + 16 * r + lr < M) xv[r] = *reinterpret_cast<const float4*>(P.x + rg + (size_t)(row0 + 16 * r + lr) * SW + lc);
  }
  wload(std::integral_constant<int, 0>{});
  if constexpr (AS_AHEAD > 1) wload(std::integral_constant<int, 1>{});
  if constexpr (AS_AHEAD > 2) wload(std::integral_constant<int, 2>{});
  if constexpr (AS_AHEAD > 3) wload(std::integral_constant<int, 3>{});
  if constexpr (AS_AHEAD > 4) wload(std::integral_constant<int, 4>{});
  if constexpr (AS_AHEAD > 5) wload(std::integral_constant<int, 5>{});
  if constexpr (AS_AHEAD > 6) wload(std::integral_constant<int, 6>{});

  auto plane_ptr = [&](int r, int slot, int p) -> unsigned char* { return smem + r * TILE + slot * SLOT + p * PLANE; };
  // byte offset of columns col .. col+3 (col % 4 == 0) of row `row` inside a plane (the swizzle of chain2.hip)
  auto sw_off = [&](int row, int col) -> int { return row * ROWB + ((((col >> 3) ^ row) & 15) << 4) + ((col & 4) << 1); };
  auto slot_write = [&](int r, int slot, int row, int col, const float4 v) {
    const int off = sw_off(row, col);
    uint2 H, Lo;
    split4h(v, H, Lo);
    *reinterpret_cast<uint2*>(plane_ptr(r, slot, 0) + off) = H;
    *reinterpret_cast<uint2*>(plane_ptr(r, slot, 1) + off) = Lo;
  };

  // LOAD: rows past M are zero
#pragma unroll
  for (int r = 0; r < RT; ++r) slot_write(r, 0, lr, lc, xv[r]);
  lds_barrier();

  // accumulator layout of this lane: row l15 of the tile, columns 16 wave + 4 lg .. + 3
  const int n0 = wave * 16 + (lg << 2);
  bool ok[RT];
  uint32_t off[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    ok[r] = row0 + 16 * r + l15 < M;
    off[r] = (uint32_t)(row0 + 16 * r + l15) * (uint32_t)SW + (uint32_t)n0;   // M <= 4 096 rows
  }
  const int my = sw_off(l15, n0);

  auto gemm = [&](auto jc) {
    constexpr int j = decltype(jc)::value;
    constexpr bool tail = j >= NM;
    constexpr bool second = !tail && j > 0 && (j & 1) == 0;     // second GEMM of a ResidualLayer: residual, scale
    constexpr bool last = j == NM - 1;
    constexpr int a_slot = tail ? 1 : (j & 1);
    constexpr int y_slot = a_slot ^ 1;
    // every operand of the op is requested before its first MFMA
    uint4 xf[RT][4][2];
    uint2 rH[RT], rL[RT];
    float4 q2[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      const unsigned char* xb = smem + r * TILE + a_slot * SLOT + l15 * ROWB;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const unsigned char* xp = xb + ((((c << 2) | lg) ^ l15) << 4);
        xf[r][c][0] = *reinterpret_cast<const uint4*>(xp);
        xf[r][c][1] = *reinterpret_cast<const uint4*>(xp + PLANE);
      }
      rH[r] = make_uint2(0u, 0u); rL[r] = make_uint2(0u, 0u);
      if constexpr (second) {
        rH[r] = *reinterpret_cast<const uint2*>(plane_ptr(r, y_slot, 0) + my);
        rL[r] = *reinterpret_cast<const uint2*>(plane_ptr(r, y_slot, 1) + my);
      }
      q2[r] = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (last && RES2) {
        if (ok[r]) q2[r] = *reinterpret_cast<const float4*>(P.res2 + off[r]);
      }
    }
    v4f acc[RT][3];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[r][k] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f16x8 ah = __builtin_bit_cast(f16x8, w[j][c][0]), al = __builtin_bit_cast(f16x8, w[j][c][1]);
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        const f16x8 yh = __builtin_bit_cast(f16x8, xf[r][c][0]), yl = __builtin_bit_cast(f16x8, xf[r][c][1]);
        if constexpr (AS_EXP == 3) {      // (the operands stay live: one add per fragment)
          acc[r][0][0] += __uint_as_float(w[j][c][0].x ^ xf[r][c][0].x); acc[r][1][0] += __uint_as_float(w[j][c][0].y ^ xf[r][c][1].y);
          acc[r][2][0] += __uint_as_float(w[j][c][1].z ^ xf[r][c][0].z);
          continue;
        }
        acc[r][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, yh, acc[r][0], 0, 0, 0);
        acc[r][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, yl, acc[r][1], 0, 0, 0);
        acc[r][2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, yh, acc[r][2], 0, 0, 0);
      }
    }
    float4 v[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      const v4f corr = acc[r][1] + acc[r][2];
      v[r] = make_float4(as_fma(corr[0], H_DOWN, acc[r][0][0]), as_fma(corr[1], H_DOWN, acc[r][0][1]),
                         as_fma(corr[2], H_DOWN, acc[r][0][2]), as_fma(corr[3], H_DOWN, acc[r][0][3]));
    }
    wload(std::integral_constant<int, j + AS_AHEAD>{});     // this op's fragments are dead
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      float4& vr = v[r];
      if constexpr (tail) {
        if (ok[r]) *reinterpret_cast<float4*>(P.t[j - NM] + off[r]) = vr;
      } else {
        // the activation and its derivative from one sigmoid; the factor is what the adjoint multiplies by
        float4 d;
        if constexpr (AS_EXP == 2) {
          d = vr;
        } else {
          as_ssilu_pair(vr.x, vr.x, d.x); as_ssilu_pair(vr.y, vr.y, d.y);
          as_ssilu_pair(vr.z, vr.z, d.z); as_ssilu_pair(vr.w, vr.w, d.w);
        }
        if (ok[r]) *reinterpret_cast<float4*>(P.z[j] + rg + off[r]) = d;
        if constexpr (second) {
          const float4 q = join4h(rH[r], rL[r]);
          const float b = P.s;
          vr.x = (vr.x + q.x) * b; vr.y = (vr.y + q.y) * b; vr.z = (vr.z + q.z) * b; vr.w = (vr.w + q.w) * b;
        }
        if constexpr (last && RES2) {
          if (ok[r]) {
            const float b = P.beta2;
            vr.x = (vr.x + q2[r].x) * b; vr.y = (vr.y + q2[r].y) * b; vr.z = (vr.z + q2[r].z) * b; vr.w = (vr.w + q2[r].w) * b;
          }
        }
        if constexpr (last) {
          if (ok[r]) *reinterpret_cast<float4*>(P.y + rg + off[r]) = vr;
        }
        if constexpr (!last || T > 0) {      // somebody reads the tile again
          slot_write(r, y_slot, l15, n0, ok[r] ? vr : make_float4(0.f, 0.f, 0.f, 0.f));
        }
      }
    }
    if constexpr (!tail && (!last || T > 0) && AS_EXP != 4) lds_barrier();
  };
  gemm(std::integral_constant<int, 0>{});
  if constexpr (NG > 1) gemm(std::integral_constant<int, 1>{});
  if constexpr (NG > 2) gemm(std::integral_constant<int, 2>{});
  if constexpr (NG > 3) gemm(std::integral_constant<int, 3>{});
  if constexpr (NG > 4) gemm(std::integral_constant<int, 4>{});
  if constexpr (NG > 5) gemm(std::integral_constant<int, 5>{});
  if constexpr (NG > 6) gemm(std::integral_constant<int, 6>{});
}

template <int L, int T, bool RES2>
int launch_fwd(const as_fwd_args& a, hipStream_t st) {
  hipLaunchKernelGGL((atom_stack_fwd_kernel<L, T, RES2, false, 1>), dim3((unsigned)gn_cdiv(a.M, 16)), dim3(NT), 0, st, a);
  GN_LAUNCH_CHECK();
  return 0;
}

template <int L, int T>
int launch_fwd_res(const as_fwd_args& a, hipStream_t st) {
  if constexpr (L > 0) {
    if (a.res2) return launch_fwd<L, T, true>(a, st);
  }
  return launch_fwd<L, T, false>(a, st);
}

template <int L>
int launch_fwd_tails(const as_fwd_args& a, int tails, hipStream_t st) {
  switch (tails) {
    case 0: return launch_fwd_res<L, 0>(a, st);
    case 1: return launch_fwd_res<L, 1>(a, st);
    default: return launch_fwd_res<L, 2>(a, st);
  }
}

template <int L>
int launch_fwd_grouped(const as_fwd_args& a, int groups, hipStream_t st) {
  hipLaunchKernelGGL((atom_stack_fwd_kernel<L, 0, false, true, AS_GROUP_TILES>), dim3((unsigned)gn_cdiv(a.M, 16 * AS_GROUP_TILES), (unsigned)groups),
                     dim3(NT), 0, st, a);
  GN_LAUNCH_CHECK();
  return 0;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ------------------------------------------------------------------------------------------------------------- adjoint
// The first-order adjoint of the stack (gn_atom_stack_bwd_f32): the fused program of ops._Stack.backward, a LINEAR program, which
// chain_split_kernel<1, 2, true, true> runs in the row-scaled form of the two fp16 planes (meta & 0x100 there).  The program's
// two LDS slots are used very differently: slot 1 (X) is the operand of every GEMM, slot 0 (G, the running gradient) is only
// ever read and rewritten element by element (residual of a GEMM, stand-alone SCALE).  So here
//   * G lives in registers in accumulator layout AS ITS TWO PLANES plus its row scale: what the interpreter writes to the slot
//     and reads back is split and joined at the same places under the same power-of-two scale, it just never travels;
//   * X rotates through three LDS tiles, so that an op may write its output (or second output) while slower waves still read
//     its operand: one barrier per op and none in front of an epilogue, none behind a tail GEMM that only updates G;
//   * the stand-alone SCALE ops behind the last tail GEMM (the form with a skip gradient of its own) run inside its epilogue;
//   * all LOADs sit in front of the first barrier; the stored factor of an op is requested in front of its first MFMA.
// Arithmetic in the interpreter's order: acc -> * 1 / sigma(operand) -> * mul -> (+ residual) * beta -> out -> * sigma(result),
// split; second output = Z2 * v.  Every multiplication that the interpreter's compiler may or may not have contracted with an
// addition is one by a power of two, exact either way; contraction stays off in this file.
// Knock-outs of diagnosis builds (never defined in the product library; tools/atom_stack_bwd_bench.py):
//   AS_BWD_EXP == 1  no weight fetch      AS_BWD_EXP == 2  no factor loads (ones)
//   AS_BWD_EXP == 3  no row-scale reductions (sigma = 1)      AS_BWD_EXP == 4  no barriers between the ops (timing only)
#ifndef AS_BWD_EXP
#define AS_BWD_EXP 0
#endif
#ifndef AS_BWD_AHEAD
// Weight sets in flight or resident ahead of the running op.  Measured at M = 1 024 (us per launch, form A / B / no tails):
// 1 -> 7.21 / 7.01 / 5.49, 2 -> 7.43 / 7.14 / 5.66, 3 -> 7.59 / 7.33 / 5.73 (profiles/atom_stack_bwd_timeline.txt): as in the
// forward, what is requested early delays the fragments the first op waits for; one set ahead is the least that hides a fetch.
#define AS_BWD_AHEAD 1
#endif

struct as_bwd_args {
  const float* g;
  const float* gt[2];              // cotangents of the tails
  int M;
  const uint4* W[AS_MAX_GEMMS];    // packed transposed planes in program order
  const float* F[5];               // stored factors in the order of use
  float alpha0, a_out, a_s;        // LOAD alpha; SCALE with the skip output (T = 0, form A); plain SCALE of form A
  float bt[2], bl[2];              // beta of the tail GEMMs / of the second GEMM of every layer, program order
  float* g_skip;
  float* gx;
  int pitch;                       // grouped launch: rows between the groups' slabs of g, F, gx
  const float* g_E;                // grouped launch with the seed formed in the LOAD: g[grp, a, :] = g_E[a] * w_out[grp, :]
  const float* w_out;
};

__device__ __forceinline__ float4 as_mul4(const float4 v, const float a) { return make_float4(v.x * a, v.y * a, v.z * a, v.w * a); }

// One template for the single and the grouped launch, as in the forward.  L ResidualLayers, T tails, A: the skip gradient is an
// output of its own (SCALE ops stay stand-alone in the fused program).  GR (gn_atom_stack_bwd_grouped_f32): groups laid out as in
// the forward; SEED: the cotangent is not a tensor but the product the energy head's adjoint would have written, formed here
// from g_E (M,1) and w_out (groups,128); RT: 16-row tiles of one workgroup as in the forward (every tile has its own four LDS
// tiles, row scales and G registers)
template <int L, int T, bool A, bool GR, bool SEED, int RT>
__global__ __launch_bounds__(NT) void atom_stack_bwd_kernel(const as_bwd_args P) {
  static_assert(L >= 1 && L <= 2 && (T == 0 || T == 2), "adjoint programs of the atom stack");
  static_assert((!GR || (T == 0 && !A)) && (!SEED || GR), "adjoint programs of the grouped output blocks");
  static_assert(RT == 1 || (GR && RT == 2), "one row tile, or two in the grouped launch");
  constexpr int NG = T + 2 * L + 1;
  constexpr int PLANE = 16 * ROWB;
  constexpr int SLOT = 2 * PLANE;
  constexpr int TILE = 4 * SLOT;                                            // LDS of one row tile
  __shared__ __attribute__((aligned(16))) unsigned char smem[RT * TILE];    // per tile: G (once, to change layout) | X0 X1 X2
  __shared__ float rs[RT][3][16];                                           // row scales of the LOADs: g, gt[0], gt[1]
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int l15 = lane & 15;
  const int lg = lane >> 4;
  const int M = P.M;
  const int row0 = (int)blockIdx.x * (16 * RT);
  size_t rg = 0, wg = 0;                     // this group's offset into the row operands (floats) / the weights (uint4)
  if constexpr (GR) {
    rg = (size_t)blockIdx.y * (size_t)P.pitch * SW;
    wg = (size_t)blockIdx.y * AS_W_UINT4;
  }

  uint4 w[NG][4][2];
  auto wload = [&](auto jc) {
    constexpr int j = decltype(jc)::value;
    if constexpr (j < NG) {
      const uint4* __restrict__ const base = P.W[j] + wg + (size_t)wave * (4 * 2 * 64) + lane;
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int p = 0; p < 2; ++p) w[j][c][p] = AS_BWD_EXP == 1 ? make_uint4(0x3c003c00u + lane, 0u, 0u, 0u) : base[(c * 2 + p) * 64];
    }
  };
  auto plane_ptr = [&](int r, int buf, int p) -> unsigned char* { return smem + r * TILE + buf * SLOT + p * PLANE; };      // buf 0: G, 1 + i: X_i
  auto sw_off = [&](int row, int col) -> int { return row * ROWB + ((((col >> 3) ^ row) & 15) << 4) + ((col & 4) << 1); };
  auto put_planes = [&](int r, int buf, int off, const uint2 H, const uint2 Lo) {
    *reinterpret_cast<uint2*>(plane_ptr(r, buf, 0) + off) = H;
    *reinterpret_cast<uint2*>(plane_ptr(r, buf, 1) + off) = Lo;
  };
  auto sigma_of = [&](const float4 v) -> float {      // row scale of a LOAD: one row = 32 consecutive lanes
    if constexpr (AS_BWD_EXP == 3) return 1.f;
    const float m = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
    return row_sigma(group_max(m, 32));
  };
  // a stand-alone SCALE of the interpreter on planes held in registers: read (join), * alpha / sigma, [* Z]; the caller
  // stores the true-scale value where the op has an output and splits value * sigma again
  auto scale_read = [&](const uint2 H, const uint2 Lo, const float alpha, const float sc) -> float4 {
    return as_mul4(join4h(H, Lo), alpha * inv_pow2(sc));
  };

  // ---- the LOADs (linear layout: 16 rows x 32 float4, one per thread and tile); the rows are requested first
  const int lr = tid >> 5, lc = (tid & 31) << 2;
  bool in[RT];
  size_t loff[RT];
  float4 gv[RT], tv0[RT], tv1[RT], zv[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    in[r] = row0 + 16 * r + lr < M;
    loff[r] = rg + (size_t)(row0 + 16 * r + lr) * SW + lc;
    gv[r] = make_float4(0.f, 0.f, 0.f, 0.f); tv0[r] = gv[r]; tv1[r] = gv[r]; zv[r] = gv[r];
    if (in[r]) {
      if constexpr (SEED) {
        // one fp32 product per element, as energy_head_bwd_kernel rounds it; the LOAD's alpha, row maximum, row scale and
        // split below take it like a value read from memory
        const float ge = P.g_E[row0 + 16 * r + lr];
        const float4 wv = *reinterpret_cast<const float4*>(P.w_out + (size_t)blockIdx.y * SW + lc);
        gv[r] = make_float4(ge * wv.x, ge * wv.y, ge * wv.z, ge * wv.w);
      } else {
        gv[r] = *reinterpret_cast<const float4*>(P.g + loff[r]);
      }
      if constexpr (T > 0) tv0[r] = *reinterpret_cast<const float4*>(P.gt[0] + loff[r]);
      if constexpr (T > 1) tv1[r] = *reinterpret_cast<const float4*>(P.gt[1] + loff[r]);
      if constexpr (T == 0) zv[r] = AS_BWD_EXP == 2 ? make_float4(1.f, 1.f, 1.f, 1.f) : *reinterpret_cast<const float4*>(P.F[0] + loff[r]);
    }
  }
  wload(std::integral_constant<int, 0>{});
  if constexpr (AS_BWD_AHEAD > 1) wload(std::integral_constant<int, 1>{});
  if constexpr (AS_BWD_AHEAD > 2) wload(std::integral_constant<int, 2>{});
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    const int o = sw_off(lr, lc);
    const float4 v = as_mul4(gv[r], P.alpha0);
    const float sig = sigma_of(v);
    uint2 H, Lo;
    split4h(as_mul4(v, sig), H, Lo);
    if (lc == 0) rs[r][0][lr] = sig;
    if constexpr (T == 0) {
      if constexpr (A) {
        // SCALE 0 <- 0 * a_out with the skip gradient as its output, SCALE 0 <- 0 * a_s, SCALE 1 <- 0 * Z
        float4 u = scale_read(H, Lo, P.a_out, sig);
        if (in[r]) *reinterpret_cast<float4*>(P.g_skip + loff[r]) = u;
        split4h(as_mul4(u, sig), H, Lo);
        u = scale_read(H, Lo, P.a_s, sig);
        split4h(as_mul4(u, sig), H, Lo);
        put_planes(r, 0, o, H, Lo);
        u = scale_read(H, Lo, 1.f, sig);
        if (in[r]) { u.x *= zv[r].x; u.y *= zv[r].y; u.z *= zv[r].z; u.w *= zv[r].w; }
        split4h(as_mul4(u, sig), H, Lo);
        put_planes(r, 1, o, H, Lo);
      } else {
        // the LOAD's second tensor: v * alpha2 (1) * Z2
        put_planes(r, 0, o, H, Lo);
        float4 u = v;
        if (in[r]) { u.x *= zv[r].x; u.y *= zv[r].y; u.z *= zv[r].z; u.w *= zv[r].w; }
        split4h(as_mul4(u, sig), H, Lo);
        put_planes(r, 1, o, H, Lo);
      }
    } else {
      put_planes(r, 0, o, H, Lo);
      const float s0 = sigma_of(tv0[r]);
      split4h(as_mul4(tv0[r], s0), H, Lo);
      put_planes(r, 1, o, H, Lo);
      if (lc == 0) rs[r][1][lr] = s0;
      if constexpr (T > 1) {
        const float s1 = sigma_of(tv1[r]);
        split4h(as_mul4(tv1[r], s1), H, Lo);
        put_planes(r, 2, o, H, Lo);
        if (lc == 0) rs[r][2][lr] = s1;
      }
    }
  }
  lds_barrier();

  // accumulator layout of this lane: row l15 of the tile, columns 16 wave + 4 lg .. + 3
  const int n0 = wave * 16 + (lg << 2);
  const int my = sw_off(l15, n0);
  bool ok[RT];
  uint32_t off[RT];
  // G: its planes and its row scale, from here on in registers; rs1: the row scale of X
  uint2 GH[RT], GL[RT];
  float rs0[RT], rs1[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    ok[r] = row0 + 16 * r + l15 < M;
    off[r] = (uint32_t)(row0 + 16 * r + l15) * (uint32_t)SW + (uint32_t)n0;   // M <= 4 096 rows
    GH[r] = *reinterpret_cast<const uint2*>(plane_ptr(r, 0, 0) + my);
    GL[r] = *reinterpret_cast<const uint2*>(plane_ptr(r, 0, 1) + my);
    rs0[r] = rs[r][0][l15];
    rs1[r] = rs0[r];
  }

  auto gemm = [&](auto jc) {
    constexpr int j = decltype(jc)::value;
    constexpr bool tail = j < T;
    constexpr bool fin = j == NG - 1;
    constexpr int m = j - T;                                       // main GEMMs: even = first of a layer's adjoint (mul), odd = second
    constexpr bool mulop = !tail && !fin && (m & 1) == 0;
    constexpr bool resop = tail || (!fin && (m & 1) == 1);         // (. + G) * beta
    constexpr bool scales = tail && j == T - 1 && A;               // out = g_skip and the two SCALE ops
    constexpr bool second = resop && !scales && !(tail && j < T - 1);      // second output Z2 * v -> X
    constexpr int fi = tail ? 0 : 1 + m;                           // stored factor of this op
    constexpr bool factor = mulop || second || scales;
    constexpr int a_buf = 1 + j % 3, y_buf = 1 + (j + 1) % 3;
    // every operand of the op is requested before its first MFMA
    uint4 xf[RT][4][2];
    float sa[RT];
    float4 fz[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      const unsigned char* xb = smem + r * TILE + a_buf * SLOT + l15 * ROWB;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const unsigned char* xp = xb + ((((c << 2) | lg) ^ l15) << 4);
        xf[r][c][0] = *reinterpret_cast<const uint4*>(xp);
        xf[r][c][1] = *reinterpret_cast<const uint4*>(xp + PLANE);
      }
      sa[r] = rs1[r];
      if constexpr (tail) sa[r] = rs[r][1 + j][l15];
      fz[r] = mulop ? make_float4(1.f, 1.f, 1.f, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (factor) {
        if (ok[r]) fz[r] = AS_BWD_EXP == 2 ? make_float4(1.f, 1.f, 1.f, 1.f) : *reinterpret_cast<const float4*>(P.F[fi] + rg + off[r]);
      }
    }
    v4f acc[RT][3];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[r][k] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f16x8 ah = __builtin_bit_cast(f16x8, w[j][c][0]), al = __builtin_bit_cast(f16x8, w[j][c][1]);
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        const f16x8 yh = __builtin_bit_cast(f16x8, xf[r][c][0]), yl = __builtin_bit_cast(f16x8, xf[r][c][1]);
        acc[r][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, yh, acc[r][0], 0, 0, 0);
        acc[r][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, yl, acc[r][1], 0, 0, 0);
        acc[r][2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, yh, acc[r][2], 0, 0, 0);
      }
    }
    float4 vv[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      const v4f corr = acc[r][1] + acc[r][2];
      vv[r] = make_float4(as_fma(corr[0], H_DOWN, acc[r][0][0]), as_fma(corr[1], H_DOWN, acc[r][0][1]),
                          as_fma(corr[2], H_DOWN, acc[r][0][2]), as_fma(corr[3], H_DOWN, acc[r][0][3]));
    }
    wload(std::integral_constant<int, j + AS_BWD_AHEAD>{});     // this op's fragments are dead
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      float4 v = as_mul4(vv[r], inv_pow2(sa[r]));                 // the products are sigma(operand) times the true values
      if constexpr (fin) {
        if (ok[r]) *reinterpret_cast<float4*>(P.gx + rg + off[r]) = v;
      } else if constexpr (mulop) {
        v.x *= fz[r].x; v.y *= fz[r].y; v.z *= fz[r].z; v.w *= fz[r].w;
        uint2 H, Lo;
        split4h(ok[r] ? as_mul4(v, sa[r]) : make_float4(0.f, 0.f, 0.f, 0.f), H, Lo);
        put_planes(r, y_buf, my, H, Lo);
        rs1[r] = sa[r];
      } else {
        // what the op leaves behind takes the smaller scale (the larger magnitude) of its operand and of G
        const float sy = fminf(sa[r], rs0[r]);
        const float4 q = as_mul4(join4h(GH[r], GL[r]), inv_pow2(rs0[r]));
        const float b = tail ? P.bt[tail ? j : 0] : P.bl[tail ? 0 : (m >> 1)];
        v.x = (v.x + q.x) * b; v.y = (v.y + q.y) * b; v.z = (v.z + q.z) * b; v.w = (v.w + q.w) * b;
        if constexpr (scales) {
          if (ok[r]) *reinterpret_cast<float4*>(P.g_skip + off[r]) = v;
        }
        split4h(ok[r] ? as_mul4(v, sy) : make_float4(0.f, 0.f, 0.f, 0.f), GH[r], GL[r]);
        rs0[r] = sy;
        if constexpr (scales) {
          // SCALE 0 <- 0 * a_s and SCALE 1 <- 0 * Z of the interpreter, on the planes just written
          float4 u = scale_read(GH[r], GL[r], P.a_s, sy);
          split4h(as_mul4(u, sy), GH[r], GL[r]);
          u = scale_read(GH[r], GL[r], 1.f, sy);
          if (ok[r]) { u.x *= fz[r].x; u.y *= fz[r].y; u.z *= fz[r].z; u.w *= fz[r].w; }
          uint2 H, Lo;
          split4h(as_mul4(u, sy), H, Lo);
          put_planes(r, y_buf, my, H, Lo);
        } else if constexpr (second) {
          float4 u = fz[r];
          u.x *= v.x; u.y *= v.y; u.z *= v.z; u.w *= v.w;
          uint2 H, Lo;
          split4h(ok[r] ? as_mul4(u, sy) : make_float4(0.f, 0.f, 0.f, 0.f), H, Lo);
          put_planes(r, y_buf, my, H, Lo);
        }
        if constexpr (scales || second) rs1[r] = sy;
      }
    }
    if constexpr (!fin && (mulop || scales || second) && AS_BWD_EXP != 4) lds_barrier();
  };
  gemm(std::integral_constant<int, 0>{});
  gemm(std::integral_constant<int, 1>{});
  gemm(std::integral_constant<int, 2>{});
  if constexpr (NG > 3) gemm(std::integral_constant<int, 3>{});
  if constexpr (NG > 4) gemm(std::integral_constant<int, 4>{});
  if constexpr (NG > 5) gemm(std::integral_constant<int, 5>{});
  if constexpr (NG > 6) gemm(std::integral_constant<int, 6>{});
}

template <int L, int T, bool A>
int launch_bwd(const as_bwd_args& a, hipStream_t st) {
  hipLaunchKernelGGL((atom_stack_bwd_kernel<L, T, A, false, false, 1>), dim3((unsigned)gn_cdiv(a.M, 16)), dim3(NT), 0, st, a);
  GN_LAUNCH_CHECK();
  return 0;
}

template <int L>
int launch_bwd_form(const as_bwd_args& a, int tails, int form, hipStream_t st) {
  if (tails == 0) return form ? launch_bwd<L, 0, true>(a, st) : launch_bwd<L, 0, false>(a, st);
  return form ? launch_bwd<L, 2, true>(a, st) : launch_bwd<L, 2, false>(a, st);
}

template <int L>
int launch_bwd_grouped(const as_bwd_args& a, int groups, hipStream_t st) {
  const dim3 grid((unsigned)gn_cdiv(a.M, 16 * AS_GROUP_TILES), (unsigned)groups);
  if (a.g_E) {
    hipLaunchKernelGGL((atom_stack_bwd_kernel<L, 0, false, true, true, AS_GROUP_TILES>), grid, dim3(NT), 0, st, a);
  } else {
    hipLaunchKernelGGL((atom_stack_bwd_kernel<L, 0, false, true, false, AS_GROUP_TILES>), grid, dim3(NT), 0, st, a);
  }
  GN_LAUNCH_CHECK();
  return 0;
}

// the argument checks the two grouped entry points share
bool grouped_shape_ok(int M, int groups, int group_pitch, int layers) {
  return M <= AS_MAX_ROWS && groups >= 1 && groups <= AS_MAX_GROUPS && group_pitch >= M && layers >= 1 && layers <= 2;
}

}  // namespace

extern "C" int gn_atom_stack_fwd_f32(const float* x, int M, int layers, int tails, const void* const* W, float* const* z,
                                     float s, const float* res2, float beta2, float* y, float* const* t, void* stream) {
  if (M <= 0) return 0;
  if (M > AS_MAX_ROWS || layers < 0 || layers > 2 || tails < 0 || tails > 2) return (int)hipErrorInvalidValue;
  if (!x || !y || !W || !z || (tails && !t) || (res2 && layers == 0)) return (int)hipErrorInvalidValue;
  if (!aligned16(x) || !aligned16(y) || !aligned16(res2)) return (int)hipErrorInvalidValue;
  as_fwd_args a = {};
  a.x = x; a.M = M; a.s = s; a.res2 = res2; a.beta2 = beta2; a.y = y;
  const int nm = 1 + 2 * layers;
  for (int j = 0; j < nm + tails; ++j) {
    if (!W[j] || !aligned16(W[j])) return (int)hipErrorInvalidValue;
    a.W[j] = static_cast<const uint4*>(W[j]);
  }
  for (int j = 0; j < nm; ++j) {
    if (!z[j] || !aligned16(z[j])) return (int)hipErrorInvalidValue;
    a.z[j] = z[j];
  }
  for (int j = 0; j < tails; ++j) {
    if (!t[j] || !aligned16(t[j])) return (int)hipErrorInvalidValue;
    a.t[j] = t[j];
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (layers) {
    case 0: return launch_fwd_tails<0>(a, tails, st);
    case 1: return launch_fwd_tails<1>(a, tails, st);
    default: return launch_fwd_tails<2>(a, tails, st);
  }
}

extern "C" int gn_atom_stack_bwd_f32(const float* g, int M, int layers, int tails, int form, const float* const* gt,
                                     const void* const* W, const float* const* F, float alpha0, float a_out, float a_s, float bt0,
                                     float bt1, float bl0, float bl1, float* g_skip, float* gx, void* stream) {
  if (M <= 0) return 0;
  if (M > AS_MAX_ROWS || layers < 1 || layers > 2 || (tails != 0 && tails != 2) || form < 0 || form > 1) return (int)hipErrorInvalidValue;
  if (!g || !gx || !W || !F || (tails && !gt) || (form == 1) != (g_skip != nullptr)) return (int)hipErrorInvalidValue;
  if (!aligned16(g) || !aligned16(gx) || !aligned16(g_skip)) return (int)hipErrorInvalidValue;
  as_bwd_args a = {};
  a.g = g; a.M = M; a.alpha0 = alpha0; a.a_out = a_out; a.a_s = a_s; a.g_skip = g_skip; a.gx = gx;
  a.bt[0] = bt0; a.bt[1] = bt1; a.bl[0] = bl0; a.bl[1] = bl1;
  for (int j = 0; j < tails; ++j) {
    if (!gt[j] || !aligned16(gt[j])) return (int)hipErrorInvalidValue;
    a.gt[j] = gt[j];
  }
  for (int j = 0; j < tails + 2 * layers + 1; ++j) {
    if (!W[j] || !aligned16(W[j])) return (int)hipErrorInvalidValue;
    a.W[j] = static_cast<const uint4*>(W[j]);
  }
  for (int j = 0; j < 2 * layers + 1; ++j) {
    if (!F[j] || !aligned16(F[j])) return (int)hipErrorInvalidValue;
    a.F[j] = F[j];
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  return layers == 1 ? launch_bwd_form<1>(a, tails, form, st) : launch_bwd_form<2>(a, tails, form, st);
}

extern "C" int gn_atom_stack_fwd_grouped_f32(const float* x, int M, int groups, int group_pitch, int layers, const void* const* W,
                                             float* const* z, float s, float* y, void* stream) {
  if (M <= 0) return 0;
  if (!grouped_shape_ok(M, groups, group_pitch, layers)) return (int)hipErrorInvalidValue;
  if (!x || !y || !W || !z || !aligned16(x) || !aligned16(y)) return (int)hipErrorInvalidValue;
  as_fwd_args a = {};
  a.x = x; a.M = M; a.s = s; a.beta2 = 1.f; a.y = y; a.pitch = group_pitch;
  for (int j = 0; j < 1 + 2 * layers; ++j) {
    if (!W[j] || !aligned16(W[j]) || !z[j] || !aligned16(z[j])) return (int)hipErrorInvalidValue;
    a.W[j] = static_cast<const uint4*>(W[j]);
    a.z[j] = z[j];
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  return layers == 1 ? launch_fwd_grouped<1>(a, groups, st) : launch_fwd_grouped<2>(a, groups, st);
}

extern "C" int gn_atom_stack_bwd_grouped_f32(const float* g, const float* g_E, const float* w_out, int M, int groups,
                                             int group_pitch, int layers, const void* const* W, const float* const* F,
                                             float alpha0, float bl0, float bl1, float* gx, void* stream) {
  if (M <= 0) return 0;
  if (!grouped_shape_ok(M, groups, group_pitch, layers)) return (int)hipErrorInvalidValue;
  // the cotangent is either a tensor or the seed pair, never both
  if ((g != nullptr) == (g_E != nullptr) || (g_E != nullptr) != (w_out != nullptr)) return (int)hipErrorInvalidValue;
  if (!gx || !W || !F || !aligned16(g) || !aligned16(w_out) || !aligned16(gx)) return (int)hipErrorInvalidValue;
  as_bwd_args a = {};
  a.g = g; a.g_E = g_E; a.w_out = w_out; a.M = M; a.pitch = group_pitch; a.alpha0 = alpha0; a.a_out = 1.f; a.a_s = 1.f; a.gx = gx;
  a.bt[0] = 1.f; a.bt[1] = 1.f; a.bl[0] = bl0; a.bl[1] = bl1;
  for (int j = 0; j < 2 * layers + 1; ++j) {
    if (!W[j] || !aligned16(W[j]) || !F[j] || !aligned16(F[j])) return (int)hipErrorInvalidValue;
    a.W[j] = static_cast<const uint4*>(W[j]);
    a.F[j] = F[j];
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  return layers == 1 ? launch_bwd_grouped<1>(a, groups, st) : launch_bwd_grouped<2>(a, groups, st);
}
