"""Thin launchers: torch tensors in, torch tensors out, one C-ABI call each (include/gemnet_hip.h).

PyTorch only provides device memory and the current stream here.  No fallbacks: CPU tensors or a
missing library raise.  (tests/cpu_kernels.py monkeypatches these launchers with CPU
restatements to exercise the autograd/model logic on machines without a GPU; that emulation
lives under tests/ and is never imported by the product.)
"""
import contextlib
import ctypes
import functools
import os
import threading

import torch

from . import _lib
from ._lib import (GN_ANG_F16, GN_CHAIN_MAX_GROUPS, GN_CHAIN_MAX_OPS, GN_CHAIN_ROW, GN_SPLIT_F16X2_ROW, GemmArgs, addr, check, ptr,
                   require_device, stream)


def _f32c(t):
    if t.dtype != torch.float32:
        raise TypeError(f"HIP path is fp32; got {t.dtype}")
    return t.contiguous()


def _rowmajor(t):
    """2-D fp32 operand with unit inner stride (row slices of a weight are passed in place)."""
    if t.dtype != torch.float32:
        raise TypeError(f"HIP path is fp32; got {t.dtype}")
    if t.dim() != 2:
        raise ValueError("2-D operand expected")
    if t.shape[0] > 0 and t.shape[1] > 0 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t
    return t.contiguous()


def _rowsize(t):
    c = 1
    for s in t.shape[1:]:
        c *= int(s)
    return c

def gemm(A, B, trans_a=False, trans_b=False, *, a_dact_pre=None, act=False, pre_out=False,
         mul=None, alpha=1.0, res=None, beta=1.0, gadd1=None, gidx1=None, gadd2=None, gidx2=None,
         ridx=None, res2=None, beta2=1.0, cfg=-1, out=None):
    """C = epilogue(opA(A) @ opB(B)); see gn_gemm_f32 in include/gemnet_hip.h.
    trans_b=False means B is a torch Linear weight (N, K).  Returns C or (C, pre).
    `out`: write C there instead of into a new tensor; `out is res2` accumulates in place (every element is read and
    rewritten by the same thread)."""
    require_device(A, B)
    if (trans_a and trans_b and cfg < 0 and a_dact_pre is None and not act and not pre_out and mul is None
            and res is None and res2 is None and gadd1 is None and gadd2 is None):
        return gemm_tn(A, B, alpha)
    A, B = _rowmajor(A), _rowmajor(B)
    if B.numel() <= (1 << 20) and (B.stride(0) % 4 or B.data_ptr() % 16) and B.shape[1] % 4 == 0:
        # weight slice with an unaligned row pitch (edge embedding: columns of a (128, 262) matrix): a <= 4 MB copy
        # buys the pipelined kernel instead of the scalar-staging generic one (19 us vs 7 us at M = 1024)
        B = B.contiguous()
    M, K = (A.shape[1], A.shape[0]) if trans_a else (A.shape[0], A.shape[1])
    N, Kb = (B.shape[1], B.shape[0]) if trans_b else (B.shape[0], B.shape[1])
    if K != Kb:
        raise ValueError(f"gemm shape mismatch: {tuple(A.shape)} ta={trans_a} x {tuple(B.shape)} tb={trans_b}")
    if out is not None:
        assert tuple(out.shape) == (M, N) and out.dtype == torch.float32 and out.is_contiguous()
    C = out if out is not None else torch.empty((M, N), device=A.device, dtype=torch.float32)
    pre = torch.empty_like(C) if pre_out else None
    a = GemmArgs()
    a.A, a.B, a.C = ptr(A), ptr(B), ptr(C)
    a.M, a.N, a.K = M, N, K
    a.lda, a.ldb, a.ldc = A.stride(0), B.stride(0), N
    a.trans_a, a.trans_b = int(trans_a), int(trans_b)
    if a_dact_pre is not None:
        a_dact_pre = _f32c(a_dact_pre)
        A = _f32c(A)
        assert a_dact_pre.shape == A.shape
        a.A, a.lda = ptr(A), A.stride(0)
    a.a_dact_pre = ptr(a_dact_pre)
    a.act = int(act)
    a.pre_out = ptr(pre)
    if mul is not None:
        mul = _f32c(mul)
        assert mul.shape == C.shape
    a.mul, a.ldmul = ptr(mul), N
    a.alpha = float(alpha)
    if res is not None:
        res = _f32c(res)
        if ridx is None:
            assert res.shape == C.shape
        else:
            assert res.shape[1] == N and ridx.dtype == torch.int32 and ridx.shape[0] == M
    a.res, a.ldres = ptr(res), N
    a.beta = float(beta)
    a.ridx = ptr(ridx)
    if res2 is not None:
        res2 = _f32c(res2)
        assert res2.shape == C.shape
    a.res2, a.ldres2 = ptr(res2), N
    a.beta2 = float(beta2)
    if gadd1 is not None:
        gadd1 = _f32c(gadd1)
        assert gadd1.shape[1] == N and gidx1.dtype == torch.int32 and gidx1.shape[0] == M
    if gadd2 is not None:
        gadd2 = _f32c(gadd2)
        assert gadd2.shape[1] == N and gidx2.dtype == torch.int32 and gidx2.shape[0] == M
    a.gadd1, a.gidx1 = ptr(gadd1), ptr(gidx1)
    a.gadd2, a.gidx2 = ptr(gadd2), ptr(gidx2)
    a.ldg = N
    # split-K for "weight-gradient shaped" products: few output tiles, very long contraction
    a.splitk, a.splitk_ws = 0, None
    plain = (a_dact_pre is None and not act and not pre_out and mul is None and res is None and res2 is None
             and gadd1 is None and gadd2 is None)
    tiles = ((M + 31) // 32) * ((N + 127) // 128)
    if plain and K >= 2048 and tiles <= 64:
        splitk = max(2, min(256, K // 128, 1024 // tiles))
        ws = torch.empty((splitk, M, N), device=A.device, dtype=torch.float32)
        a.splitk, a.splitk_ws = splitk, ptr(ws)
    check(_lib.load().gn_gemm_f32_cfg(ctypes.byref(a), int(cfg), stream()), "gn_gemm_f32")
    return (C, pre) if pre_out else C



def gemm_tn(A, B, alpha=1.0, splitk=-1):
    """alpha * A^T @ B for A (K,M), B (K,N): weight-gradient shaped products (split-K, deterministic)."""
    require_device(A, B)
    A, B = _rowmajor(A), _rowmajor(B)
    K, M = A.shape
    N = B.shape[1]
    if B.shape[0] != K:
        raise ValueError(f"gemm_tn shape mismatch: {tuple(A.shape)} x {tuple(B.shape)}")
    lib = _lib.load()
    C = torch.empty((M, N), device=A.device, dtype=torch.float32)
    if splitk < 0:
        splitk = lib.gn_gemm_tn_splitk(M, N, K)
    ws = torch.empty((splitk, M, N), device=A.device, dtype=torch.float32) if splitk > 1 else None
    check(lib.gn_gemm_tn_f32(ptr(A), ptr(B), ptr(C), M, N, K, A.stride(0), B.stride(0), N, float(alpha), ptr(ws),
                             int(splitk), stream()), "gn_gemm_tn_f32")
    return C


def gather(x, idx32):
    require_device(x, idx32)
    x = _f32c(x)
    y = torch.empty((idx32.shape[0],) + tuple(x.shape[1:]), device=x.device, dtype=torch.float32)
    check(_lib.load().gn_gather_rows_f32(ptr(x), ptr(idx32), ptr(y), idx32.shape[0], _rowsize(x), stream()),
          "gn_gather_rows_f32")
    return y


def gather_mul(x, idx32, m, scale=1.0):
    """scale * x[idx] (.) m in one launch (gn_gather_mul_f32)."""
    require_device(x, idx32, m)
    x, m = _f32c(x), _f32c(m)
    assert m.shape[0] == idx32.shape[0] and _rowsize(m) == _rowsize(x)
    y = torch.empty_like(m)
    check(_lib.load().gn_gather_mul_f32(ptr(x), ptr(idx32), ptr(m), ptr(y), idx32.shape[0], _rowsize(x), float(scale), stream()),
          "gn_gather_mul_f32")
    return y


def segsum(y, perm, seg_off, n_rows):
    require_device(y, seg_off)
    y = _f32c(y)
    x = torch.empty((n_rows,) + tuple(y.shape[1:]), device=y.device, dtype=torch.float32)
    check(_lib.load().gn_segsum_rows_f32(ptr(y), ptr(perm), ptr(seg_off), ptr(x), n_rows, _rowsize(y), stream()),
          "gn_segsum_rows_f32")
    return x


def segsum_pair(y, perm1, seg_off1, n_rows1, perm2, seg_off2, n_rows2):
    """-> (segsum(y, perm1, seg_off1, n_rows1), segsum(y, perm2, seg_off2, n_rows2)), bit for bit, in one launch when both
    groupings have at most 4 096 rows (gn_segsum_pair_f32): y is read from memory once.  Host tensors go to `segsum`, which
    refuses them (or, under the tests' CPU restatement of the launchers, sums them)."""
    if not y.is_cuda:
        return segsum(y, perm1, seg_off1, n_rows1), segsum(y, perm2, seg_off2, n_rows2)
    require_device(y, seg_off1, seg_off2)
    y = _f32c(y)
    x1 = torch.empty((n_rows1,) + tuple(y.shape[1:]), device=y.device, dtype=torch.float32)
    x2 = torch.empty((n_rows2,) + tuple(y.shape[1:]), device=y.device, dtype=torch.float32)
    check(_lib.load().gn_segsum_pair_f32(ptr(y), ptr(perm1), ptr(seg_off1), ptr(x1), n_rows1, ptr(perm2), ptr(seg_off2),
                                         ptr(x2), n_rows2, _rowsize(y), stream()), "gn_segsum_pair_f32")
    return x1, x2


def segsum_multi(terms, n_rows):
    """x[n] = sum_k sign_k * segsum(y_k, perm_k, seg_k)[n] for up to 4 terms (y, perm, seg_off, sign) sharing the row
    space, rows of <= 4 floats, in one launch (gn_segsum_multi_f32)."""
    ys = [_f32c(t[0]) for t in terms]
    require_device(*ys)
    C = _rowsize(ys[0])
    assert 1 <= len(terms) <= 4 and C <= 4 and all(_rowsize(y) == C for y in ys)
    n = len(terms)
    x = torch.empty((n_rows,) + tuple(ys[0].shape[1:]), device=ys[0].device, dtype=torch.float32)
    P = ctypes.c_void_p * n
    yp = P(*[ptr(y) for y in ys])
    pp = P(*[ptr(t[1]) for t in terms])
    sp = P(*[ptr(t[2]) for t in terms])
    sg = (ctypes.c_float * n)(*[float(t[3]) for t in terms])
    check(_lib.load().gn_segsum_multi_f32(n, yp, pp, sp, sg, ptr(x), n_rows, C, stream()), "gn_segsum_multi_f32")
    return x


USE_NATIVE_CSR = os.environ.get("GEMNET_NATIVE_CSR", "1") == "1"
USE_NATIVE_EXPANDED = os.environ.get("GEMNET_NATIVE_EXPANDED", "1") == "1"     # graph.expanded_csr through gn_expanded_csr_i32


def expanded_csr(perm_e, seg_e, seg_off_of_edge, n_items):
    """(perm int32 (n_items), seg_off int32 (n_rows + 1)) of items sorted by edge, grouped by the row of their edge, from the edge
    CSR (perm_e or None, seg_e) — gn_expanded_csr_i32 (two launches; graph.expanded_csr's torch form was ~13)."""
    require_device(seg_e, seg_off_of_edge)
    assert seg_e.dtype == torch.int32 and seg_off_of_edge.dtype == torch.int32 and (perm_e is None or perm_e.dtype == torch.int32)
    E, n_rows = int(seg_off_of_edge.shape[0]) - 1, int(seg_e.shape[0]) - 1
    dev = seg_e.device
    perm = torch.empty(int(n_items), dtype=torch.int32, device=dev)
    seg = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(E + 1, dtype=torch.int32, device=dev)
    check(_lib.load().gn_expanded_csr_i32(ptr(perm_e), ptr(seg_e), n_rows, ptr(seg_off_of_edge), E, ptr(perm), ptr(seg), ptr(ws),
                                          stream()), "gn_expanded_csr_i32")
    return perm, seg


def csr_build(idx32, n_rows):
    """(perm int32, seg_off int32 (n_rows + 1)) of the int32 keys `idx32` by row, stable (gn_csr_build_i32: one radix sort over
    the significant key bits + one lower-bound launch; the torch form was argsort + gather + arange + searchsorted + casts)."""
    require_device(idx32)
    assert idx32.dtype == torch.int32 and idx32.dim() == 1
    idx32 = idx32.contiguous()
    n = int(idx32.shape[0])
    lib = _lib.load()
    nbytes = int(lib.gn_csr_ws_bytes(n, int(n_rows)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=idx32.device)
    perm = torch.empty(n, dtype=torch.int32, device=idx32.device)
    seg = torch.empty(int(n_rows) + 1, dtype=torch.int32, device=idx32.device)
    check(lib.gn_csr_build_i32(ptr(idx32), n, int(n_rows), ptr(perm), ptr(seg), ptr(ws), nbytes, stream()), "gn_csr_build_i32")
    return perm, seg


def seg_offsets(sorted_idx32, n_rows):
    """seg_off int32 (n_rows + 1) of SORTED int32 keys (gn_seg_offsets_i32)."""
    require_device(sorted_idx32)
    assert sorted_idx32.dtype == torch.int32
    sorted_idx32 = sorted_idx32.contiguous()
    seg = torch.empty(int(n_rows) + 1, dtype=torch.int32, device=sorted_idx32.device)
    check(_lib.load().gn_seg_offsets_i32(ptr(sorted_idx32), int(sorted_idx32.shape[0]), int(n_rows), ptr(seg), stream()),
          "gn_seg_offsets_i32")
    return seg


def nonfinite_flag(x, flag, bit=1):
    """flag[0] |= bit when x holds an inf / NaN (gn_nonfinite_flag_f32; no host read-back: runtime.RangeFlag)."""
    require_device(x, flag)
    x = x.contiguous()
    assert x.dtype == torch.float32 and flag.dtype == torch.int32
    check(_lib.load().gn_nonfinite_flag_f32(ptr(x), x.numel(), ptr(flag), int(bit), stream()), "gn_nonfinite_flag_f32")


def index_padded_t(builder, R, e_cap, t_cap, a_cap, n_groups, deg_bound, staging, bufs, state):
    """The triplets-only index build of `builder` (index_device.DeviceGraphBuilder) for positions R, straight into the
    capacity-sized arrays `bufs` (id_c, id_a, id_swap, id_undir, id3_reduce_ca, id3_expand_ba: int32) with the dummy
    molecule's pad rows behind the batch — no read-back, capturable (gn_index_gpu_padded_t; state: int32[4], see the header)."""
    require_device(R, staging, state)
    assert builder.triplets_only and R.is_contiguous() and tuple(R.shape) == (builder.A, 3)
    assert staging.dtype == torch.int32 and staging.numel() >= 4 * e_cap + 2 * t_cap and state.dtype == torch.int32
    for k in ("id_c", "id_a", "id_swap", "id_undir"):
        assert bufs[k].dtype == torch.int32 and bufs[k].numel() == e_cap and bufs[k].is_contiguous()
    for k in ("id3_reduce_ca", "id3_expand_ba"):
        assert bufs[k].dtype == torch.int32 and bufs[k].numel() == t_cap and bufs[k].is_contiguous()
    check(_lib.load().gn_index_gpu_padded_t(
        ptr(R), int(R.dtype == torch.float64), ptr(builder.mol_off), ptr(builder.sq_off), builder.B, builder.A, builder.nmax,
        builder.sum_n2, builder.cutoff, ptr(builder.ws), int(e_cap), int(t_cap), int(a_cap), int(n_groups), int(deg_bound),
        ptr(staging), ptr(bufs["id_c"]), ptr(bufs["id_a"]), ptr(bufs["id_swap"]), ptr(bufs["id_undir"]),
        ptr(bufs["id3_reduce_ca"]), ptr(bufs["id3_expand_ba"]), ptr(state), stream()), "gn_index_gpu_padded_t")


def index_cap_ws_bytes(a_cap, n_max, quad=False):
    """Bytes of the workspace gn_index_gpu_padded_tv needs for `a_cap` atom rows of molecules of at most `n_max` atoms: that
    of the triplets-only build with the adjacency blocks at their upper bound a_cap * n_max (gn_index_gpu_ws_bytes).
    `quad=True`: that of the quadruplet build over the same shapes (gn_index_gpu_padded_qv)."""
    a_cap, n_max = int(a_cap), int(n_max)
    if a_cap <= 0 or n_max <= 0 or a_cap * n_max >= 2 ** 31:
        raise ValueError(f"a_cap * n_max = {a_cap * n_max} must be positive and fit int32 (the adjacency blocks)")
    return int(_lib.load().gn_index_gpu_ws_bytes(a_cap, a_cap * n_max, 0 if quad else 1))


def index_layout(N32, n_atoms, n_mol, a_cap, a_tot, n_max, mol_off, sq_off, atom_mol, batch_seg, N_pad, mask, state):
    """The capacity layout of a molecular batch from its molecule sizes ON THE DEVICE (gn_index_gpu_layout): `pbc_layout` plus
    sq_off (n_mol + 1) int32, the exclusive scan of N_b^2, and the bound `n_max` on one molecule — no read-back, capturable.
    Sizes that do not add up to n_atoms, hold a zero, exceed a_cap or hold a molecule above n_max set bit 128 in state[0] /
    state[3] and leave every array as it was."""
    require_device(N32, n_atoms, mol_off, sq_off, atom_mol, batch_seg, N_pad, mask, state)
    n_mol, a_cap, a_tot, n_max = int(n_mol), int(a_cap), int(a_tot), int(n_max)
    assert 0 < n_mol <= a_cap <= a_tot and 0 < n_max and a_cap * n_max < 2 ** 31
    assert N32.dtype == torch.int32 and N32.numel() == n_mol and N32.is_contiguous()
    assert n_atoms.dtype == torch.int32 and n_atoms.numel() == 1
    assert mol_off.dtype == torch.int32 and mol_off.numel() == n_mol + 2 and mol_off.is_contiguous()
    assert sq_off.dtype == torch.int32 and sq_off.numel() == n_mol + 1 and sq_off.is_contiguous()
    assert atom_mol.dtype == torch.int32 and atom_mol.numel() == a_cap and atom_mol.is_contiguous()
    assert batch_seg.dtype == torch.int64 and batch_seg.numel() == a_tot and batch_seg.is_contiguous()
    assert N_pad.dtype == torch.int64 and N_pad.numel() == n_mol + 1 and N_pad.is_contiguous()
    assert mask.dtype == torch.float32 and mask.numel() == a_cap and mask.is_contiguous()
    assert state.dtype == torch.int32 and state.numel() >= 4
    check(_lib.load().gn_index_gpu_layout(ptr(N32), ptr(n_atoms), n_mol, a_cap, a_tot, n_max, ptr(mol_off), ptr(sq_off),
                                          ptr(atom_mol), ptr(batch_seg), ptr(N_pad), ptr(mask), ptr(state), stream()),
          "gn_index_gpu_layout")


def index_padded_tv(builder, R, e_cap, t_cap, a_cap, n_groups, deg_bound, staging, bufs, state):
    """`index_padded_t` for a builder whose layout changes from replay to replay (index_device.DeviceCapacityGraphBuilder): R
    (a_cap,3) — the batch, then the filler atoms — read at replay time with the layout `index_layout` wrote in the same step
    (gn_index_gpu_padded_tv; the builder's ws: index_cap_ws_bytes(a_cap, n_max), staging: int32[4 e_cap + 2 t_cap], state:
    int32[4], see the header)."""
    require_device(R, staging, state, builder.ws)
    assert builder.a_cap == int(a_cap) and builder.B <= int(a_cap)
    assert R.dtype in (torch.float32, torch.float64) and R.is_contiguous() and tuple(R.shape) == (builder.a_cap, 3)
    assert builder.mol_off.numel() == builder.B + 2 and builder.sq_off.numel() == builder.B + 1
    assert builder.atom_mol.numel() == builder.a_cap and builder.atom_mol.dtype == torch.int32
    assert builder.ws.dtype == torch.uint8 and builder.ws.numel() >= index_cap_ws_bytes(builder.a_cap, builder.n_max)
    assert staging.dtype == torch.int32 and staging.numel() >= 4 * e_cap + 2 * t_cap
    assert state.dtype == torch.int32 and state.numel() >= 4
    for k in ("id_c", "id_a", "id_swap", "id_undir"):
        assert bufs[k].dtype == torch.int32 and bufs[k].numel() == e_cap and bufs[k].is_contiguous()
    for k in ("id3_reduce_ca", "id3_expand_ba"):
        assert bufs[k].dtype == torch.int32 and bufs[k].numel() == t_cap and bufs[k].is_contiguous()
    check(_lib.load().gn_index_gpu_padded_tv(
        ptr(R), int(R.dtype == torch.float64), ptr(builder.mol_off), ptr(builder.sq_off), ptr(builder.atom_mol), builder.B,
        builder.n_max, builder.cutoff, ptr(builder.ws), int(e_cap), int(t_cap), int(a_cap), int(n_groups), int(deg_bound),
        ptr(staging), ptr(bufs["id_c"]), ptr(bufs["id_a"]), ptr(bufs["id_swap"]), ptr(bufs["id_undir"]),
        ptr(bufs["id3_reduce_ca"]), ptr(bufs["id3_expand_ba"]), ptr(state), stream()), "gn_index_gpu_padded_tv")


def pbc_index_ws_bytes(n_atoms, e_cap):
    """Bytes of the workspace gn_pbc_index_padded_t needs for `n_atoms` atoms and an edge capacity of `e_cap`."""
    return int(_lib.load().gn_pbc_index_ws_bytes(int(n_atoms), int(e_cap)))


def pbc_index_padded_t(builder, R, cell, e_cap, t_cap, a_cap, n_groups, deg_bound, ws, staging, bufs, state):
    """The image neighbour list of `builder` (pbc.PeriodicGraphBuilder) for positions R (A,3) and `cell` (>= B rows of (3,3)),
    both float32 ON THE DEVICE, straight into the capacity-sized arrays `bufs` (id_c, id_a, id_swap, id_undir, cell_offsets,
    id3_reduce_ca, id3_expand_ba: int32) with the dummy molecule's pad rows behind the batch — no read-back, capturable
    (gn_pbc_index_padded_t; ws: uint8 of pbc_index_ws_bytes(A, e_cap), staging: int32[7 e_cap], state: int32[8], see the
    header)."""
    require_device(R, cell, ws, staging, state)
    assert R.dtype == torch.float32 and R.is_contiguous() and tuple(R.shape) == (builder.A, 3)
    assert cell.dtype == torch.float32 and cell.is_contiguous() and cell.shape[0] >= builder.B and tuple(cell.shape[1:]) == (3, 3)
    assert staging.dtype == torch.int32 and staging.numel() >= 7 * e_cap
    assert state.dtype == torch.int32 and state.numel() >= 8
    assert ws.dtype == torch.uint8 and ws.numel() >= pbc_index_ws_bytes(builder.A, e_cap)
    for k in ("id_c", "id_a", "id_swap", "id_undir"):
        assert bufs[k].dtype == torch.int32 and bufs[k].numel() == e_cap and bufs[k].is_contiguous()
    assert bufs["cell_offsets"].dtype == torch.int32 and tuple(bufs["cell_offsets"].shape) == (e_cap, 3)
    assert bufs["cell_offsets"].is_contiguous()
    for k in ("id3_reduce_ca", "id3_expand_ba"):
        assert bufs[k].dtype == torch.int32 and bufs[k].numel() == t_cap and bufs[k].is_contiguous()
    check(_lib.load().gn_pbc_index_padded_t(
        ptr(R), ptr(cell), ptr(builder.pbc), ptr(builder.mol_off), ptr(builder.atom_mol), builder.B, builder.A, builder.cutoff,
        ptr(ws), int(e_cap), int(t_cap), int(a_cap), int(n_groups), int(deg_bound), ptr(staging), ptr(bufs["id_c"]),
        ptr(bufs["id_a"]), ptr(bufs["id_swap"]), ptr(bufs["id_undir"]), ptr(bufs["cell_offsets"]), ptr(bufs["id3_reduce_ca"]),
        ptr(bufs["id3_expand_ba"]), ptr(state), stream()), "gn_pbc_index_padded_t")


def pbc_layout(N32, n_atoms, n_mol, a_cap, a_tot, mol_off, atom_mol, batch_seg, N_pad, mask, state):
    """The capacity layout of a periodic batch from its structure sizes ON THE DEVICE (gn_pbc_layout; what
    padded.capacity_layout computes): N32 (n_mol) int32, n_atoms (1) int32 -> mol_off (n_mol + 2) int32, atom_mol (a_cap) int32,
    batch_seg (a_tot) int64, N_pad (n_mol + 1) int64, mask (a_cap) float32 — no read-back, capturable.  Sizes that do not add up
    to n_atoms, hold a zero or exceed a_cap set bit 128 in state[0] / state[3] and leave every array as it was."""
    require_device(N32, n_atoms, mol_off, atom_mol, batch_seg, N_pad, mask, state)
    n_mol, a_cap, a_tot = int(n_mol), int(a_cap), int(a_tot)
    assert 0 < n_mol <= a_cap <= a_tot
    assert N32.dtype == torch.int32 and N32.numel() == n_mol and N32.is_contiguous()
    assert n_atoms.dtype == torch.int32 and n_atoms.numel() == 1
    assert mol_off.dtype == torch.int32 and mol_off.numel() == n_mol + 2 and mol_off.is_contiguous()
    assert atom_mol.dtype == torch.int32 and atom_mol.numel() == a_cap and atom_mol.is_contiguous()
    assert batch_seg.dtype == torch.int64 and batch_seg.numel() == a_tot and batch_seg.is_contiguous()
    assert N_pad.dtype == torch.int64 and N_pad.numel() == n_mol + 1 and N_pad.is_contiguous()
    assert mask.dtype == torch.float32 and mask.numel() == a_cap and mask.is_contiguous()
    assert state.dtype == torch.int32 and state.numel() >= 8
    check(_lib.load().gn_pbc_layout(ptr(N32), ptr(n_atoms), n_mol, a_cap, a_tot, ptr(mol_off), ptr(atom_mol), ptr(batch_seg),
                                    ptr(N_pad), ptr(mask), ptr(state), stream()), "gn_pbc_layout")


def pbc_index_padded_tv(builder, R, cell, e_cap, t_cap, a_cap, n_groups, deg_bound, ws, staging, bufs, state):
    """`pbc_index_padded_t` for a builder whose layout changes from replay to replay (pbc.PeriodicCapacityGraphBuilder): R
    (a_cap,3) — the batch, then the filler atoms —, `cell` (n_mol + 1 rows of (3,3)) and the builder's `pbc` (n_mol + 1,3), all
    read at replay time with the layout `pbc_layout` wrote in the same step (gn_pbc_index_padded_tv; ws: uint8 of
    pbc_index_ws_bytes(a_cap, e_cap), staging: int32[7 e_cap], state: int32[8], see the header)."""
    require_device(R, cell, ws, staging, state)
    assert builder.a_cap == int(a_cap) and builder.B <= int(a_cap)
    assert R.dtype == torch.float32 and R.is_contiguous() and tuple(R.shape) == (builder.a_cap, 3)
    assert cell.dtype == torch.float32 and cell.is_contiguous() and cell.shape[0] >= builder.B + 1 and tuple(cell.shape[1:]) == (3, 3)
    assert builder.pbc.dtype == torch.uint8 and tuple(builder.pbc.shape) == (builder.B + 1, 3)
    assert builder.mol_off.numel() == builder.B + 2 and builder.atom_mol.numel() == builder.a_cap
    assert staging.dtype == torch.int32 and staging.numel() >= 7 * e_cap
    assert state.dtype == torch.int32 and state.numel() >= 8
    assert ws.dtype == torch.uint8 and ws.numel() >= pbc_index_ws_bytes(builder.a_cap, e_cap)
    for k in ("id_c", "id_a", "id_swap", "id_undir"):
        assert bufs[k].dtype == torch.int32 and bufs[k].numel() == e_cap and bufs[k].is_contiguous()
    assert bufs["cell_offsets"].dtype == torch.int32 and tuple(bufs["cell_offsets"].shape) == (e_cap, 3)
    assert bufs["cell_offsets"].is_contiguous()
    for k in ("id3_reduce_ca", "id3_expand_ba"):
        assert bufs[k].dtype == torch.int32 and bufs[k].numel() == t_cap and bufs[k].is_contiguous()
    check(_lib.load().gn_pbc_index_padded_tv(
        ptr(R), ptr(cell), ptr(builder.pbc), ptr(builder.mol_off), ptr(builder.atom_mol), builder.B, builder.cutoff,
        ptr(ws), int(e_cap), int(t_cap), int(a_cap), int(n_groups), int(deg_bound), ptr(staging), ptr(bufs["id_c"]),
        ptr(bufs["id_a"]), ptr(bufs["id_swap"]), ptr(bufs["id_undir"]), ptr(bufs["cell_offsets"]), ptr(bufs["id3_reduce_ca"]),
        ptr(bufs["id3_expand_ba"]), ptr(state), stream()), "gn_pbc_index_padded_tv")


PADDED_Q_KEYS = ("id_c", "id_a", "id_swap", "id_undir", "id3_reduce_ca", "id3_expand_ba", "id4_int_a", "id4_int_b",
                 "id4_reduce_intm_ca", "id4_expand_intm_db", "id4_reduce_intm_ab", "id4_expand_intm_ab",
                 "id4_reduce_ca", "id4_expand_db", "id4_reduce_cab", "id4_expand_abd")


def index_padded_q(builder, R, caps, a_cap, n_groups, deg_bound, staging, bufs, state):
    """The quadruplet index build of `builder` for positions R straight into the capacity-sized arrays `bufs` (the sixteen
    arrays PADDED_Q_KEYS, int32) with the dummy molecule's pad rows — no read-back, capturable (gn_index_gpu_padded_q;
    caps = (e_cap, t_cap, eint_cap, i_cap, q_cap); state: int32[8])."""
    require_device(R, staging, state)
    assert not builder.triplets_only and R.is_contiguous() and tuple(R.shape) == (builder.A, 3)
    e_cap, t_cap, eint_cap, i_cap, q_cap = (int(c) for c in caps)
    assert staging.dtype == torch.int32 and staging.numel() >= 4 * e_cap + 2 * eint_cap
    assert state.dtype == torch.int32 and state.numel() >= 8
    want = dict(zip(PADDED_Q_KEYS, (e_cap,) * 4 + (t_cap,) * 2 + (eint_cap,) * 2 + (i_cap,) * 4 + (q_cap,) * 4))
    for k, n in want.items():
        assert bufs[k].dtype == torch.int32 and bufs[k].numel() == n and bufs[k].is_contiguous(), k
    c_arr = (ctypes.c_void_p * 16)(*[addr(bufs[k]) for k in PADDED_Q_KEYS])
    check(_lib.load().gn_index_gpu_padded_q(
        ptr(R), int(R.dtype == torch.float64), ptr(builder.mol_off), ptr(builder.sq_off), builder.B, builder.A, builder.nmax,
        builder.sum_n2, builder.cutoff, builder.int_cutoff, ptr(builder.ws), e_cap, t_cap, eint_cap, i_cap, q_cap, int(a_cap),
        int(n_groups), int(deg_bound), ptr(staging), c_arr, ptr(state), stream()),
        "gn_index_gpu_padded_q")


def index_padded_qv(builder, R, caps, a_cap, n_groups, deg_bound, staging, bufs, state):
    """`index_padded_q` for a builder whose layout changes from replay to replay (index_device.DeviceCapacityQuadGraphBuilder): R
    (a_cap,3) — the batch, then the filler atoms — read at replay time with the layout `index_layout` wrote in the same step
    (gn_index_gpu_padded_qv; the builder's ws: index_cap_ws_bytes(a_cap, n_max, quad=True), staging: int32[4 e_cap + 2 eint_cap],
    caps = (e_cap, t_cap, eint_cap, i_cap, q_cap); state: int32[8], see the header)."""
    require_device(R, staging, state, builder.ws)
    assert not builder.triplets_only and builder.a_cap == int(a_cap) and builder.B <= int(a_cap) and builder.n_max >= 2
    assert R.dtype in (torch.float32, torch.float64) and R.is_contiguous() and tuple(R.shape) == (builder.a_cap, 3)
    assert builder.mol_off.numel() == builder.B + 2 and builder.sq_off.numel() == builder.B + 1
    assert builder.atom_mol.numel() == builder.a_cap and builder.atom_mol.dtype == torch.int32
    assert builder.ws.dtype == torch.uint8 and builder.ws.numel() >= index_cap_ws_bytes(builder.a_cap, builder.n_max, quad=True)
    e_cap, t_cap, eint_cap, i_cap, q_cap = (int(c) for c in caps)
    assert staging.dtype == torch.int32 and staging.numel() >= 4 * e_cap + 2 * eint_cap
    assert state.dtype == torch.int32 and state.numel() >= 8
    want = dict(zip(PADDED_Q_KEYS, (e_cap,) * 4 + (t_cap,) * 2 + (eint_cap,) * 2 + (i_cap,) * 4 + (q_cap,) * 4))
    for k, n in want.items():
        assert bufs[k].dtype == torch.int32 and bufs[k].numel() == n and bufs[k].is_contiguous(), k
    c_arr = (ctypes.c_void_p * 16)(*[addr(bufs[k]) for k in PADDED_Q_KEYS])
    check(_lib.load().gn_index_gpu_padded_qv(
        ptr(R), int(R.dtype == torch.float64), ptr(builder.mol_off), ptr(builder.sq_off), ptr(builder.atom_mol), builder.B,
        builder.n_max, builder.cutoff, builder.int_cutoff, ptr(builder.ws), e_cap, t_cap, eint_cap, i_cap, q_cap, int(a_cap),
        int(n_groups), int(deg_bound), ptr(staging), c_arr, ptr(state), stream()),
        "gn_index_gpu_padded_qv")


@functools.lru_cache(maxsize=64)
def pbc_qindex_ws_bytes(n_atoms, e_cap, eint_cap):
    """Bytes of the workspace gn_pbc_qindex_padded needs for `n_atoms` atoms and capacities of `e_cap` edges and `eint_cap`
    interaction edges (its staging array: 7 e_cap + 5 eint_cap int32).  A pure function of the three sizes, remembered: the
    size check of `pbc_index_padded_q` inside a capture then asks nothing of the library."""
    return int(_lib.load().gn_pbc_qindex_ws_bytes(int(n_atoms), int(e_cap), int(eint_cap), None))


PADDED_QP_KEYS = PADDED_Q_KEYS + ("cell_offsets", "int_cell_offsets")


def pbc_index_padded_q(builder, R, cell, caps, a_cap, n_groups, deg_bound, ws, staging, bufs, state):
    """The quadruplet index build of `builder` (pbc.PeriodicQuadGraphBuilder) for positions R (A,3) and `cell` (>= B rows of
    (3,3)), both float32 ON THE DEVICE, straight into the capacity-sized arrays `bufs` (the sixteen arrays PADDED_Q_KEYS +
    cell_offsets (e_cap,3) + int_cell_offsets (eint_cap,3): int32) with the dummy molecule's pad rows behind the batch — no
    read-back, capturable (gn_pbc_qindex_padded; caps = (e_cap, t_cap, eint_cap, i_cap, q_cap); ws: uint8 of
    pbc_qindex_ws_bytes(A, e_cap, eint_cap), staging: int32[7 e_cap + 5 eint_cap], state: int32[8], see the header)."""
    require_device(R, cell, ws, staging, state)
    assert R.dtype == torch.float32 and R.is_contiguous() and tuple(R.shape) == (builder.A, 3)
    assert cell.dtype == torch.float32 and cell.is_contiguous() and cell.shape[0] >= builder.B and tuple(cell.shape[1:]) == (3, 3)
    e_cap, t_cap, eint_cap, i_cap, q_cap = (int(c) for c in caps)
    assert staging.dtype == torch.int32 and staging.numel() >= 7 * e_cap + 5 * eint_cap
    assert state.dtype == torch.int32 and state.numel() >= 8
    assert ws.dtype == torch.uint8 and ws.numel() >= pbc_qindex_ws_bytes(builder.A, e_cap, eint_cap)
    want = dict(zip(PADDED_Q_KEYS, (e_cap,) * 4 + (t_cap,) * 2 + (eint_cap,) * 2 + (i_cap,) * 4 + (q_cap,) * 4))
    for k, n in want.items():
        assert bufs[k].dtype == torch.int32 and bufs[k].numel() == n and bufs[k].is_contiguous(), k
    for k, n in (("cell_offsets", e_cap), ("int_cell_offsets", eint_cap)):
        assert bufs[k].dtype == torch.int32 and tuple(bufs[k].shape) == (n, 3) and bufs[k].is_contiguous(), k
    c_arr = (ctypes.c_void_p * 18)(*[addr(bufs[k]) for k in PADDED_QP_KEYS])
    check(_lib.load().gn_pbc_qindex_padded(
        ptr(R), ptr(cell), ptr(builder.pbc), ptr(builder.mol_off), ptr(builder.atom_mol), builder.B, builder.A, builder.cutoff,
        builder.int_cutoff, ptr(ws), e_cap, t_cap, eint_cap, i_cap, q_cap, int(a_cap), int(n_groups), int(deg_bound), ptr(staging),
        c_arr, ptr(state), stream()), "gn_pbc_qindex_padded")


def cbf_project_supported(rad, y, W):
    return rad.dim() == 3 and rad.shape[1] * rad.shape[2] <= 64 and W.shape[0] <= 16 and W.shape[1] == rad.shape[1] * rad.shape[2] \
        and y.shape[1] == rad.shape[1]


def cbf_project_fwd(rad, ie32, y, W):
    """out[i, n] = sum_{l, r} rad[ie[i], l, r] y[i, l] W[n, l R + r] (gn_cbf_project_fwd_f32)."""
    require_device(rad, ie32, y, W)
    rad, y, W = _f32c(rad), _f32c(y), _f32c(W)
    I, S, R, N = int(y.shape[0]), int(rad.shape[1]), int(rad.shape[2]), int(W.shape[0])
    out = torch.empty((I, N), device=y.device, dtype=torch.float32)
    check(_lib.load().gn_cbf_project_fwd_f32(ptr(rad), ptr(ie32), ptr(y), ptr(W), ptr(out), I, S, R, N, stream()),
          "gn_cbf_project_fwd_f32")
    return out


def cbf_project_bwd(g, rad, seg_off, y, W):
    """-> (g_rad like rad, g_y like y): the adjoint of cbf_project_fwd for a frozen W (gn_cbf_project_bwd_f32)."""
    require_device(g, rad, seg_off, y, W)
    g, rad, y, W = _f32c(g), _f32c(rad), _f32c(y), _f32c(W)
    E, S, R, N = int(rad.shape[0]), int(rad.shape[1]), int(rad.shape[2]), int(W.shape[0])
    if seg_off.dtype != torch.int32:
        seg_off = seg_off.to(torch.int32)
    assert seg_off.numel() == E + 1
    g_rad, g_y = torch.empty_like(rad), torch.empty_like(y)
    check(_lib.load().gn_cbf_project_bwd_f32(ptr(g), ptr(rad), ptr(seg_off), ptr(y), ptr(W), ptr(g_rad), ptr(g_y), E, S, R, N,
                                             stream()), "gn_cbf_project_bwd_f32")
    return g_rad, g_y


def force_loss(E, Et, F, Ft, w_e, w_f, mask=None, w_f_dev=None):
    """-> (loss (), gE like E, gF like F): loss = w_e sum|E - Et| + w_f [* w_f_dev] sum_a mask_a |F_a - Ft_a|_2 and its
    cotangents in one launch (gn_force_loss_f32)."""
    require_device(E, Et, F, Ft)
    E, Et, F, Ft = _f32c(E), _f32c(Et), _f32c(F), _f32c(Ft)
    assert E.shape == Et.shape and F.shape == Ft.shape and F.dim() == 2 and F.shape[1] == 3
    if mask is not None:
        mask = _f32c(mask)
        assert mask.numel() == F.shape[0]
    loss = torch.empty((), device=E.device, dtype=torch.float32)
    gE, gF = torch.empty_like(E), torch.empty_like(F)
    check(_lib.load().gn_force_loss_f32(ptr(E), ptr(Et), E.numel(), ptr(F), ptr(Ft), F.shape[0], ptr(mask), float(w_e), float(w_f),
                                        ptr(w_f_dev), ptr(loss), ptr(gE), ptr(gF), stream()), "gn_force_loss_f32")
    return loss, gE, gF


def periodic_loss(E, Et, F, Ft, w_e, w_f, S=None, St=None, w_s=0.0, mask=None, w_f_dev=None):
    """-> (loss (), gE like E, gF like F, gS like S or None): force_loss plus w_s sum_b |S_b - St_b|_F over the (B,3,3) stresses
    and its cotangent, in one launch (gn_periodic_loss_f32).  S = None: no stress term — loss, gE, gF are force_loss's bit for bit."""
    require_device(E, Et, F, Ft)
    E, Et, F, Ft = _f32c(E), _f32c(Et), _f32c(F), _f32c(Ft)
    assert E.shape == Et.shape and F.shape == Ft.shape and F.dim() == 2 and F.shape[1] == 3
    if mask is not None:
        mask = _f32c(mask)
        assert mask.numel() == F.shape[0]
    gS, B = None, 0
    if S is not None:
        require_device(S, St)
        S, St = _f32c(S), _f32c(St)
        assert S.shape == St.shape and S.dim() == 3 and tuple(S.shape[1:]) == (3, 3)
        gS, B = torch.empty_like(S), int(S.shape[0])
    loss = torch.empty((), device=E.device, dtype=torch.float32)
    gE, gF = torch.empty_like(E), torch.empty_like(F)
    check(_lib.load().gn_periodic_loss_f32(ptr(E), ptr(Et), E.numel(), ptr(F), ptr(Ft), F.shape[0], ptr(mask), ptr(S), ptr(St), B,
                                           float(w_e), float(w_f), ptr(w_f_dev), float(w_s), ptr(loss), ptr(gE), ptr(gF), ptr(gS),
                                           stream()), "gn_periodic_loss_f32")
    return loss, gE, gF, gS


def index_poison(x, state):
    """x <- NaN when the index build of this step reported an error (gn_index_poison_f32)."""
    require_device(x, state)
    assert x.dtype == torch.float32 and x.is_contiguous()
    check(_lib.load().gn_index_poison_f32(ptr(x), x.numel(), ptr(state), stream()), "gn_index_poison_f32")


def rbf_aggregate_supported(m, rbf, W):
    return m.shape[1] == 128 and rbf.shape[1] == 16 and tuple(W.shape) == (128, 16)


def rbf_aggregate_fwd(m, rbf, W, perm, seg_off, n_atoms, scale):
    """out[a] = scale * sum_{e -> a} m[e] * (W rbf[e]) in one pass (gn_rbf_aggregate_fwd_f32)."""
    require_device(m, rbf, W)
    m, rbf, W = _f32c(m), _f32c(rbf), _f32c(W)
    out = torch.empty((n_atoms, m.shape[1]), device=m.device, dtype=torch.float32)
    check(_lib.load().gn_rbf_aggregate_fwd_f32(ptr(m), ptr(rbf), ptr(W), ptr(perm), ptr(seg_off), ptr(out), n_atoms,
                                               m.shape[1], rbf.shape[1], float(scale), stream()), "gn_rbf_aggregate_fwd_f32")
    return out


def rbf_aggregate_bwd(g_out, m, rbf, W, id_a32, scale, want_m=True, want_rbf=True, acc_m=None, acc_rbf=None):
    """-> (g_m (E,C) or None, g_rbf (E,R) or None) (gn_rbf_aggregate_bwd_f32).  acc_m / acc_rbf: running gradients
    the contribution is ADDED to in the same pass (and which are returned) instead of new tensors."""
    require_device(g_out, m, rbf, W)
    g_out, m, rbf, W = _f32c(g_out), _f32c(m), _f32c(rbf), _f32c(W)
    for t, like in ((acc_m, m), (acc_rbf, rbf)):
        assert t is None or (t.shape == like.shape and t.dtype == torch.float32 and t.is_contiguous())
    g_m = acc_m if acc_m is not None else (torch.empty_like(m) if want_m else None)
    g_rbf = acc_rbf if acc_rbf is not None else (torch.empty_like(rbf) if want_rbf else None)
    accum = (1 if acc_m is not None else 0) | (2 if acc_rbf is not None else 0)
    check(_lib.load().gn_rbf_aggregate_bwd_f32(ptr(g_out), ptr(m), ptr(rbf), ptr(W), ptr(id_a32), ptr(g_m), ptr(g_rbf),
                                               m.shape[0], m.shape[1], rbf.shape[1], float(scale), accum, stream()),
          "gn_rbf_aggregate_bwd_f32")
    return g_m, g_rbf


def rbf_aggregate_grouped_fwd(m_list, rbf, W_list, scales, perm, seg_off, n_atoms):
    """out (G, n_atoms, C): out[g] = scales[g] * sum_{e -> a} m_list[g][e] * (W_list[g] rbf[e]) for the G groups that share
    rbf and the CSR, one launch (gn_rbf_aggregate_grouped_fwd_f32).  `scales`: device tensor (G)."""
    require_device(rbf, scales, *m_list, *W_list)
    m_list, W_list = [_f32c(t) for t in m_list], [_f32c(t) for t in W_list]
    rbf, scales = _f32c(rbf), _f32c(scales)
    G = len(m_list)
    assert len(W_list) == G and scales.numel() == G
    if m_list[0].shape[0] == 0:
        # no edge at all (a single atom, a dissociated pair): every segment is empty and an empty tensor has no address to put
        # into the pointer table, which the launcher rejects — the sums are zero, nothing is launched
        return torch.zeros((G, n_atoms, m_list[0].shape[1]), device=rbf.device, dtype=torch.float32)
    out = torch.empty((G, n_atoms, m_list[0].shape[1]), device=rbf.device, dtype=torch.float32)
    arr = ctypes.c_void_p * G
    check(_lib.load().gn_rbf_aggregate_grouped_fwd_f32(arr(*[addr(t) for t in m_list]), arr(*[addr(t) for t in W_list]),
                                                       ptr(scales), G, ptr(rbf), ptr(perm), ptr(seg_off), ptr(out), n_atoms,
                                                       m_list[0].shape[1], rbf.shape[1], stream()),
          "gn_rbf_aggregate_grouped_fwd_f32")
    return out


def rbf_aggregate_grouped_bwd(g_out, m_list, rbf, W_list, scales, id_a32, acc_m=None, want_rbf=True, acc_rbf=None):
    """Adjoint of `rbf_aggregate_grouped_fwd` (gn_rbf_aggregate_grouped_bwd_f32) -> ([g_m[g] (E,C)], g_rbf (E,R) or None).
    g_out: the stacked (G, n_atoms, C) gradient.  acc_m[g] / acc_rbf: running gradients the contribution is ADDED to in the
    same pass (and which are returned); g_rbf is the sum over the groups, in group order."""
    require_device(g_out, rbf, scales, *m_list, *W_list)
    m_list, W_list = [_f32c(t) for t in m_list], [_f32c(t) for t in W_list]
    g_out, rbf, scales = _f32c(g_out), _f32c(rbf), _f32c(scales)
    G = len(m_list)
    acc_m = list(acc_m) if acc_m is not None else [None] * G
    g_m, accum = [], 0
    for g, (t, like) in enumerate(zip(acc_m, m_list)):
        assert t is None or (t.shape == like.shape and t.dtype == torch.float32 and t.is_contiguous())
        accum |= (1 << g) if t is not None else 0
        g_m.append(t if t is not None else torch.empty_like(like))
    assert acc_rbf is None or (acc_rbf.shape == rbf.shape and acc_rbf.dtype == torch.float32 and acc_rbf.is_contiguous())
    g_rbf = acc_rbf if acc_rbf is not None else (torch.empty_like(rbf) if want_rbf else None)
    arr = ctypes.c_void_p * G
    check(_lib.load().gn_rbf_aggregate_grouped_bwd_f32(ptr(g_out), arr(*[addr(t) for t in m_list]),
                                                       arr(*[addr(t) for t in W_list]), ptr(scales), G, ptr(rbf), ptr(id_a32),
                                                       arr(*[addr(t) for t in g_m]), ptr(g_rbf), m_list[0].shape[0],
                                                       g_out.shape[1], m_list[0].shape[1], rbf.shape[1], accum,
                                                       int(acc_rbf is not None), stream()),
          "gn_rbf_aggregate_grouped_bwd_f32")
    return g_m, g_rbf


def energy_head_fwd(x, w):
    """E (A,1) = sum_g x[g] @ w[g], g in order: x (G,A,C) stacked, w (G,C) (gn_energy_head_fwd_f32)."""
    require_device(x, w)
    x, w = _f32c(x), _f32c(w)
    G, A, C = x.shape
    E = torch.empty((A, 1), device=x.device, dtype=torch.float32)
    check(_lib.load().gn_energy_head_fwd_f32(ptr(x), ptr(w), ptr(E), G, A, C, stream()), "gn_energy_head_fwd_f32")
    return E


def energy_head_bwd(g_E, w):
    """g_x (G,A,C) = g_E[a] * w[g] (gn_energy_head_bwd_f32)."""
    require_device(g_E, w)
    g_E, w = _f32c(g_E), _f32c(w)
    G, C = w.shape
    A = g_E.shape[0]
    g_x = torch.empty((G, A, C), device=w.device, dtype=torch.float32)
    check(_lib.load().gn_energy_head_bwd_f32(ptr(g_E), ptr(w), ptr(g_x), G, A, C, stream()), "gn_energy_head_bwd_f32")
    return g_x


def bmm(A, B, ta, tb):
    """(A^T if ta else A) @ (B^T if tb else B), batched over dim 0."""
    require_device(A, B)
    A, B = _f32c(A), _f32c(B)
    b = A.shape[0]
    m, k = (A.shape[2], A.shape[1]) if ta else (A.shape[1], A.shape[2])
    n = B.shape[1] if tb else B.shape[2]
    C = torch.empty((b, m, n), device=A.device, dtype=torch.float32)
    check(_lib.load().gn_bmm_f32(ptr(A), ptr(B), ptr(C), b, m, n, k, int(ta), int(tb), stream()), "gn_bmm_f32")
    return C


def ssilu(x, k):
    require_device(x)
    x = _f32c(x)
    out = torch.empty_like(x)
    check(_lib.load().gn_ssilu_f32(ptr(x), ptr(out), x.numel(), k, stream()), "gn_ssilu_f32")
    return out


def pm(z, k, a=None, b=None, d=None, c=1.0):
    """c * ssilu^(k)(z) * a * b * d  (k = -1: no activation factor; a, b, d optional, all of one shape)."""
    ref = z if z is not None else a
    require_device(ref)
    ts = [None if t is None else _f32c(t) for t in (z, a, b, d)]
    for t in ts:
        assert t is None or t.shape == ref.shape, "pm operands must share one shape"
    out = torch.empty(ref.shape, device=ref.device, dtype=torch.float32)
    check(_lib.load().gn_pm_f32(ptr(ts[0]), int(k), ptr(ts[1]), ptr(ts[2]), ptr(ts[3]), float(c), ptr(out),
                                out.numel(), stream()), "gn_pm_f32")
    return out


def dact_mul(g, z, act, mul, c, want_gmul=False):
    """dz = g*c*(mul or 1)*(ssilu'(z) if act else 1); gmul = g*c*(ssilu(z) if act else z)."""
    require_device(g)
    g = _f32c(g)
    z = None if z is None else _f32c(z)
    mul = None if mul is None else _f32c(mul)
    dz = torch.empty_like(g)
    gmul = torch.empty_like(g) if want_gmul else None
    check(_lib.load().gn_dact_mul_f32(ptr(g), ptr(z), int(bool(act)), ptr(mul), float(c), ptr(dz), ptr(gmul),
                                      g.numel(), stream()), "gn_dact_mul_f32")
    return dz, gmul


def bil_reduce(Y, x, sp):
    """Sm[e,s,c] = sum_{t in seg(e)} Y[t,s] x[g(t),c]."""
    require_device(Y, x)
    Y, x = _f32c(Y), _f32c(x)
    S, C = Y.shape[1], x.shape[1]
    Sm = torch.empty((sp.n_reduce, S, C), device=x.device, dtype=torch.float32)
    check(_lib.load().gn_bil_reduce_f32(ptr(Y), ptr(x), ptr(sp.expand.idx32), ptr(sp.seg_off), ptr(Sm),
                                        sp.n_reduce, S, C, stream()), "gn_bil_reduce_f32")
    return Sm


# The x-adjoint of the tensor basis without per-quadruplet rows in memory (round 6, gn_bil_expand_rows_ang_f32: a WAVE owns 32
# expand rows of one atom and walks the atom's reduce edges with the accumulators in registers — no LDS accumulation, no barrier,
# rows written once; the quadruplet of (edge, row) from a dense per-atom grid built with the index plan,
# graph.SegmentPlan.row_grid).  GEMNET_ROW_GRID=0: per-quadruplet rows + a segmented sum.
USE_ROW_GRID = os.environ.get("GEMNET_ROW_GRID", "1") == "1"
# Which angle-form kernels run their products on the fp16 matrix pipe (`arith` = GN_ANG_F16 of the launch): bit 0 = K1 of
# bil_reduce_project (only under the "h3" Dense arithmetic: x unscaled), bit 1 = the angle gradient bil_dy_multi, bit 2 = the
# x-adjoint bil_expand (both under an exact per-edge scale: any magnitude).  Read-only configuration (A/B runs, tests).
ANG_F16_MASK = int(os.environ.get("GEMNET_ANG_F16", "7")) & 7


# The triplet x-adjoint per atom on the matrix cores (gn_bil_x_adjoint_atoms_f32: groups of <= 32 rows as one dense product
# on v_mfma_f32_16x16x4_f32, index staging from the plan's flat entry list; larger groups keep the scalar body in the same
# launch).  GEMNET_XADJ_MFMA=0: the scalar grouped launch (gn_bil_reduce_t_grouped_f32) for every group.
USE_XADJ_MFMA = os.environ.get("GEMNET_XADJ_MFMA", "1") == "1"
# The triplet Y gradient per atom on the matrix cores (gn_bil_dy_atoms_f32: one workgroup per atom, groups of <= 32 rows as one
# dense product over the plan's flat entry list, the atom's x rows read once per block instead of once per triplet; larger groups
# keep the per-edge body in the same launch).  GEMNET_DY_ATOMS=0: the per-edge launch (gn_bil_dy_multi_f32) everywhere.
USE_DY_ATOMS = os.environ.get("GEMNET_DY_ATOMS", "1") == "1"


def bil_reduce_t(Y, D, sp):
    """dx[j,c] = sum_{t: g(t)=j} sum_s Y[t,s] D[r(t),s,c].
    Angle form (GemNet-Q): the row-stationary kernel when the plan carries the per-atom grid (USE_ROW_GRID, the default: no
    per-quadruplet rows in memory), else per-quadruplet rows + a segmented sum.  Spherical basis of the triplets: the
    atom-grouped kernel; other shapes: the scalar kernels.
    (Tried and removed: one workgroup per atom with its rows in LDS, and rows written in destination order — both slower,
    profiles/r4_q_atom_blocks.txt, profiles/r5_expand_pos_ab.txt.)"""
    require_device(Y, D)
    Y, D = _f32c(Y), _f32c(D)
    S, C = D.shape[1], D.shape[2]
    permT, segT = sp.expand.csr
    if is_angle_form(Y, S):
        rg = sp.row_grid if (USE_ROW_GRID and C == 32) else None
        if rg is not None:
            a_perm, a_seg, j_off, qmap, g_off, task_atom, task_row0, n_tasks = rg
            dx = torch.empty((sp.n_expand, C), device=Y.device, dtype=torch.float32)     # the tasks partition the rows
            check(_lib.load().gn_bil_expand_rows_ang_f32(ptr(Y), ptr(D), ptr(a_perm), ptr(a_seg), ptr(j_off), ptr(qmap),
                                                         ptr(g_off), ptr(task_atom), ptr(task_row0), int(n_tasks), ptr(dx), S, C,
                                                         (GN_ANG_F16 if ANG_F16_MASK & 4 else 0) | (sp.ROW_TILE << 8), stream()),
                  "gn_bil_expand_rows_ang_f32")
            return dx
        dxt = torch.empty((sp.size, C), device=Y.device, dtype=torch.float32)
        check(_lib.load().gn_bil_expand_ang_f32(ptr(Y), ptr(D), ptr(sp.seg_off), ptr(dxt), sp.n_reduce, S, C,
                                                GN_ANG_F16 if ANG_F16_MASK & 4 else 0, stream()), "gn_bil_expand_ang_f32")
        return segsum(dxt, permT, segT, sp.n_expand)
    if S > 8:
        # tensor basis: per-quadruplet rows grouped by reduce edge (dSm[e] read once per edge), then one CSR sum
        dxt = torch.empty((sp.size, C), device=Y.device, dtype=torch.float32)
        check(_lib.load().gn_bil_expand_f32(ptr(Y), ptr(D), ptr(sp.seg_off), ptr(dxt), sp.n_reduce, S, C, stream()),
              "gn_bil_expand_f32")
        return segsum(dxt, permT, segT, sp.n_expand)
    grp = sp.groups if S == 7 and C == 64 else None
    if grp is not None and 0 < grp[4] * S * C * 4 <= 160 * 1024:
        # triplets: both edges end in the same atom — that atom's dSm blocks are parked in LDS once
        rows, off, kseg, rposT, max_rows = grp
        dx = torch.empty((sp.n_expand, C), device=Y.device, dtype=torch.float32)
        if USE_XADJ_MFMA:
            ent_off, ent_t, ent_bc = sp.group_entries
            check(_lib.load().gn_bil_x_adjoint_atoms_f32(ptr(Y), ptr(D), ptr(rows), ptr(off), ptr(kseg), ptr(permT), ptr(rposT),
                                                         ptr(ent_off), ptr(ent_t), ptr(ent_bc), ptr(dx), off.shape[0] - 1,
                                                         max_rows, S, C, stream()), "gn_bil_x_adjoint_atoms_f32")
            return dx
        check(_lib.load().gn_bil_reduce_t_grouped_f32(ptr(Y), ptr(D), ptr(rows), ptr(off), ptr(kseg), ptr(permT),
                                                      ptr(rposT), ptr(dx), off.shape[0] - 1, max_rows, S, C, stream()),
              "gn_bil_reduce_t_grouped_f32")
        return dx
    dx = torch.empty((sp.n_expand, C), device=Y.device, dtype=torch.float32)
    check(_lib.load().gn_bil_reduce_t_f32(ptr(Y), ptr(D), ptr(sp.reduce.idx32), ptr(permT), ptr(segT),
                                          ptr(dx), sp.n_expand, S, C, stream()), "gn_bil_reduce_t_f32")
    return dx


def bil_dot(D, x, sp):
    """dY[t,s] = sum_c D[r(t),s,c] x[g(t),c]."""
    require_device(D, x)
    D, x = _f32c(D), _f32c(x)
    S, C = D.shape[1], x.shape[1]
    dY = torch.empty((sp.size, S), device=x.device, dtype=torch.float32)
    check(_lib.load().gn_bil_dot_f32(ptr(D), ptr(x), ptr(sp.expand.idx32), ptr(sp.seg_off), ptr(dY),
                                     sp.n_reduce, S, C, stream()), "gn_bil_dot_f32")
    return dY


def bessel_rbf(d, freq, cutoff, p, kd, kf):
    require_device(d, freq)
    d, freq = _f32c(d), _f32c(freq)
    out = torch.empty((d.shape[0], freq.shape[0]), device=d.device, dtype=torch.float32)
    check(_lib.load().gn_bessel_rbf_f32(ptr(d), ptr(freq), ptr(out), d.shape[0], freq.shape[0],
                                        cutoff, p, kd, kf, stream()), "gn_bessel_rbf_f32")
    return out


def sph_radial(d, z, nrm, cutoff, p, kd):
    """z (S,R) float32 roots, nrm (S,R) float64 normalisers (device tensors)."""
    require_device(d, z, nrm)
    d = _f32c(d)
    assert z.dtype == torch.float32 and nrm.dtype == torch.float64 and z.is_contiguous() and nrm.is_contiguous()
    S, R = z.shape
    out = torch.empty((d.shape[0], S, R), device=d.device, dtype=torch.float32)
    check(_lib.load().gn_sph_radial_f32(ptr(d), ptr(z), ptr(nrm), ptr(out), d.shape[0], S, R,
                                        cutoff, p, kd, stream()), "gn_sph_radial_f32")
    return out


def ylm0(theta, S, k):
    require_device(theta)
    theta = _f32c(theta)
    out = torch.empty((theta.shape[0], S), device=theta.device, dtype=torch.float32)
    check(_lib.load().gn_ylm0_f32(ptr(theta), ptr(out), theta.shape[0], S, k, stream()), "gn_ylm0_f32")
    return out


def ylm(theta, phi, S, kt, kp):
    require_device(theta, phi)
    theta, phi = _f32c(theta), _f32c(phi)
    out = torch.empty((theta.shape[0], S * S), device=theta.device, dtype=torch.float32)
    check(_lib.load().gn_ylm_f32(ptr(theta), ptr(phi), ptr(out), theta.shape[0], S, kt, kp, stream()),
          "gn_ylm_f32")
    return out


def edge_basis_fwd(R, idx_c, idx_a, freq, z, nrm, cutoff, p, want_V=False, want_rbf=True):
    """-> D (E,), V (E,3)|None, rbf (E,NR)|None, rad (E,S,NR)   (gemnet.py:261-286 + basis_layers.py:45-49,121-128)."""
    require_device(R, idx_c, idx_a, z, nrm)
    R = _f32c(R)
    E = idx_c.shape[0]
    S, NR = z.shape
    D = torch.empty(E, device=R.device, dtype=torch.float32)
    V = torch.empty((E, 3), device=R.device, dtype=torch.float32) if want_V else None
    rbf = torch.empty((E, NR), device=R.device, dtype=torch.float32) if want_rbf else None
    rad = torch.empty((E, S, NR), device=R.device, dtype=torch.float32)
    if want_rbf:
        freq = _f32c(freq)
    # without rbf the kernel still walks NR "rbf" work items per edge; give it a scratch target
    rbf_t = rbf if want_rbf else torch.empty((E, NR), device=R.device, dtype=torch.float32)
    fr = freq if want_rbf else torch.zeros(NR, device=R.device, dtype=torch.float32)
    check(_lib.load().gn_edge_basis_fwd_f32(ptr(R), ptr(idx_c), ptr(idx_a), ptr(fr), ptr(z), ptr(nrm), ptr(D),
                                            ptr(V), ptr(rbf_t), ptr(rad), E, NR, S, cutoff, p, stream()),
          "gn_edge_basis_fwd_f32")
    return D, V, rbf, rad


def edge_basis_bwd(gD, g_rbf, g_rad, R, idx_c, idx_a, freq, z, nrm, cutoff, p):
    """-> W (E,3) per-edge position gradient: dE/dR = segsum(W, id_a) - segsum(W, id_c)."""
    require_device(R, idx_c, idx_a)
    R = _f32c(R)
    E = idx_c.shape[0]
    S, NR = z.shape
    gD = None if gD is None else _f32c(gD)
    g_rbf = None if g_rbf is None else _f32c(g_rbf)
    g_rad = None if g_rad is None else _f32c(g_rad)
    fr = _f32c(freq) if freq is not None else torch.zeros(NR, device=R.device, dtype=torch.float32)
    W = torch.empty((E, 3), device=R.device, dtype=torch.float32)
    check(_lib.load().gn_edge_basis_bwd_f32(ptr(gD), ptr(g_rbf), ptr(g_rad), ptr(R), ptr(idx_c), ptr(idx_a),
                                            ptr(fr), ptr(z), ptr(nrm), ptr(W), E, NR, S, cutoff, p, stream()),
          "gn_edge_basis_bwd_f32")
    return W


RADIAL_HEAD_SHAPE = (6, 7, 16)      # (NR, S, columns) the kernels are built for


def radial_head_weights(W_rbf3, W_rbf_h, W_rbf_out, W_cbf3):
    """wcat (3 + S, NR, NI) of gn_radial_head_*: the three (NI, NR) Dense weights transposed, then the (S, NR, NI) weight of the
    circular-basis down projection."""
    S, NR, NI = W_cbf3.shape
    for W in (W_rbf3, W_rbf_h, W_rbf_out):
        if tuple(W.shape) != (NI, NR):
            raise ValueError(f"radial head: Dense weight of shape {tuple(W.shape)}, expected {(NI, NR)}")
    return torch.cat([W_rbf3.t()[None], W_rbf_h.t()[None], W_rbf_out.t()[None], W_cbf3], 0).to(torch.float32).contiguous()


def _radial_head_args(R, idx_c, idx_a, freq, z, nrm, wcat):
    require_device(R, idx_c, idx_a, freq, z, nrm, wcat)
    S, NR = z.shape
    if wcat.dim() != 3 or (NR, S, wcat.shape[2]) != RADIAL_HEAD_SHAPE or tuple(wcat.shape[:2]) != (3 + S, NR):
        raise ValueError(f"radial head: tables {tuple(z.shape)} / weights {tuple(wcat.shape)}; the kernel takes "
                         f"(S, NR) = (7, 6) and wcat (10, 6, 16)")
    if freq.shape != (NR,) or nrm.shape != z.shape or nrm.dtype != torch.float64:
        raise ValueError("radial head: freq (NR,) f32, z (S, NR) f32 and nrm (S, NR) f64 expected")
    if idx_c.shape != idx_a.shape or idx_c.dim() != 1 or idx_c.dtype != torch.int32 or idx_a.dtype != torch.int32:
        raise ValueError("radial head: id_c / id_a are (E,) int32")
    return _f32c(R), idx_c.contiguous(), idx_a.contiguous(), _f32c(freq), _f32c(z), nrm.contiguous(), _f32c(wcat)


def radial_head_fwd(R, idx_c, idx_a, freq, z, nrm, wcat, cutoff, p):
    """-> rbf (E,NR), rbf3, rbf_h, rbf_out (E,16), rbf_W1 (E,S,16): distances, both radial bases and their four frozen
    projections in one launch (gn_radial_head_fwd_f32; wcat from `radial_head_weights`)."""
    R, idx_c, idx_a, freq, z, nrm, wcat = _radial_head_args(R, idx_c, idx_a, freq, z, nrm, wcat)
    E = idx_c.shape[0]
    NR, S, NI = RADIAL_HEAD_SHAPE
    new = lambda *shape: torch.empty(shape, device=R.device, dtype=torch.float32)   # noqa: E731
    rbf, rbf3, rbf_h, rbf_out, rbf_W1 = new(E, NR), new(E, NI), new(E, NI), new(E, NI), new(E, S, NI)
    check(_lib.load().gn_radial_head_fwd_f32(ptr(R), ptr(idx_c), ptr(idx_a), ptr(freq), ptr(z), ptr(nrm), ptr(wcat), ptr(rbf),
                                             ptr(rbf3), ptr(rbf_h), ptr(rbf_out), ptr(rbf_W1), E, NR, S, NI, cutoff, p,
                                             stream()), "gn_radial_head_fwd_f32")
    return rbf, rbf3, rbf_h, rbf_out, rbf_W1


def radial_head_bwd(g_rbf, g_rbf3, g_rbf_h, g_rbf_out, g_rbf_W1, R, idx_c, idx_a, freq, z, nrm, wcat, cutoff, p):
    """-> W (E,3), the per-edge position gradient of `radial_head_fwd` (dE/dR = segsum(W, id_a) - segsum(W, id_c)); any
    cotangent may be None."""
    R, idx_c, idx_a, freq, z, nrm, wcat = _radial_head_args(R, idx_c, idx_a, freq, z, nrm, wcat)
    E = idx_c.shape[0]
    NR, S, NI = RADIAL_HEAD_SHAPE
    gs = []
    for g, shape in ((g_rbf, (E, NR)), (g_rbf3, (E, NI)), (g_rbf_h, (E, NI)), (g_rbf_out, (E, NI)), (g_rbf_W1, (E, S, NI))):
        if g is not None:
            require_device(g)
            if tuple(g.shape) != shape:
                raise ValueError(f"radial head: cotangent of shape {tuple(g.shape)}, expected {shape}")
            g = _f32c(g)
        gs.append(g)
    W = torch.empty((E, 3), device=R.device, dtype=torch.float32)
    check(_lib.load().gn_radial_head_bwd_f32(*[ptr(g) for g in gs], ptr(R), ptr(idx_c), ptr(idx_a), ptr(freq), ptr(z), ptr(nrm),
                                             ptr(wcat), ptr(W), E, NR, S, NI, cutoff, p, stream()),
          "gn_radial_head_bwd_f32")
    return W


RADIAL_EMB_WIDTH = 128              # atom / edge embedding width the embedding form of the radial head is built for


def _aligned16(*tensors):
    for t in tensors:
        if t is not None and t.data_ptr() % 16:
            raise ValueError("radial head: the 128-column operands must be 16-byte aligned")


def _radial_emb_args(E, n_atoms, zrow, T_c, T_a, W_r):
    NR, NE = RADIAL_HEAD_SHAPE[0], RADIAL_EMB_WIDTH
    if tuple(W_r.shape) != (NR, NE):
        raise ValueError(f"radial head: W_r of shape {tuple(W_r.shape)}, expected {(NR, NE)} (the rbf columns, transposed)")
    if zrow is not None:
        if T_c.dim() != 2 or T_c.shape[1] != NE or T_a.shape != T_c.shape:
            raise ValueError(f"radial head: atom-term tables {tuple(T_c.shape)} / {tuple(T_a.shape)}, expected two (rows, {NE})")
        if zrow.dim() != 1 or zrow.dtype != torch.int32 or zrow.shape[0] < n_atoms:
            raise ValueError("radial head: zrow is (atoms,) int32, one table row per atom")
        T_c, T_a, zrow = _f32c(T_c), _f32c(T_a), zrow.contiguous()
    W_r = _f32c(W_r)
    _aligned16(T_c, T_a, W_r)
    require_device(zrow, T_c, T_a, W_r)
    return zrow, T_c, T_a, W_r


def radial_head_emb_fwd(R, idx_c, idx_a, freq, z, nrm, wcat, zrow, T_c, T_a, W_r, cutoff, p, want_rbf=False):
    """-> m0, d0 (E,128), rbf3, rbf_h, rbf_out (E,16), rbf_W1 (E,S,16), rbf (E,NR) or None: `radial_head_fwd` with the edge
    embedding m0 = ssilu(rbf W_r + T_c[zrow[idx_c]] + T_a[zrow[idx_a]]) and d0 = ssilu'(.) in the same launch
    (gn_radial_head_emb_fwd_f32).  T_c / T_a (rows, 128): the atom-term tables; W_r (NR, 128)."""
    E = idx_c.shape[0]
    NR, S, NI = RADIAL_HEAD_SHAPE
    NE = RADIAL_EMB_WIDTH
    zrow, T_c, T_a, W_r = _radial_emb_args(E, R.shape[0], zrow, T_c, T_a, W_r)
    R, idx_c, idx_a, freq, z, nrm, wcat = _radial_head_args(R, idx_c, idx_a, freq, z, nrm, wcat)
    new = lambda *shape: torch.empty(shape, device=R.device, dtype=torch.float32)   # noqa: E731
    rbf3, rbf_h, rbf_out, rbf_W1, m0, d0 = new(E, NI), new(E, NI), new(E, NI), new(E, S, NI), new(E, NE), new(E, NE)
    rbf = new(E, NR) if want_rbf else None
    check(_lib.load().gn_radial_head_emb_fwd_f32(ptr(R), ptr(idx_c), ptr(idx_a), ptr(freq), ptr(z), ptr(nrm), ptr(wcat),
                                                 ptr(zrow), ptr(T_c), ptr(T_a), ptr(W_r), ptr(rbf), ptr(rbf3), ptr(rbf_h),
                                                 ptr(rbf_out), ptr(rbf_W1), ptr(m0), ptr(d0), E, NR, S, NI, NE, cutoff, p,
                                                 stream()), "gn_radial_head_emb_fwd_f32")
    return m0, d0, rbf3, rbf_h, rbf_out, rbf_W1, rbf


def radial_head_emb_bwd(g_rbf, g_rbf3, g_rbf_h, g_rbf_out, g_rbf_W1, ga, gb, d0, W_r, R, idx_c, idx_a, freq, z, nrm, wcat,
                        cutoff, p):
    """-> W (E,3) of `radial_head_bwd` with the adjoint of the edge embedding added: ga / gb (E,128) are cotangents of m0
    (their sum is taken in the kernel), d0 the stored ssilu'(z0); any cotangent may be None."""
    E = idx_c.shape[0]
    NR, S, NI = RADIAL_HEAD_SHAPE
    NE = RADIAL_EMB_WIDTH
    gs = []
    for g, shape in ((g_rbf, (E, NR)), (g_rbf3, (E, NI)), (g_rbf_h, (E, NI)), (g_rbf_out, (E, NI)), (g_rbf_W1, (E, S, NI)),
                     (ga, (E, NE)), (gb, (E, NE)), (d0, (E, NE))):
        if g is not None:
            if tuple(g.shape) != shape:
                raise ValueError(f"radial head: cotangent of shape {tuple(g.shape)}, expected {shape}")
            g = _f32c(g)
        gs.append(g)
    if (gs[5] is not None or gs[6] is not None) and gs[7] is None:
        raise ValueError("radial head: a cotangent of m0 needs d0")
    _aligned16(*gs[5:])
    _, _, _, W_r = _radial_emb_args(E, R.shape[0], None, None, None, W_r)
    require_device(*gs)
    R, idx_c, idx_a, freq, z, nrm, wcat = _radial_head_args(R, idx_c, idx_a, freq, z, nrm, wcat)
    W = torch.empty((E, 3), device=R.device, dtype=torch.float32)
    check(_lib.load().gn_radial_head_emb_bwd_f32(*[ptr(g) for g in gs], ptr(W_r), ptr(R), ptr(idx_c), ptr(idx_a), ptr(freq),
                                                 ptr(z), ptr(nrm), ptr(wcat), ptr(W), E, NR, S, NI, NE, cutoff, p, stream()),
          "gn_radial_head_emb_bwd_f32")
    return W


def trip_basis_fwd(R, tc, ta, tb, S, want_theta=False):
    """-> Y (T,S) = Y_l0(angle c<-a->b), theta (T,)|None   (gemnet.py:288-311,420-451 + basis_layers.py:130-131)."""
    require_device(R, tc, ta, tb)
    R = _f32c(R)
    T = tc.shape[0]
    Y = torch.empty((T, S), device=R.device, dtype=torch.float32)
    theta = torch.empty(T, device=R.device, dtype=torch.float32) if want_theta else None
    check(_lib.load().gn_trip_basis_fwd_f32(ptr(R), ptr(tc), ptr(ta), ptr(tb), ptr(Y), ptr(theta), T, S, stream()),
          "gn_trip_basis_fwd_f32")
    return Y, theta


def trip_basis_bwd(gY, R, tc, ta, tb):
    """-> Gc, Gb (T,3): dE/dR_c, dE/dR_b per triplet (dE/dR_a = -(Gc+Gb))."""
    require_device(gY, R)
    gY, R = _f32c(gY), _f32c(R)
    T, S = gY.shape
    Gc = torch.empty((T, 3), device=R.device, dtype=torch.float32)
    Gb = torch.empty((T, 3), device=R.device, dtype=torch.float32)
    check(_lib.load().gn_trip_basis_bwd_f32(ptr(gY), ptr(R), ptr(tc), ptr(ta), ptr(tb), ptr(Gc), ptr(Gb), T, S,
                                            stream()), "gn_trip_basis_bwd_f32")
    return Gc, Gb


def dist_fwd(R, id_c, id_a):
    """D (E,) = |R[id_a] - R[id_c]|   (gemnet.py:261-286)."""
    require_device(R, id_c, id_a)
    R = _f32c(R)
    D = torch.empty(id_c.shape[0], device=R.device, dtype=torch.float32)
    check(_lib.load().gn_dist_fwd_f32(ptr(R), ptr(id_c), ptr(id_a), ptr(D), id_c.shape[0], stream()), "gn_dist_fwd_f32")
    return D


def dist_bwd(gD, R, id_c, id_a):
    """-> W (E,3) = gD dD/dR_a: dE/dR = segsum(W, id_a) - segsum(W, id_c)."""
    require_device(gD, R)
    gD, R = _f32c(gD), _f32c(R)
    W = torch.empty((id_c.shape[0], 3), device=R.device, dtype=torch.float32)
    check(_lib.load().gn_dist_bwd_f32(ptr(gD), ptr(R), ptr(id_c), ptr(id_a), ptr(W), id_c.shape[0], stream()), "gn_dist_bwd_f32")
    return W


def dist_jvp(R, tR, gD, id_c, id_a, want_D=True, want_H=True):
    """Tangent pass of the distances along the position tangent tR (A,3): -> (Ddot (E,) | None, H (E,3) | None) with
    H = d/dR_a [gD dD/dR_a] (tR[a] - tR[c])."""
    require_device(R, tR)
    R, tR = _f32c(R), _f32c(tR)
    E = id_c.shape[0]
    gD = None if gD is None else _f32c(gD)
    Dd = torch.empty(E, device=R.device, dtype=torch.float32) if want_D else None
    H = torch.empty((E, 3), device=R.device, dtype=torch.float32) if want_H else None
    check(_lib.load().gn_dist_jvp_f32(ptr(R), ptr(tR), ptr(gD), ptr(id_c), ptr(id_a), ptr(Dd), ptr(H), E, stream()),
          "gn_dist_jvp_f32")
    return Dd, H


def angle_fwd(R, tc, ta, tb):
    """theta (T,) of the angle c <- a -> b   (gemnet.py:288-311, :420-451)."""
    require_device(R, tc, ta, tb)
    R = _f32c(R)
    th = torch.empty(tc.shape[0], device=R.device, dtype=torch.float32)
    check(_lib.load().gn_angle_fwd_f32(ptr(R), ptr(tc), ptr(ta), ptr(tb), ptr(th), tc.shape[0], stream()), "gn_angle_fwd_f32")
    return th


def angle_bwd(g, R, tc, ta, tb):
    """-> Gc, Gb (T,3) = g dtheta/dR_c, g dtheta/dR_b   (dtheta/dR_a = -(Gc + Gb))."""
    require_device(g, R)
    g, R = _f32c(g), _f32c(R)
    T = tc.shape[0]
    Gc = torch.empty((T, 3), device=R.device, dtype=torch.float32)
    Gb = torch.empty((T, 3), device=R.device, dtype=torch.float32)
    check(_lib.load().gn_angle_bwd_f32(ptr(g), ptr(R), ptr(tc), ptr(ta), ptr(tb), ptr(Gc), ptr(Gb), T, stream()),
          "gn_angle_bwd_f32")
    return Gc, Gb


def angle_jvp(R, tR, g, tc, ta, tb, want_theta=True, want_H=True):
    """Tangent pass of the angles along tR (A,3): -> (thdot (T,) | None, Hc, Hb (T,3) | None): the directional
    derivative of the first adjoint g dtheta/d(R_c, R_b)."""
    require_device(R, tR)
    R, tR = _f32c(R), _f32c(tR)
    T = tc.shape[0]
    g = None if g is None else _f32c(g)
    thd = torch.empty(T, device=R.device, dtype=torch.float32) if want_theta else None
    Hc = torch.empty((T, 3), device=R.device, dtype=torch.float32) if want_H else None
    Hb = torch.empty((T, 3), device=R.device, dtype=torch.float32) if want_H else None
    check(_lib.load().gn_angle_jvp_f32(ptr(R), ptr(tR), ptr(g), ptr(tc), ptr(ta), ptr(tb), ptr(thd), ptr(Hc), ptr(Hb), T,
                                       stream()), "gn_angle_jvp_f32")
    return thd, Hc, Hb


# --- the same geometry on the edge vectors V (E,3) of a periodic batch (csrc/pbc_train.hip): force training with a cell
def dist_vec_fwd(V):
    """D (E,) = |V|."""
    require_device(V)
    V = _f32c(V)
    D = torch.empty(V.shape[0], device=V.device, dtype=torch.float32)
    check(_lib.load().gn_dist_vec_fwd_f32(ptr(V), ptr(D), V.shape[0], stream()), "gn_dist_vec_fwd_f32")
    return D


def dist_vec_bwd(gD, V):
    """-> W (E,3) = gD dD/dV."""
    require_device(gD, V)
    gD, V = _f32c(gD), _f32c(V)
    W = torch.empty_like(V)
    check(_lib.load().gn_dist_vec_bwd_f32(ptr(gD), ptr(V), ptr(W), V.shape[0], stream()), "gn_dist_vec_bwd_f32")
    return W


def dist_vec_jvp(V, tV):
    """-> Ddot (E,) = V / |V| . tV: the tangent of the distances along tV (E,3)."""
    require_device(V, tV)
    V, tV = _f32c(V), _f32c(tV)
    assert tV.shape == V.shape
    Dd = torch.empty(V.shape[0], device=V.device, dtype=torch.float32)
    check(_lib.load().gn_dist_vec_jvp_f32(ptr(V), ptr(tV), ptr(Dd), V.shape[0], stream()), "gn_dist_vec_jvp_f32")
    return Dd


def angle_vec_fwd(V, red, exp):
    """theta (T,) between u = -V[red] and v = -V[exp] (the image-aware c <- a -> b)."""
    require_device(V, red, exp)
    V = _f32c(V)
    th = torch.empty(red.shape[0], device=V.device, dtype=torch.float32)
    check(_lib.load().gn_angle_vec_fwd_f32(ptr(V), ptr(red), ptr(exp), ptr(th), red.shape[0], stream()), "gn_angle_vec_fwd_f32")
    return th


def angle_vec_bwd(g, V, red, exp):
    """-> Gu, Gv (T,3) = g dtheta/du, g dtheta/dv."""
    require_device(g, V)
    g, V = _f32c(g), _f32c(V)
    T = red.shape[0]
    Gu = torch.empty((T, 3), device=V.device, dtype=torch.float32)
    Gv = torch.empty((T, 3), device=V.device, dtype=torch.float32)
    check(_lib.load().gn_angle_vec_bwd_f32(ptr(g), ptr(V), ptr(red), ptr(exp), ptr(Gu), ptr(Gv), T, stream()),
          "gn_angle_vec_bwd_f32")
    return Gu, Gv


def angle_vec_jvp(V, tV, red, exp):
    """-> thdot (T,): the tangent of the angles along tV (E,3)."""
    require_device(V, tV)
    V, tV = _f32c(V), _f32c(tV)
    assert tV.shape == V.shape
    thd = torch.empty(red.shape[0], device=V.device, dtype=torch.float32)
    check(_lib.load().gn_angle_vec_jvp_f32(ptr(V), ptr(tV), None, ptr(red), ptr(exp), ptr(thd), red.shape[0], stream()),
          "gn_angle_vec_jvp_f32")
    return thd


def pbc_force_stress_adj(gF, gS, V, id_c, id_a, batch_seg, cell, scale=-1.0):
    """-> gG (E,3): the adjoint of F = segsum(G, id_a) - segsum(G, id_c) and S = gn_pbc_stress_f32(V, G, scale) w.r.t. G, from
    gF (A,3) and gS (B,3,3) or None."""
    require_device(gF, V, cell)
    gF, V, cell = _f32c(gF), _f32c(V), _f32c(cell)
    gS = None if gS is None else _f32c(gS)
    assert gS is None or gS.shape == cell.shape
    gG = torch.empty_like(V)
    check(_lib.load().gn_pbc_force_stress_adj_f32(ptr(gF), ptr(gS), ptr(V), ptr(id_c), ptr(id_a), ptr(batch_seg), ptr(cell),
                                                  float(scale), ptr(gG), V.shape[0], stream()), "gn_pbc_force_stress_adj_f32")
    return gG


# --- ... and of the quadruplet branch on (V, Vint) (csrc/pbc_quad_train.hip): force training of GemNet-Q with a cell
def angle_vec2_fwd(U, iu, W, iw):
    """theta (T,) between u = U[iu] and v = -W[iw] (the a - b <- d angle: U = Vint, W = V)."""
    require_device(U, iu, W, iw)
    U, W = _f32c(U), _f32c(W)
    assert iw.shape == iu.shape
    th = torch.empty(iu.shape[0], device=U.device, dtype=torch.float32)
    check(_lib.load().gn_angle_vec2_fwd_f32(ptr(U), ptr(iu), ptr(W), ptr(iw), ptr(th), iu.shape[0], stream()),
          "gn_angle_vec2_fwd_f32")
    return th


def angle_vec2_bwd(g, U, iu, W, iw):
    """-> GU, GW (T,3) = g dtheta/dU[iu], g dtheta/dW[iw] per triplet."""
    require_device(g, U, W)
    g, U, W = _f32c(g), _f32c(U), _f32c(W)
    T = iu.shape[0]
    assert iw.shape == iu.shape and g.shape == (T,)
    GU = torch.empty((T, 3), device=U.device, dtype=torch.float32)
    GW = torch.empty((T, 3), device=U.device, dtype=torch.float32)
    check(_lib.load().gn_angle_vec2_bwd_f32(ptr(g), ptr(U), ptr(iu), ptr(W), ptr(iw), ptr(GU), ptr(GW), T, stream()),
          "gn_angle_vec2_bwd_f32")
    return GU, GW


def angle_vec2_jvp(U, iu, W, iw, tU, tW):
    """-> thdot (T,): the tangent of the angles along (tU, tW), shaped like (U, W); either may be None (zero)."""
    require_device(U, W)
    U, W = _f32c(U), _f32c(W)
    tU = None if tU is None else _f32c(tU)
    tW = None if tW is None else _f32c(tW)
    assert iw.shape == iu.shape and (tU is None or tU.shape == U.shape) and (tW is None or tW.shape == W.shape)
    thd = torch.empty(iu.shape[0], device=U.device, dtype=torch.float32)
    check(_lib.load().gn_angle_vec2_jvp_f32(ptr(U), ptr(iu), ptr(W), ptr(iw), ptr(tU), ptr(tW), ptr(thd), iu.shape[0], stream()),
          "gn_angle_vec2_jvp_f32")
    return thd


def quad_angles_vec_jvp(V, Vint, tV, tVint, q_ca, q_db, q_abd, intm_ab):
    """tang (Q,4) = (dPhi_cab, dTheta_cabd, 0, 0) along (tV, tVint): the tangents of the two quadruplet angles of a periodic
    batch — the double backward of gn_quad_angles_vec_bwd_f32, with its decisions at collinear and planar quadruplets
    (gn_quad_angles_vec_jvp_f32).  tV / tVint: shaped like V / Vint, either may be None (zero)."""
    require_device(V, Vint, q_ca, q_db, q_abd, intm_ab)
    V, Vint = _f32c(V), _f32c(Vint)
    tV = None if tV is None else _f32c(tV)
    tVint = None if tVint is None else _f32c(tVint)
    assert (tV is None or tV.shape == V.shape) and (tVint is None or tVint.shape == Vint.shape)
    Q = q_ca.shape[0]
    assert q_db.shape == q_abd.shape == (Q,)
    tang = torch.empty((Q, 4), device=V.device, dtype=torch.float32)
    check(_lib.load().gn_quad_angles_vec_jvp_f32(ptr(V), ptr(Vint), ptr(tV), ptr(tVint), ptr(q_ca), ptr(q_db), ptr(q_abd),
                                                 ptr(intm_ab), ptr(tang), Q, stream()), "gn_quad_angles_vec_jvp_f32")
    return tang


def direct_force(terms, V, id_swap, perm, seg_off, n_atoms, out=None):
    """-> F (n_atoms, T, 3): the force head of the direct-force model in one launch (gn_direct_force_f32).  terms (K,E,T): the
    force magnitudes of the K output blocks; V (E,3): edge vectors, not normalised; id_swap (E) int32 or None (uncoupled);
    perm (int32 or None) / seg_off (n_atoms + 1): the CSR of id_a.  `out`: written in place (every row is written)."""
    require_device(terms, V, seg_off)
    terms, V = _f32c(terms), _f32c(V)
    if terms.dim() != 3 or V.shape != (terms.shape[1], 3):
        raise ValueError(f"terms (K,E,T) and V (E,3) expected; got {tuple(terms.shape)} and {tuple(V.shape)}")
    K, E, T = (int(s) for s in terms.shape)
    for t in (id_swap, perm, seg_off):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
            raise TypeError("id_swap, perm and seg_off must be contiguous int32")
    if seg_off.shape[0] != int(n_atoms) + 1 or (id_swap is not None and id_swap.shape[0] != E) or \
            (perm is not None and perm.shape[0] != E):
        raise ValueError("index arrays do not fit (E, n_atoms)")
    if out is None:
        out = torch.empty((int(n_atoms), T, 3), device=terms.device, dtype=torch.float32)
    elif out.shape != (int(n_atoms), T, 3) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 (n_atoms, T, 3) tensor")
    check(_lib.load().gn_direct_force_f32(ptr(terms), ptr(V), ptr(id_swap), ptr(perm), ptr(seg_off), ptr(out), int(n_atoms), E,
                                          K, T, stream()), "gn_direct_force_f32")
    return out


def direct_force_bwd(gF, V, id_swap, id_a, n_atoms, out=None):
    """-> g (E, T): the adjoint of `direct_force` w.r.t. every one of its K term planes, in one launch (gn_direct_force_bwd_f32).
    gF (n_atoms, T, 3): the cotangent of F; V (E,3): edge vectors, not normalised; id_swap (E) int32 or None (uncoupled); id_a (E)
    int32: the target atom of every edge.  `out`: written in place (every element is written)."""
    require_device(gF, V, id_a)
    gF, V = _f32c(gF), _f32c(V)
    if gF.dim() != 3 or gF.shape[0] != int(n_atoms) or gF.shape[2] != 3 or V.dim() != 2 or V.shape[1] != 3:
        raise ValueError(f"gF (n_atoms,T,3) and V (E,3) expected; got {tuple(gF.shape)} and {tuple(V.shape)}")
    E, T = int(V.shape[0]), int(gF.shape[1])
    for t in (id_swap, id_a):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
            raise TypeError("id_swap and id_a must be contiguous int32")
    if id_a.shape[0] != E or (id_swap is not None and id_swap.shape[0] != E):
        raise ValueError("index arrays do not fit E")
    if out is None:
        out = torch.empty((E, T), device=V.device, dtype=torch.float32)
    elif out.shape != (E, T) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 (E, T) tensor")
    check(_lib.load().gn_direct_force_bwd_f32(ptr(gF), ptr(V), ptr(id_swap), ptr(id_a), ptr(out), int(n_atoms), E, T, stream()),
          "gn_direct_force_bwd_f32")
    return out


COL_VAR_WIDTHS = (8, 16, 32, 64, 128)


def col_var(x, idx32, acc, slot, w):
    """acc[slot] += w * torch.var(x[idx32], dim=0).mean() in float64, the gathered rows never written (gn_col_var_f32: one pass
    over memory, shifted float64 sums, a fixed grid and a fixed-order final reduction — no atomics, bit-reproducible, nothing
    read back).  x (n_src, C) float32 contiguous, C in COL_VAR_WIDTHS; idx32 (n,) int32 or None (the rows of x as they are);
    acc: a float64 device tensor.  Fewer than two rows, another width, a non-contiguous or non-float32 x raise before a launch."""
    require_device(x, idx32, acc)
    if x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous():
        raise TypeError(f"col_var: a contiguous float32 (n_src, C) array expected; got {x.dtype} {tuple(x.shape)} "
                        f"strides {tuple(x.stride())}")
    n_src, C = int(x.shape[0]), int(x.shape[1])
    if C not in COL_VAR_WIDTHS:
        raise ValueError(f"col_var: width {C} is not one of {COL_VAR_WIDTHS}")
    if idx32 is not None and (idx32.dtype != torch.int32 or idx32.dim() != 1 or not idx32.is_contiguous()):
        raise TypeError("col_var: idx must be a contiguous int32 vector")
    n = n_src if idx32 is None else int(idx32.shape[0])
    if n < 2 or n_src < 1:
        raise ValueError(f"col_var: a variance needs at least two rows; got {n}")
    if acc.dtype != torch.float64 or not acc.is_contiguous() or not 0 <= int(slot) < acc.numel():
        raise ValueError("col_var: acc must be a contiguous float64 tensor with the slot inside it")
    ws = torch.empty((_lib.GN_COL_VAR_MAX_BLOCKS * 2 * C,), device=x.device, dtype=torch.float64)
    check(_lib.load().gn_col_var_f32(ptr(x), ptr(idx32), ptr(ws), ptr(acc), n_src, n, C, int(slot), float(w), stream()),
          "gn_col_var_f32")


class ChainProgram:
    """A program for gn_chain_f32: ops over the three LDS slots of a row tile (see include/gemnet_hip.h).
    Operands named `mul/res/res2` are either an int (LDS slot) or a tensor (global (M,N))."""
    NSLOT = 2

    def __init__(self, M):
        self.M = int(M)
        self.ops = []

    def load(self, slot, src, rows=None, alpha=1.0, y2=-1, alpha2=1.0, Z2=None, mode2=0, add2=None):
        """slot <- src[rows] * alpha; optional second tensor y2 (slot) <- that * alpha2 * phi2(Z2) (as for gemm)
        [+ add2: a source term, see `source`]."""
        self.ops.append(dict(kind="load", slot=slot, src=src, rows=rows, alpha=float(alpha), y2=int(y2),
                             alpha2=float(alpha2), Z2=Z2, mode2=int(mode2), add2=add2))

    def scale(self, dst, a, alpha=1.0, Z=None, out=None, width=None, mode=0, add=None):
        """dst <- a * alpha * phi(Z) [+ add]: mode 0 phi = ssilu', 1 identity (Hadamard with Z), 2 ssilu;
        `add`: a source term (see `source`; its phis(Z) uses this op's Z)."""
        self.ops.append(dict(kind="scale", slot=dst, a_slot=a, alpha=float(alpha), Z=Z, out=out, width=width,
                             mode=int(mode), add=add))

    @staticmethod
    def source(P, Q=None, d2=False, alpha=1.0):
        """The extra summand  alpha * (ssilu''(Z) if d2 else 1) * P * Q  of the second-order sweeps (gn_chain_op.src_*);
        Z is the factor tensor of the op (stage) it is attached to.  P, Q: global (M,N) tensors (Q optional)."""
        return dict(P=P, Q=Q, mode=1 if d2 else 0, alpha=float(alpha))

    def gemm(self, W, a_slot, y_slot=-1, act=False, alpha=1.0, gadd1=None, gidx1=None, gadd2=None, gidx2=None,
             pre_out=None, mul=None, res=None, res_rows=None, beta=1.0, res2=None, beta2=1.0, out=None, packed=None,
             mul_mode=1, y2=-1, y2_src=0, alpha2=1.0, Z2=None, mode2=0, out2=None, add=None, add2=None, pre_deriv=False):
        """W: the (N,K) fp32 weight; `packed`: its split fragment form (pack_weight_split(W), format of the launch mode) if the caller
        caches it — the split-operand kernel packs on the fly otherwise.
        mul_mode (global `mul` only): 1 identity, 2 ssilu'(mul), 3 ssilu(mul).
        Second output: y2 (slot) / out2 (global) <- (y2_src ? activation output : final y) * alpha2 * phi2(Z2),
        phi2 by mode2: 0 ssilu', 1 identity, 2 ssilu (Z2 None: plain scale).
        add / add2: a source term (`source`) added to y after the mul and alpha stages (its ssilu'' factor reads the
        GLOBAL mul operand) / to the second output (ssilu'' of Z2); at most one of them per op.
        pre_deriv (with act and pre_out; split-operand kernel only): `pre_out` receives ssilu'(z) instead of z."""
        assert add is None or add2 is None, "one source term per op"
        assert not pre_deriv or (act and pre_out is not None)
        self.ops.append(dict(kind="gemm", W=W, packed=packed, a_slot=a_slot, slot=y_slot, act=bool(act), alpha=float(alpha),
                             pre_deriv=bool(pre_deriv),
                             add=add, add2=add2,
                             mul_mode=int(mul_mode), y2=int(y2), y2_src=int(y2_src), alpha2=float(alpha2), Z2=Z2,
                             mode2=int(mode2), out2=out2,
                             gadd1=gadd1, gidx1=gidx1, gadd2=gadd2, gidx2=gidx2, pre_out=pre_out, mul=mul,
                             res=res, res_rows=res_rows, beta=float(beta), res2=res2, beta2=float(beta2), out=out))

    def store(self, slot, out):
        self.ops.append(dict(kind="store", slot=slot, out=out))


def fuse_program(prog):
    """Peephole pass over a ChainProgram: SCALE ops that directly follow the GEMM producing their operand move into
    that GEMM's epilogue (every stand-alone SCALE is a full LDS round trip + barrier: 4-5 us at 18 k rows, and the
    adjoint of a residual layer used to carry three of them per two GEMMs).  Rewrites, with g the GEMM writing slot y:
      A  g; scale(y <- y * a * phi(Z))            ->  g(mul = Z, mul_mode = phi, alpha *= a)       [g: plain epilogue]
      B  g; [park]; scale(y <- y * c) ...          ->  g(final factor * c); park alpha / c
         g; scale(y <- y * c, out = T)             ->  g(final factor * c, out = T)
      C  g; ...; scale(o <- y * a2 * phi2(Z2)[, out2])  ->  g(y2 = o, alpha2 = a2, Z2, mode2, out2)
    The result computes the same values (tests/test_ops_cpu.py runs both forms through the interpreter)."""
    ops = [dict(o) for o in prog.ops]
    out = []
    i = 0
    while i < len(ops):
        g = ops[i]
        i += 1
        out.append(g)
        if g["kind"] == "load" and g["slot"] in (0, 1):
            # a LOAD produces its slot like a GEMM does: [park]; y *= c; o = y * a2 * phi2(Z2) ride on it (B, C)
            y, N = g["slot"], g["src"].shape[1]
            parks = []
            while i < len(ops) and ops[i]["kind"] == "scale" and ops[i]["slot"] == 2 and ops[i]["a_slot"] == y:
                parks.append(ops[i])
                i += 1
            while (i < len(ops) and ops[i]["kind"] == "scale" and ops[i]["slot"] == y and ops[i]["a_slot"] == y
                   and (ops[i]["width"] or N) == N and ops[i]["Z"] is None and ops[i]["out"] is None
                   and ops[i].get("add") is None and ops[i]["alpha"] != 0.0 and g["y2"] < 0):
                g["alpha"] *= ops[i]["alpha"]
                for pk in parks:
                    pk["alpha"] /= ops[i]["alpha"]
                i += 1
            if i < len(ops) and g["y2"] < 0:
                sc = ops[i]
                if (sc["kind"] == "scale" and sc["slot"] in (0, 1) and sc["slot"] != y and sc["a_slot"] == y
                        and (sc["width"] or N) == N and sc["out"] is None):
                    g.update(y2=sc["slot"], alpha2=sc["alpha"], Z2=sc["Z"], mode2=sc.get("mode", 0), add2=sc.get("add"))
                    i += 1
            out.extend(parks)
            continue
        if g["kind"] != "gemm" or g["slot"] not in (0, 1):
            continue
        y, N = g["slot"], g["W"].shape[0]

        def is_scale(o, dst, src):
            return o["kind"] == "scale" and o["slot"] == dst and o["a_slot"] == src and (o["width"] or N) == N

        def fold_factor(c):
            if g["res2"] is not None:
                g["beta2"] *= c
            elif g["res"] is not None:
                g["beta"] *= c
            else:
                g["alpha"] *= c

        # A: activation-derivative / Hadamard factor of a plain GEMM
        if (i < len(ops) and is_scale(ops[i], y, y) and ops[i]["Z"] is not None
                and g["mul"] is None and g["res"] is None and g["res2"] is None and g["out"] is None and g["y2"] < 0
                and g.get("out2") is None and g.get("add") is None and g.get("add2") is None):
            sc = ops[i]
            g["mul"], g["mul_mode"] = sc["Z"], {0: 2, 1: 1, 2: 3}[sc.get("mode", 0)]
            g["alpha"] *= sc["alpha"]
            g["out"] = sc["out"]          # the value after the mul / alpha (/ source) stages
            g["add"] = sc.get("add")      # y = a phi(Z) alpha + source: the GEMM's stage-1 source term
            i += 1
        parks = []
        while i < len(ops) and ops[i]["kind"] == "scale" and ops[i]["slot"] == 2 and ops[i]["a_slot"] == y:
            parks.append(ops[i])
            i += 1
        # B: in-place plain scales of y
        while (i < len(ops) and is_scale(ops[i], y, y) and ops[i]["Z"] is None and ops[i]["alpha"] != 0.0
               and ops[i].get("add") is None and g.get("add") is None and g["y2"] < 0 and g.get("out2") is None):
            sc = ops[i]
            if sc["out"] is not None:
                if g["out"] is not None:
                    break
                g["out"] = sc["out"]
            elif g["out"] is not None:
                break          # g already stores the unscaled value
            fold_factor(sc["alpha"])
            for pk in parks:
                pk["alpha"] /= sc["alpha"]
            i += 1
        # C: a second tensor derived from y into the other slot
        if i < len(ops) and g["y2"] < 0 and g.get("out2") is None:
            sc = ops[i]
            o = sc.get("slot")
            used = {y} | {x for x in (g["mul"], g["res"], g["res2"]) if isinstance(x, int)}
            if (sc["kind"] == "scale" and o in (0, 1) and o not in used and sc["a_slot"] == y and (sc["width"] or N) == N
                    and not (sc.get("add") is not None and g.get("add") is not None)):
                g.update(y2=o, y2_src=0, alpha2=sc["alpha"], Z2=sc["Z"], mode2=sc.get("mode", 0), out2=sc["out"],
                         add2=sc.get("add"))
                i += 1
        out.extend(parks)
    fused = ChainProgram(prog.M)
    fused.ops = out
    return fused


def _sel(x):
    """(slot, tensor) of a slot-or-global operand."""
    if x is None:
        return -1, None
    if isinstance(x, int):
        return x, None
    return -1, x


# Arithmetic of the chain GEMMs: "f32" = v_mfma_f32_16x16x4_f32 (csrc/chain.hip); "split6" / "split3" / "bf16" =
# bf16 matrix pipe with 6 / 3 / 1 products of split operands (csrc/chain2.hip; split6 is fp32-equivalent).
# nprod codes of gn_chain_split_f32: 6 / 3 / 1 products of bf16 planes; 2 = GN_CHAIN_F16X2, the two-plane fp16 form
# (three products, csrc/chain2.hip "format H").  "h3" needs its weights packed with SPLIT_FORMAT 1.
CHAIN_MODES = {"f32": 0, "split6": 6, "split3": 3, "bf16": 1, "h3": 2}
SPLIT_FORMAT = {"split6": 0, "split3": 0, "bf16": 0, "h3": 1}
# The process DEFAULT (read once; `bench.py --chain-mode` and tests replace it before any model runs).  The mode a launch runs
# in is per-call state, never a mutable global: a forward pass selects it for its own thread (`use_mode`, thread-local — the
# model's `matmul_precision`), every autograd Function records it at forward time (`ctx.mode`) and its backward — which the
# autograd engine runs on ITS thread, possibly long after the forward's context has closed and after another model with
# another precision has run — restores it from there (`ops._in_mode`, `ops_train._sweep_mode`).
DEFAULT_CHAIN_MODE = os.environ.get("GEMNET_CHAIN_MODE", "h3")
_tls = threading.local()


def current_mode():
    """Arithmetic of the chain / bilinear launches issued by this thread right now."""
    return getattr(_tls, "mode", None) or DEFAULT_CHAIN_MODE


@contextlib.contextmanager
def use_mode(mode):
    """Select the arithmetic (CHAIN_MODES) for the launches this THREAD issues inside the block; None keeps the current one."""
    if mode is None:
        yield
        return
    if mode not in CHAIN_MODES:
        raise ValueError(f"matmul_precision must be one of {sorted(CHAIN_MODES)}; got {mode!r}")
    prev = getattr(_tls, "mode", None)
    _tls.mode = mode
    try:
        yield
    finally:
        _tls.mode = prev


# Kernel layout of the "h3" launches: "tall" = csrc/chain2.hip (one 8-wave workgroup per CU on row tiles of <= 80 rows, a wave
# owns 16 columns): the default; programs that use the parking slot always take it (the library decides).
# (Tried and removed: a "wide" layout of 4 waves x 32 columns, two workgroups per CU — bit-identical, never faster:
# profiles/r4_chain_layouts.txt.)
# "row" (round 6) = csrc/chain4.hip: a wave owns 16 ROWS and all columns, the slots are fp32 register arrays, the fp16 planes of
# every GEMM operand are formed under a fresh row scale (no fp16 range limit on activations, no `h3_hazards`), only the weights
# pass through LDS (GN_CHAIN_ROW; weights packed with GN_SPLIT_F16X2_ROW = 2).  Same arithmetic ("h3": two fp16 planes, three
# products) to fp32 rounding.  Measured slower than "tall" on the batch sizes of BASELINE.json (profiles/r6_chain4_*.txt: 1 133
# row blocks on 1 024 SIMDs put two 16-row waves on one SIMD of every CU, and a wave's ds_read_b128 stream of weight fragments
# runs at ~28 B/clk) — selectable, not the default.
CHAIN_LAYOUT = os.environ.get("GEMNET_CHAIN_LAYOUT", "tall")
if CHAIN_LAYOUT not in ("tall", "row"):
    raise ValueError(f"GEMNET_CHAIN_LAYOUT must be 'tall' or 'row'; got {CHAIN_LAYOUT!r}")
# The fp16 planes of "h3" cover the magnitudes the MODEL fixes (activations, first-order adjoints dE/d.): sweeps whose
# scale follows the caller's loss (S3 / S4 and the energy-only final adjoint of force training, ops_train.py) run in this
# mode instead when the stack's mode is "h3" — bf16 planes have the fp32 exponent range.
CHAIN_MODE_LINEAR = os.environ.get("GEMNET_CHAIN_MODE_LINEAR", "split6")
assert SPLIT_FORMAT.get(CHAIN_MODE_LINEAR) == 0, "GEMNET_CHAIN_MODE_LINEAR: one of the bf16-plane modes"


def linear_mode(mode):
    """Arithmetic of the loss-scaled sweeps of a stack whose forward ran in `mode`."""
    return CHAIN_MODE_LINEAR if mode == "h3" else mode


def split_format(mode=None):
    """Packed-weight format (GN_SPLIT_*) of a chain mode in the current kernel layout; None for the f32 kernel."""
    fmt = SPLIT_FORMAT.get(mode or current_mode())
    return GN_SPLIT_F16X2_ROW if (fmt == 1 and CHAIN_LAYOUT == "row") else fmt


def pack_weight_split(W, trans=False, fmt=None):
    """(N,K) fp32 weight (or, trans, the (K,N) matrix whose transpose is the weight) -> packed planes (uint8) in the
    format of the current chain mode (`fmt`: GN_SPLIT_BF16X3 = 0 three bf16 planes, GN_SPLIT_F16X2 = 1 two fp16 planes)."""
    require_device(W)
    W = _rowmajor(W)
    if fmt is None:
        fmt = split_format() or 0
    N, Kd = (W.shape[1], W.shape[0]) if trans else (W.shape[0], W.shape[1])
    nbytes = -(-N // 16) * -(-Kd // 32) * (2 if fmt else 3) * 64 * 16
    out = torch.empty(nbytes, device=W.device, dtype=torch.uint8)
    check(_lib.load().gn_pack_weight_split_fmt(ptr(W), N, Kd, W.stride(0), int(bool(trans)), int(fmt), ptr(out), stream()),
          "gn_pack_weight_split_fmt")
    out._gn_fmt = fmt
    return out


def _op_planes(o, mode, fmt):
    """The weight planes of GEMM op `o` for a launch in `mode` (format `fmt`): its `packed`, which must be in that format (`W`
    then only carries the shape, any strides), or `W` packed now."""
    Wp = o.get("packed")
    if Wp is None:
        _mat(o["W"])
        return pack_weight_split(o["W"], fmt=fmt)
    if getattr(Wp, "_gn_fmt", 0) != fmt:
        raise RuntimeError(f"chain: weight planes packed in format {getattr(Wp, '_gn_fmt', 0)} handed to a launch in "
                           f"mode {mode!r} (format {fmt})")
    return Wp


def pack_job_table(entries):
    """Device job table (gn_pack_job) for `pack_weight_split_grouped`: entries = [(W, trans, packed uint8 tensor)]; the
    format of each job is the one its buffer was first packed in (`packed._gn_fmt`).
    -> (table tensor, total_units).  Host -> device copy: not inside a stream capture."""
    import numpy as np
    JOB = np.dtype(_lib.ABI.structs["gn_pack_job"])
    jobs = np.zeros(len(entries), dtype=JOB)
    unit = 0
    for i, (W, trans, packed) in enumerate(entries):
        W = _rowmajor(W)
        assert W.data_ptr() == entries[i][0].data_ptr(), "registered weights must have unit inner stride"
        N, Kd = (W.shape[1], W.shape[0]) if trans else (W.shape[0], W.shape[1])
        jobs[i] = (W.data_ptr(), packed.data_ptr(), N, Kd, W.stride(0), int(bool(trans)), unit, getattr(packed, "_gn_fmt", 0))
        unit += -(-N // 16) * -(-Kd // 32) * 64
    dev = entries[0][0].device
    table = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
    return table, unit


def pack_weight_split_grouped(table, n_jobs, total_units):
    check(_lib.load().gn_pack_weight_split_grouped(ptr(table), int(n_jobs), int(total_units), stream()),
          "gn_pack_weight_split_grouped")


def chain_split_supported(prog):
    """What gn_chain_split_f32 accepts: N % 16 == 0, slot 2 only as a parking slot."""
    for o in prog.ops:
        if o["kind"] == "gemm":
            N = o["W"].shape[0]
            if N % 16 or o["a_slot"] > 1 or o["y2"] > 1:
                return False
        elif o["kind"] == "scale":
            if o["a_slot"] > 1 or (o["slot"] == 2 and (o["Z"] is not None or o["out"] is not None)):
                return False
        elif o["slot"] > 1 or o.get("y2", -1) > 1:
            return False
    return True


def chain_row_supported(prog):
    """What the row-resident layout (csrc/chain4.hip) takes on top of chain_split_supported: K and every width a multiple of 16."""
    for o in prog.ops:
        if o["kind"] == "gemm":
            if o["W"].shape[1] % 16:
                return False
        elif o["kind"] == "load":
            if o["src"].shape[1] % 16:
                return False
        elif o["kind"] == "store":
            if o["out"].shape[1] % 16:
                return False
        else:
            Z, out = o["Z"], o["out"]
            w = o["width"] or (Z.shape[1] if Z is not None else out.shape[1])
            if w % 16:
                return False
    return True


def chain_is_linear(prog):
    """No activation inside: an adjoint / tangent program, every LDS-resident value is linear in the loaded rows."""
    return not any(o["kind"] == "gemm" and o["act"] for o in prog.ops)


def h3_hazards(prog):
    """Ops of a LINEAR program that the row-scaled fp16 form ("h3", csrc/chain2.hip) cannot take: the scale of a row
    in LDS is fixed by the LOAD that brought it in and inherited by what is computed from it, so an op that ADDS a
    global tensor of foreign magnitude (gathered rows, a global residual, a second-order source term) into a value that
    stays in LDS may leave the fp16 range.  Non-linear programs (activations: O(1) by the model's normalisation) carry no
    row scale and have no such restriction.  -> list of op indices."""
    if not chain_is_linear(prog):
        return []
    bad = []
    for i, o in enumerate(prog.ops):
        if o["kind"] == "gemm":
            stays = o["slot"] in (0, 1) or o.get("y2", -1) >= 0
            foreign = (o["gadd1"] is not None or o["gadd2"] is not None or o.get("add") is not None
                       or o.get("add2") is not None
                       or any(o[k] is not None and not isinstance(o[k], int) for k in ("res", "res2")))
            if stays and foreign:
                bad.append(i)
        elif o["kind"] == "scale" and o["slot"] in (0, 1) and o.get("add") is not None:
            bad.append(i)
        elif o["kind"] == "load" and o.get("add2") is not None:
            bad.append(i)
    return bad


_CHAIN_PACK = None


def _chain_packer():
    """(struct.Struct of one gn_chain_op, default field values, offset of ops[0], sizeof(op), sizeof(args)) derived from
    the ctypes mirror — `chain()` fills the argument block with one pack_into per op instead of ~50 ctypes attribute
    stores (171 us -> ~60 us of host time per launch: the eager / dynamic-shape path issues 50 of them per forward+force).
    The field indices become module globals F_<name>."""
    global _CHAIN_PACK
    if _CHAIN_PACK is None:
        import struct
        from ._lib import ChainArgs, ChainOp
        code = {ctypes.c_int: "i", ctypes.c_float: "f", ctypes.c_void_p: "P"}
        names, fmt = [], "@"
        for name, ct in ChainOp._fields_:
            names.append(name)
            fmt += code[ct]
        st = struct.Struct(fmt)
        # native alignment of `struct` == the C / ctypes layout: every field lands on its ctypes offset
        probe = bytearray(ctypes.sizeof(ChainOp))
        vals = list(range(1, len(names) + 1))
        st.pack_into(probe, 0, *[float(v) if c == ctypes.c_float else v for v, (_, c) in zip(vals, ChainOp._fields_)])
        chk = ChainOp.from_buffer_copy(bytes(probe))
        assert all(getattr(chk, n) == (float(v) if c == ctypes.c_float else v)
                   for v, (n, c) in zip(vals, ChainOp._fields_)) and st.size <= ctypes.sizeof(ChainOp)
        default = [0.0 if c == ctypes.c_float else 0 for _, c in ChainOp._fields_]
        for i, n in enumerate(names):
            globals()["F_" + n] = i
            if n in ("slot", "a_slot", "mul_slot", "res_slot", "res2_slot", "y2_slot"):
                default[i] = -1
        _CHAIN_PACK = (st, default, ChainArgs.ops.offset, ctypes.sizeof(ChainOp), ctypes.sizeof(ChainArgs),
                       struct.Struct("@ii"))
    return _CHAIN_PACK


def _mat(t, cols=None):
    """Address of a contiguous fp32 2-D device tensor (the chain kernel's global operands)."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()):
        require_device(t)
        raise AssertionError("chain operands: contiguous fp32 2-D")
    if cols is not None and t.shape[1] != cols:
        raise AssertionError((tuple(t.shape), cols))
    return addr(t)


def _source(v, src, stage, cols):
    v[F_src_stage], v[F_src_mode], v[F_src_alpha] = stage, int(src["mode"]), float(src["alpha"])
    v[F_srcP] = _mat(src["P"], cols)
    v[F_srcQ] = _mat(src["Q"], cols) if src["Q"] is not None else 0


# tile height of the grouped launch (16 or 32 rows; 0 = the library's default, GN_CHAIN_GROUP_TILE_ROWS)
GROUP_TILE_ROWS = int(os.environ.get("GN_CHAIN_GROUP_TILE_ROWS", "0"))


def pack_weight_split_stacked(Ws, trans=False, fmt=None):
    """The packed planes of G equally shaped weights back to back (the operand layout of the grouped chain launch)."""
    if fmt is None:
        fmt = split_format() or 0
    W0 = Ws[0]
    N, Kd = (W0.shape[1], W0.shape[0]) if trans else (W0.shape[0], W0.shape[1])
    nbytes = -(-N // 16) * -(-Kd // 32) * (2 if fmt else 3) * 64 * 16
    out = torch.empty((len(Ws), nbytes), device=W0.device, dtype=torch.uint8)
    for g, W in enumerate(Ws):
        require_device(W)
        W = _rowmajor(W)
        assert tuple(W.shape) == tuple(W0.shape)
        check(_lib.load().gn_pack_weight_split_fmt(ptr(W), N, Kd, W.stride(0), int(bool(trans)), int(fmt), ptr(out[g]), stream()),
              "gn_pack_weight_split_fmt")
    out._gn_fmt = fmt
    return out


def chain_grouped_supported(mode=None):
    """Does the grouped launch exist for this arithmetic and kernel layout?"""
    return (mode or current_mode()) in ("h3", "split6") and CHAIN_LAYOUT == "tall"


# The forward of the atom-row stacks (AtomUpdateBlock: Dense + ResidualLayers + tail projections, M <= 4 096 rows of 128
# columns, mode "h3") runs on a kernel of its own (csrc/atom_stack.hip) with bit-identical results;
# GEMNET_ATOM_STACK=0 hands those programs to gn_chain_split_f32 like every other.
USE_ATOM_STACK = os.environ.get("GEMNET_ATOM_STACK", "1") == "1"
ATOM_STACK_MAX_ROWS = 4096     # up to here gn_chain_split_f32 runs 16-row tiles as well
ATOM_STACK_WIDTH = 128


def _atom_mat(t, M):
    return (torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == (M, ATOM_STACK_WIDTH)
            and t.is_contiguous() and t.data_ptr() % 16 == 0)


def _atom_gemm_plain(o):
    """A GEMM op of 128 x 128 with none of the operand forms the atom-row kernel leaves out."""
    return (o["kind"] == "gemm" and tuple(o["W"].shape) == (ATOM_STACK_WIDTH, ATOM_STACK_WIDTH) and o["alpha"] == 1.0
            and o["gadd1"] is None and o["gadd2"] is None and o["mul"] is None and o["res_rows"] is None
            and o["y2"] < 0 and o["Z2"] is None and o["out2"] is None and o.get("add") is None and o.get("add2") is None)


def atom_stack_match(prog, mode=None):
    """Is `prog` the forward of an atom-row MLP stack in the form csrc/atom_stack.hip runs?
         LOAD x -> 0;  GEMM W0 (act, ssilu' stored) 0 -> 1;  L in {0, 1, 2} times [GEMM W1 (act) 1 -> 0,  GEMM W2 (act) 0 -> 1 with
         the LDS residual (. + slot 1) * s];  on the last of them the stack's output and (L > 0) the optional global skip
         (. + res2) * beta2;  T in {0, 1, 2} tail GEMMs 1 -> their own output
    at width 128 -> 128, 1 <= M <= 4 096, mode "h3" in the tall layout.  -> dict(x, W [ops], z, s, res2, beta2, y, t) or None
    (gathered adds, parked or intermediate skips, a residual of the Dense, other widths / modes: not this kernel).  A program
    does not say whether it is group 0 of a grouped launch: `chain` asks this matcher for single launches only."""
    return _atom_fwd_match(prog, mode)


def _atom_fwd_match(prog, mode):
    M, ops = prog.M, prog.ops
    if not (1 <= M <= ATOM_STACK_MAX_ROWS) or (mode or current_mode()) != "h3" or CHAIN_LAYOUT != "tall":
        return None
    if len(ops) < 2 or len(ops) > 8:
        return None
    o = ops[0]
    if not (o["kind"] == "load" and o["slot"] == 0 and o["rows"] is None and o.get("alpha", 1.0) == 1.0 and o.get("y2", -1) < 0
            and o.get("Z2") is None and o.get("add2") is None and _atom_mat(o["src"], M)):
        return None
    n_main = 0
    while 1 + n_main < len(ops) and ops[1 + n_main]["kind"] == "gemm" and ops[1 + n_main]["slot"] >= 0:
        n_main += 1
    main, tails = ops[1:1 + n_main], ops[1 + n_main:]
    L = (n_main - 1) // 2
    if n_main not in (1, 3, 5) or len(tails) > 2:
        return None
    s, res2, beta2 = 1.0, None, 1.0
    for j, g in enumerate(main):
        last = j + 1 == len(main)
        if not (_atom_gemm_plain(g) and g["act"] and g.get("pre_deriv") and _atom_mat(g["pre_out"], M)
                and g["a_slot"] == (j & 1) and g["slot"] == 1 - (j & 1)):
            return None
        if (g["out"] is not None) != last or (last and not _atom_mat(g["out"], M)):
            return None
        second = j > 0 and j % 2 == 0
        if second:
            if not (isinstance(g["res"], int) and g["res"] == 1 and (j == 2 or g["beta"] == s)):
                return None
            s = g["beta"]
        elif g["res"] is not None:
            return None
        if g["res2"] is not None:
            if not (second and last and _atom_mat(g["res2"], M)):
                return None
            res2, beta2 = g["res2"], g["beta2"]
    for g in tails:
        if not (_atom_gemm_plain(g) and not g["act"] and g["a_slot"] == 1 and g["slot"] < 0 and g["pre_out"] is None
                and g["res"] is None and g["res2"] is None and _atom_mat(g["out"], M)):
            return None
    return dict(x=ops[0]["src"], L=L, gemms=main + tails, z=[g["pre_out"] for g in main], s=s, res2=res2, beta2=beta2,
                y=main[-1]["out"], t=[g["out"] for g in tails])


def _atom_stack_fwd(M, m):
    """Launch gn_atom_stack_fwd_f32 for a matched program (atom_stack_match)."""
    require_device(m["x"], m["y"], m["res2"], *m["z"], *m["t"])
    Ws = [_op_planes(g, "h3", SPLIT_FORMAT["h3"]) for g in m["gemms"]]
    z, t = m["z"], m["t"]
    arr = ctypes.c_void_p
    check(_lib.load().gn_atom_stack_fwd_f32(ptr(m["x"]), int(M), int(m["L"]), len(t), (arr * len(Ws))(*[addr(W) for W in Ws]),
                                            (arr * len(z))(*[addr(a) for a in z]), float(m["s"]), ptr(m["res2"]),
                                            float(m["beta2"]), ptr(m["y"]), (arr * max(1, len(t)))(*[addr(a) for a in t]),
                                            stream()),
          "gn_atom_stack_fwd_f32")


# The first-order adjoint of those stacks (ops._Stack.backward behind fuse_program) runs on the second kernel of the same file
# (DESIGN.md section 25), bit-identical again; a switch of its own, so that GEMNET_ATOM_STACK=0 / 1 compare forwards only.
USE_ATOM_STACK_BWD = os.environ.get("GEMNET_ATOM_STACK_BWD", "1") == "1"


def _atom_adj_gemm(o):
    """A GEMM op of 128 x 128 of a first-order adjoint program: no activation, no form gn_atom_stack_bwd_f32 leaves out."""
    return (o["kind"] == "gemm" and tuple(o["W"].shape) == (ATOM_STACK_WIDTH, ATOM_STACK_WIDTH) and not o["act"]
            and not o.get("pre_deriv") and o["alpha"] == 1.0 and o["a_slot"] == 1 and o["pre_out"] is None
            and o["gadd1"] is None and o["gadd2"] is None and o["res_rows"] is None and o["res2"] is None
            and o["out2"] is None and o.get("add") is None and o.get("add2") is None and o["alpha2"] == 1.0 and o["y2_src"] == 0)


def _atom_adj_res(o, M):
    """GEMM 1 -> 0 with the running gradient as its residual: (. + slot 0) * beta."""
    return (_atom_adj_gemm(o) and o["slot"] == 0 and o["mul"] is None and type(o["res"]) is int and o["res"] == 0)


def _atom_adj_second(o, M):
    """... whose second output is slot 1 <- y * Z2 (a stored factor)."""
    return _atom_adj_res(o, M) and o["out"] is None and o["y2"] == 1 and o["mode2"] == 1 and _atom_mat(o["Z2"], M)


def _atom_adj_scale(o, dst, M, Z=False, out=False):
    """SCALE dst <- slot 0 * alpha [* Z, a stored factor] [with a global output]."""
    return (o["kind"] == "scale" and o["slot"] == dst and o["a_slot"] == 0 and o["width"] in (None, ATOM_STACK_WIDTH)
            and o.get("add") is None and (_atom_mat(o["Z"], M) and o.get("mode", 0) == 1 and o["alpha"] == 1.0 if Z else o["Z"] is None)
            and (_atom_mat(o["out"], M) if out else o["out"] is None))


def _atom_seed(seed, M):
    """(g_E (M,1), w_out (G,128)): the operands of a LOAD that forms the energy head's adjoint itself (grouped launch only)."""
    return (isinstance(seed, tuple) and len(seed) == 2 and all(torch.is_tensor(t) and t.dtype == torch.float32 and t.is_contiguous()
                                                              for t in seed)
            and tuple(seed[0].shape) == (M, 1) and seed[1].dim() == 2 and seed[1].shape[1] == ATOM_STACK_WIDTH
            and seed[1].data_ptr() % 16 == 0)


def atom_stack_adjoint_match(prog, mode=None):
    """Is `prog` the FUSED first-order adjoint of an atom-row stack in a form csrc/atom_stack.hip runs?  With G = slot 0, X = slot 1:
         T = 2:  LOAD g -> G;  LOAD gt1 -> X, GEMM (. + G) * beta -> G;  LOAD gt2 -> X, GEMM (. + G) * beta -> G
                 form 0: that GEMM's second output X = G * Z        form 1: its output g_skip, SCALE G *= a, SCALE X = G * Z
         T = 0:  form 0: LOAD g * alpha -> G with the second tensor X = G * Z
                 form 1: LOAD g -> G, SCALE G *= a with output g_skip, SCALE G *= a, SCALE X = G * Z
         L in {1, 2} times [GEMM X -> X times a stored factor;  GEMM (. + G) * beta -> G, second output X = G * Z];  GEMM X -> gx
    at width 128 -> 128, 1 <= M <= 4 096, mode "h3", tall layout, factors stored as ssilu'(z).  -> the operands of
    gn_atom_stack_bwd_f32, or None (running sums, parked skips, gathered adds, dz0 outputs, one tail, training sweeps, a LOAD
    that carries a `seed`: the chain launch).  Like atom_stack_match, `chain` asks it for single launches only."""
    return _atom_adjoint_match(prog, mode)


def _atom_adjoint_match(prog, mode, seeded=False):
    """seeded (the grouped matcher only): the T = 0 form 0 LOAD may carry `seed` = (g_E, w_out) in place of a cotangent tensor."""
    M, ops = prog.M, prog.ops
    if not (1 <= M <= ATOM_STACK_MAX_ROWS) or (mode or current_mode()) != "h3" or CHAIN_LAYOUT != "tall":
        return None
    if not (4 <= len(ops) <= 12) or any(o["kind"] == "store" for o in ops):
        return None

    def plain_load(o, slot):
        return (o["kind"] == "load" and o["slot"] == slot and o["rows"] is None and o.get("add2") is None and _atom_mat(o["src"], M)
                and o.get("alpha", 1.0) == 1.0 and o.get("y2", -1) < 0 and o.get("Z2") is None and o.get("seed") is None)
    o = ops[0]
    m = dict(g=None, gt=[], gemms=[], F=[], form=0, alpha0=1.0, a_out=1.0, a_s=1.0, bt=[1.0, 1.0], bl=[1.0, 1.0], g_skip=None, gx=None)
    i = 1
    if plain_load(o, 0):
        if plain_load(ops[1], 1):                                   # two tails
            if not (len(ops) >= 8 and _atom_adj_res(ops[2], M) and ops[2]["out"] is None and ops[2]["y2"] < 0 and ops[2]["Z2"] is None
                    and plain_load(ops[3], 1) and _atom_adj_res(ops[4], M)):
                return None
            m["gt"], m["gemms"], m["bt"] = [ops[1]["src"], ops[3]["src"]], [ops[2], ops[4]], [ops[2]["beta"], ops[4]["beta"]]
            t = ops[4]
            if _atom_adj_second(t, M):
                m["F"].append(t["Z2"])
                i = 5
            elif (_atom_mat(t["out"], M) and t["y2"] < 0 and t["Z2"] is None and _atom_adj_scale(ops[5], 0, M)
                  and _atom_adj_scale(ops[6], 1, M, Z=True)):
                m.update(form=1, g_skip=t["out"], a_s=ops[5]["alpha"])
                m["F"].append(ops[6]["Z"])
                i = 7
            else:
                return None
        elif (_atom_adj_scale(ops[1], 0, M, out=True) and _atom_adj_scale(ops[2], 0, M) and _atom_adj_scale(ops[3], 1, M, Z=True)):
            m.update(form=1, g_skip=ops[1]["out"], a_out=ops[1]["alpha"], a_s=ops[2]["alpha"])
            m["F"].append(ops[3]["Z"])
            i = 4
        else:
            return None
    elif (o["kind"] == "load" and o["slot"] == 0 and o["rows"] is None and o.get("add2") is None
          and (_atom_mat(o["src"], M) if o.get("seed") is None else seeded and _atom_seed(o["seed"], M))
          and o.get("y2", -1) == 1 and o.get("alpha2", 1.0) == 1.0 and o.get("mode2", 0) == 1 and _atom_mat(o.get("Z2"), M)):
        m["alpha0"] = o.get("alpha", 1.0)
        m["F"].append(o["Z2"])
    else:
        return None
    m["g"], m["seed"] = o["src"], o.get("seed")
    main = ops[i:]
    L = (len(main) - 1) // 2
    if len(main) not in (3, 5):
        return None
    for k in range(L):
        a, b = main[2 * k], main[2 * k + 1]
        if not (_atom_adj_gemm(a) and a["slot"] == 1 and a["res"] is None and a["out"] is None and a["y2"] < 0 and a["Z2"] is None
                and a["mul_mode"] == 1 and _atom_mat(a["mul"], M) and _atom_adj_second(b, M)):
            return None
        m["F"] += [a["mul"], b["Z2"]]
        m["bl"][k] = b["beta"]
    f = main[-1]
    if not (_atom_adj_gemm(f) and f["slot"] < 0 and f["mul"] is None and f["res"] is None and f["y2"] < 0 and f["Z2"] is None
            and _atom_mat(f["out"], M)):
        return None
    m["gemms"] = m["gemms"] + list(main)
    m.update(L=L, gx=f["out"])
    return m


def _atom_stack_bwd(M, m):
    """Launch gn_atom_stack_bwd_f32 for a matched program (atom_stack_adjoint_match)."""
    require_device(m["g"], m["gx"], m["g_skip"], *m["gt"], *m["F"])
    Ws = [_op_planes(g, "h3", SPLIT_FORMAT["h3"]) for g in m["gemms"]]
    gt, F = m["gt"], m["F"]
    arr = ctypes.c_void_p
    check(_lib.load().gn_atom_stack_bwd_f32(ptr(m["g"]), int(M), int(m["L"]), len(gt), int(m["form"]),
                                            (arr * max(1, len(gt)))(*[addr(a) for a in gt]), (arr * len(Ws))(*[addr(W) for W in Ws]),
                                            (arr * len(F))(*[addr(a) for a in F]), float(m["alpha0"]), float(m["a_out"]),
                                            float(m["a_s"]), float(m["bt"][0]), float(m["bt"][1]), float(m["bl"][0]),
                                            float(m["bl"][1]), ptr(m["g_skip"]), ptr(m["gx"]), stream()),
          "gn_atom_stack_bwd_f32")


# The stage of the grouped OutputBlocks (ops._OutputGroup: G stacks of Dense + ResidualLayers on A atom rows each, and their
# adjoint) on grouped launches of the same two kernels, bit-identical to gn_chain_split_grouped_f32; the
# adjoint forms the energy head's seed in its LOAD.  A switch of its own, independent of the two above.
USE_ATOM_STACK_GROUPED = os.environ.get("GEMNET_OUT_GROUP_ATOMS", "1") == "1"
ATOM_STACK_PLANE_BYTES = 8 * 4 * 2 * 64 * 16      # one packed 128 x 128 weight of format "h3"


def _atom_slabs(t, M, groups, group_pitch):
    """Is `t` (group 0's slab) followed, in its own storage, by the slabs of the other groups?"""
    need = (t.storage_offset() + ((groups - 1) * group_pitch + M) * ATOM_STACK_WIDTH) * t.element_size()
    return need <= t.untyped_storage().nbytes()


def atom_stack_grouped_match(prog, groups, group_pitch, mode=None):
    """Is the grouped launch `chain(prog, groups=, group_pitch=)` the forward or the fused adjoint of the grouped output-block stage in
    the form csrc/atom_stack.hip runs?  The program of group 0 must be one atom_stack_match / atom_stack_adjoint_match accept, with
         forward: L in {1, 2}, no tails, no skip (an activation on the Dense: every form of the kernel has one)
         adjoint: L in {1, 2}, T = 0, form 0 — LOAD g * alpha -> G with the second tensor X = G * Z; the LOAD's cotangent is a tensor
                  or `seed` = (g_E (M,1), w_out (G,128)) (ops._OutputGroup.backward)
    1 <= G <= 8, group_pitch >= M, every `packed` the (G, 65 536) stacked planes of pack_weight_split_stacked in format "h3", every row
    operand followed by the other groups' slabs.  -> ("fwd" | "bwd", operands) or None (the grouped chain launch)."""
    M = prog.M
    if not (1 <= groups <= GN_CHAIN_MAX_GROUPS and group_pitch >= M >= 1):
        return None
    m, kind = _atom_fwd_match(prog, mode), "fwd"
    if m is not None:
        if m["L"] < 1 or m["t"] or m["res2"] is not None:
            return None
        rows = [m["x"], m["y"], *m["z"]]
    else:
        m, kind = _atom_adjoint_match(prog, mode, seeded=True), "bwd"
        if m is None or m["form"] != 0 or m["gt"] or m["g_skip"] is not None:
            return None
        if m["seed"] is not None and m["seed"][1].shape[0] != groups:
            return None
        rows = [m["gx"], *m["F"]] + ([m["g"]] if m["seed"] is None else [])
    for g in m["gemms"]:
        Wp = g.get("packed")
        if not (torch.is_tensor(Wp) and tuple(Wp.shape) == (groups, ATOM_STACK_PLANE_BYTES) and Wp.is_contiguous()
                and Wp.data_ptr() % 16 == 0 and getattr(Wp, "_gn_fmt", 0) == SPLIT_FORMAT["h3"]):
            return None
    if not all(_atom_slabs(t, M, groups, group_pitch) for t in rows):
        return None
    return kind, m


def _atom_stack_grouped(M, groups, group_pitch, kind, m):
    """Launch gn_atom_stack_fwd_grouped_f32 / gn_atom_stack_bwd_grouped_f32 for a matched program (atom_stack_grouped_match)."""
    arr = ctypes.c_void_p
    Ws = [g["packed"] for g in m["gemms"]]
    span = ((int(groups) - 1) * int(group_pitch) + int(M)) * ATOM_STACK_WIDTH * 4
    if kind == "fwd":
        reads, writes = [m["x"]], [m["y"], *m["z"]]
    else:
        reads, writes = [*m["F"]] + ([m["g"]] if m["seed"] is None else []), [m["gx"]]
    require_device(*reads, *writes, *Ws, *(m.get("seed") or ()))
    if _lib.TRACE is not None:
        # the arguments name group 0's slab of every row operand; the launch touches all of them (hbcheck.py)
        _lib.note(reads=[(t.data_ptr(), span) for t in reads], writes=[(t.data_ptr(), span) for t in writes])
    W_arr = (arr * len(Ws))(*[addr(W) for W in Ws])
    if kind == "fwd":
        z = m["z"]
        check(_lib.load().gn_atom_stack_fwd_grouped_f32(ptr(m["x"]), int(M), int(groups), int(group_pitch), int(m["L"]), W_arr,
                                                        (arr * len(z))(*[addr(a) for a in z]), float(m["s"]), ptr(m["y"]), stream()),
              "gn_atom_stack_fwd_grouped_f32")
        return
    F, seed = m["F"], m["seed"] or (None, None)
    check(_lib.load().gn_atom_stack_bwd_grouped_f32(ptr(m["g"]) if m["seed"] is None else None, ptr(seed[0]), ptr(seed[1]), int(M),
                                                    int(groups), int(group_pitch), int(m["L"]), W_arr,
                                                    (arr * len(F))(*[addr(a) for a in F]), float(m["alpha0"]), float(m["bl"][0]),
                                                    float(m["bl"][1]), ptr(m["gx"]), stream()),
          "gn_atom_stack_bwd_grouped_f32")


def chain(prog, mode=None, groups=0, group_pitch=0, tile_rows=None):
    """Run a ChainProgram (one launch).
    groups > 0 (gn_chain_split_grouped_f32): `prog` describes group 0 — M rows, operands = the first slab of stacked tensors
    whose slabs lie `group_pitch` rows apart, every `packed` = the G packed weights back to back (pack_weight_split_stacked)."""
    from ._lib import GN_OP_GEMM, GN_OP_LOAD, GN_OP_SCALE, GN_OP_STORE
    ops = prog.ops
    if len(ops) > GN_CHAIN_MAX_OPS:
        raise ValueError("chain program too long")
    mode = mode or current_mode()
    if USE_ATOM_STACK and not groups and prog.M <= ATOM_STACK_MAX_ROWS:
        m = atom_stack_match(prog, mode)
        if m is not None:
            return _atom_stack_fwd(prog.M, m)
    if USE_ATOM_STACK_BWD and not groups and prog.M <= ATOM_STACK_MAX_ROWS:
        m = atom_stack_adjoint_match(prog, mode)
        if m is not None:
            return _atom_stack_bwd(prog.M, m)
    if USE_ATOM_STACK_GROUPED and groups and tile_rows is None and prog.M <= ATOM_STACK_MAX_ROWS:     # (a tile height asks for the chain kernel)
        m = atom_stack_grouped_match(prog, groups, group_pitch, mode)
        if m is not None:
            return _atom_stack_grouped(prog.M, groups, group_pitch, *m)
    if any(o["kind"] == "load" and o.get("seed") is not None for o in ops):
        raise RuntimeError("chain: a LOAD that forms its rows from `seed` exists on the grouped atom-row kernel only "
                           "(kernels.atom_stack_grouped_match refused this program, a tile height was asked for, or GEMNET_OUT_GROUP_ATOMS=0)")
    nprod = CHAIN_MODES[mode]
    if nprod and not chain_split_supported(prog):
        nprod = 0
    if groups and not (nprod and chain_grouped_supported(mode)):
        raise RuntimeError(f"chain: no grouped launch in mode {mode!r} / layout {CHAIN_LAYOUT!r} for this program")
    fmt = SPLIT_FORMAT.get(mode, 0)
    row = nprod == CHAIN_MODES["h3"] and CHAIN_LAYOUT == "row"
    if row and not chain_row_supported(prog):
        raise RuntimeError("chain: the row-resident layout needs K and every width to be a multiple of 16 "
                           "(GEMNET_CHAIN_LAYOUT=tall runs other shapes)")
    if row:
        fmt = GN_SPLIT_F16X2_ROW
    if nprod == CHAIN_MODES["h3"] and not row and h3_hazards(prog):
        raise RuntimeError("chain: this linear program adds a global tensor into an LDS-resident value "
                           f"(ops {h3_hazards(prog)}): not representable in the row-scaled fp16 form 'h3' — "
                           "launch it in kernels.linear_mode('h3')")
    st, default, ops_off, op_size, args_size, hdr = _chain_packer()
    keep = []
    buf = bytearray(args_size)
    M = prog.M
    hdr.pack_into(buf, 0, M, len(ops))
    has_src = False
    off = ops_off
    for o in ops:
        v = default[:]
        kind = o["kind"]
        if kind == "gemm":
            W = o["W"]
            N, Kd = W.shape
            if nprod:
                Wp = _op_planes(o, mode, fmt)
                keep.append(Wp)
                v[F_W] = addr(Wp)
            else:
                v[F_W] = _mat(W)
            v[F_kind], v[F_N], v[F_K], v[F_a_slot], v[F_slot] = GN_OP_GEMM, N, Kd, o["a_slot"], o["slot"]
            v[F_act], v[F_alpha], v[F_beta], v[F_beta2] = int(o["act"]) | (2 if o.get("pre_deriv") else 0), o["alpha"], o["beta"], o["beta2"]
            if o.get("pre_deriv") and not nprod:
                raise RuntimeError("chain: pre_deriv needs the split-operand kernel (not CHAIN_MODE 'f32')")
            t = o["gadd1"]
            if t is not None:
                v[F_gadd1], v[F_gidx1] = _mat(t, N), addr(o["gidx1"])
            t = o["gadd2"]
            if t is not None:
                v[F_gadd2], v[F_gidx2] = _mat(t, N), addr(o["gidx2"])
            t = o["pre_out"]
            if t is not None:
                v[F_pre_out] = _mat(t, N)
            t = o["out"]
            if t is not None:
                v[F_out] = _mat(t, N)
            t = o["mul"]
            if t is not None:
                if isinstance(t, int):
                    v[F_mul_slot] = t
                else:
                    v[F_mul_g] = _mat(t, N)
            t = o["res"]
            if t is not None:
                if isinstance(t, int):
                    v[F_res_slot] = t
                else:
                    v[F_res_g] = _mat(t, N)
            t = o["res2"]
            if t is not None:
                if isinstance(t, int):
                    v[F_res2_slot] = t
                else:
                    v[F_res2_g] = _mat(t, N)
            t = o["res_rows"]
            if t is not None:
                v[F_res_rows] = addr(t)
            mm = o["mul_mode"]
            v[F_mul_mode], v[F_y2_slot], v[F_y2_src], v[F_mode2], v[F_alpha2] = mm, o["y2"], o["y2_src"], o["mode2"], o["alpha2"]
            t = o["Z2"]
            if t is not None:
                v[F_Z2] = _mat(t, N)
            t = o["out2"]
            if t is not None:
                v[F_out2] = _mat(t, N)
            if mm > 1:
                assert v[F_mul_slot] < 0 and v[F_mul_g], "mul_mode applies to a global mul operand"
            t = o.get("add")
            if t is not None:
                _source(v, t, 1, N)
                has_src = True
            t = o.get("add2")
            if t is not None:
                _source(v, t, 2, N)
                has_src = True
        elif kind == "load":
            src = o["src"]
            sp = _mat(src)
            assert o["rows"] is not None or src.shape[0] == M
            w = src.shape[1]
            v[F_kind], v[F_slot], v[F_width], v[F_ld], v[F_src] = GN_OP_LOAD, o["slot"], w, src.stride(0), sp
            t = o["rows"]
            if t is not None:
                v[F_rows] = addr(t)
            v[F_alpha], v[F_y2_slot], v[F_alpha2], v[F_mode2] = o.get("alpha", 1.0), o.get("y2", -1), o.get("alpha2", 1.0), o.get("mode2", 0)
            t = o.get("Z2")
            if t is not None:
                v[F_Z2] = _mat(t, w)
            t = o.get("add2")
            if t is not None:
                _source(v, t, 2, w)
                has_src = True
        elif kind == "scale":
            Z, out = o["Z"], o["out"]
            w = o["width"] or (Z.shape[1] if Z is not None else out.shape[1])
            v[F_kind], v[F_slot], v[F_a_slot], v[F_width], v[F_ld] = GN_OP_SCALE, o["slot"], o["a_slot"], w, w
            v[F_alpha], v[F_act] = o["alpha"], o.get("mode", 0)
            if Z is not None:
                v[F_src] = _mat(Z, w)
            if out is not None:
                v[F_out] = _mat(out, w)
            t = o.get("add")
            if t is not None:
                _source(v, t, 1, w)
                has_src = True
        else:   # store
            out = o["out"]
            v[F_kind], v[F_slot], v[F_width], v[F_ld], v[F_out] = GN_OP_STORE, o["slot"], out.shape[1], out.stride(0), _mat(out)
        st.pack_into(buf, off, *v)
        off += op_size
    if has_src and not nprod:
        raise RuntimeError("chain programs with second-order source terms run on the split-operand kernel only "
                           "(CHAIN_MODE f32 / an unsupported shape): use the composite training path")
    cbuf = (ctypes.c_char * args_size).from_buffer(buf)
    if row:
        nprod |= GN_CHAIN_ROW
    if groups:
        if _lib.TRACE is not None:
            # the argument block names group 0's slab of every operand; the launch touches all `groups` slabs, `group_pitch`
            # rows apart, and the stacked packed weights: declared as regions (hbcheck.py)
            reads, writes = [], []
            for o in ops:
                for key, t in o.items():
                    if key == "packed" and t is not None:
                        reads.append((t.data_ptr(), t.numel() * t.element_size()))
                    elif torch.is_tensor(t) and key not in ("W", "packed") and t.dim() == 2:
                        span = ((int(groups) - 1) * int(group_pitch) + t.shape[0]) * t.stride(0) * t.element_size()
                        (writes if key in ("pre_out", "out", "out2") else reads).append((t.data_ptr(), span))
            _lib.note(reads=reads, writes=writes)
        check(_lib.load().gn_chain_split_grouped_f32(ctypes.addressof(cbuf), nprod, int(groups), int(group_pitch),
                                                     GROUP_TILE_ROWS if tile_rows is None else int(tile_rows), stream()),
              "gn_chain_split_grouped_f32")
    elif nprod:
        check(_lib.load().gn_chain_split_f32(ctypes.addressof(cbuf), nprod, stream()), "gn_chain_split_f32")
    else:
        check(_lib.load().gn_chain_f32(ctypes.addressof(cbuf), stream()), "gn_chain_f32")


def bil_train_supported(S, C, I):
    """Shapes for which the bilinear layer has its fused twice-differentiable training form (ops_train._Bilinear2): the
    spherical basis of the triplet interaction (the extended K1 + K2 kernel gn_bil_reduce_project2_f32)."""
    return (S, C, I) == (7, 64, 16)


def bil_reduce_project(Y, x, B, sp, Sm_init=None, B2=None, Sm2=None, want_P=True):
    """Fused K1+K2 -> (Sm (E,S,C), P (E,I,C)); B = rbf_W1 (E,S,I).
    Extended form (gn_bil_reduce_project2_f32, spherical-basis shapes only): Sm starts from `Sm_init` instead of zero,
    P = B^T Sm + B2^T Sm2 (a second K2 term from given blocks), `want_P=False` skips K2 — the tangent sweep of the
    training step: dSm = K1(dY, x) + K1(Y, dx), dP = B^T dSm + dB^T Sm."""
    require_device(Y, x, B)
    Y, x, B = _f32c(Y), _f32c(x), _f32c(B)
    S, C, I = B.shape[1], x.shape[1], B.shape[2]
    Sm = torch.empty((sp.n_reduce, S, C), device=x.device, dtype=torch.float32)
    P = torch.empty((sp.n_reduce, I, C), device=x.device, dtype=torch.float32) if want_P else None
    if Sm_init is not None or B2 is not None or not want_P:
        assert bil_train_supported(S, C, I) and not is_angle_form(Y, S) and (B2 is None) == (Sm2 is None)
        ts = [None if t is None else _f32c(t) for t in (Sm_init, B2, Sm2)]
        assert ts[0] is None or ts[0].shape == Sm.shape
        assert ts[1] is None or (ts[1].shape == B.shape and ts[2].shape == Sm.shape)
        check(_lib.load().gn_bil_reduce_project2_f32(ptr(Y), ptr(x), ptr(sp.expand.idx32), ptr(sp.seg_off), ptr(B),
                                                     ptr(ts[0]), ptr(ts[1]), ptr(ts[2]), ptr(Sm), ptr(P), sp.n_reduce,
                                                     S, C, I, stream()), "gn_bil_reduce_project2_f32")
        return Sm, P
    if is_angle_form(Y, S):   # Y_lm rebuilt in-kernel from (sin, cos) of the two angles
        # K1 on the fp16 pipe takes x unscaled (fp16 range): only under the fp16-plane Dense arithmetic, whose overflow guard
        # (model/gemnet.py) covers it — a model on "split6" / "f32" keeps the f32-input MFMA here (`arith` is an argument of
        # the launch: no library state)
        arith = GN_ANG_F16 if (ANG_F16_MASK & 1 and current_mode() == "h3") else 0
        check(_lib.load().gn_bil_reduce_project_ang_f32(ptr(Y), ptr(x), ptr(sp.expand.idx32), ptr(sp.seg_off), ptr(B),
                                                        ptr(Sm), ptr(P), sp.n_reduce, S, C, I, arith, stream()),
              "gn_bil_reduce_project_ang_f32")
        return Sm, P
    check(_lib.load().gn_bil_reduce_project_f32(ptr(Y), ptr(x), ptr(sp.expand.idx32), ptr(sp.seg_off), ptr(B),
                                                ptr(Sm), ptr(P), sp.n_reduce, S, C, I, stream()),
          "gn_bil_reduce_project_f32")
    return Sm, P


USE_K3_F16 = os.environ.get("GEMNET_K3_F16", "1") == "1"


def bil_fused_fwd(Y, x, B, W2T, sp, alpha=1.0, W2T_planes=None, up=None):
    """K1+K2+K3 in one launch -> (Sm (E,S,C), out (E,O)); W2T (O, I*C) = the bilinear weight, k-contiguous.
    W2T_planes: pack_weight_split(W2T, fmt=1) — K3 then runs on the fp16 matrix pipe with split operands.
    Spherical basis only (S, C, I, O) = (7, 64, 16, 64); see `bil_fused_fwd_supported`.
    `up` = dict(planes=pack_weight_split(cat(W_ac, W_ca), fmt=1), act, alpha): the up-projection pair of the interaction
    tail runs as one more phase of the launch (gn_bil_up_fwd_f32) -> (Sm, z_ac, z_ca, y_ac, y_ca), z_* None without
    activation; `out` is not formed.  Needs W2T_planes."""
    require_device(Y, x, B, W2T)
    Y, x, B, W2T = _f32c(Y), _f32c(x), _f32c(B), _f32c(W2T)
    S, C, I, O = Y.shape[1], x.shape[1], B.shape[2], W2T.shape[0]
    Sm = torch.empty((sp.n_reduce, S, C), device=x.device, dtype=torch.float32)
    if up is not None:
        planes, act, N = up["planes"], bool(up["act"]), UP_PAIR_WIDTH
        if not (USE_K3_F16 and W2T_planes is not None and getattr(W2T_planes, "_gn_fmt", None) == 1
                and W2T_planes.numel() == 4 * 32 * 2 * 64 * 16):
            raise RuntimeError("bil_fused_fwd(up=...): the up-projection phase needs the fp16 planes of the bilinear weight")
        assert getattr(planes, "_gn_fmt", None) == 1 and planes.numel() == 16 * 2 * 2 * 64 * 16
        E = sp.n_reduce
        z_ac, z_ca = (torch.empty((E, N), device=x.device, dtype=torch.float32) for _ in range(2)) if act else (None, None)
        y_ac, y_ca = (torch.empty((E, N), device=x.device, dtype=torch.float32) for _ in range(2))
        check(_lib.load().gn_bil_up_fwd_f32(ptr(Y), ptr(x), ptr(sp.expand.idx32), ptr(sp.seg_off), ptr(B), ptr(W2T_planes),
                                            ptr(planes), ptr(Sm), ptr(z_ac), ptr(z_ca), ptr(y_ac), ptr(y_ca), E, S, C, I, O, N,
                                            float(alpha), float(up["alpha"]), int(act), stream()), "gn_bil_up_fwd_f32")
        return Sm, z_ac, z_ca, y_ac, y_ca
    out = torch.empty((sp.n_reduce, O), device=x.device, dtype=torch.float32)
    if W2T_planes is not None:
        assert getattr(W2T_planes, "_gn_fmt", None) == 1 and W2T_planes.numel() == 4 * 32 * 2 * 64 * 16
    check(_lib.load().gn_bil_fused_fwd_f32(ptr(Y), ptr(x), ptr(sp.expand.idx32), ptr(sp.seg_off), ptr(B), ptr(W2T),
                                           ptr(W2T_planes) if USE_K3_F16 else None,
                                           ptr(Sm), ptr(out), sp.n_reduce, S, C, I, O, float(alpha), stream()),
          "gn_bil_fused_fwd_f32")
    return Sm, out


def bil_fused_fwd_supported(S, C, I, O):
    return (S, C, I, O) == (7, 64, 16, 64)


UP_PAIR_WIDTH = 128     # width of the two up projections the bilinear kernels can carry


def bil_up_supported(S, C, I, O, N_up, K_up):
    """Shapes for which the up-projection pair rides in the fused bilinear launches (`up=` of bil_fused_fwd / bil_fused_bwd)."""
    return (S, C, I, O) == (7, 64, 16, 64) and (N_up, K_up) == (UP_PAIR_WIDTH, O)


def is_angle_form(Y, S):
    """The tensor basis given as (Q,4) = (sin, cos) of Phi_cab and Theta_cabd instead of the (Q,49) harmonics."""
    return S == 49 and Y.dim() == 2 and Y.shape[1] == 4


def quad_angles_fwd(R, qc, qa, qb, qd):
    """-> ang (Q,4): (sin, cos) of the polar angle Phi_cab and of the azimuth Theta_cabd (gemnet.py:334-418)."""
    require_device(R, qc, qa, qb, qd)
    R = _f32c(R)
    Q = qc.shape[0]
    ang = torch.empty((Q, 4), device=R.device, dtype=torch.float32)
    check(_lib.load().gn_quad_angles_fwd_f32(ptr(R), ptr(qc), ptr(qa), ptr(qb), ptr(qd), ptr(ang), Q, stream()),
          "gn_quad_angles_fwd_f32")
    return ang


def quad_angles_bwd(g_ang, R, qc, qa, qb, qd, packed=False):
    """g_ang (Q,4) = (dE/dPhi_cab, dE/dTheta_cabd, -, -) -> (Gc, Gb, Gd) (Q,3) each, or packed: Gc and
    Gbd (Q,8) = [Gb xyz, 0, Gd xyz, 0]."""
    require_device(g_ang, R)
    g_ang, R = _f32c(g_ang), _f32c(R)
    Q = qc.shape[0]
    Gc = torch.empty((Q, 3), device=R.device, dtype=torch.float32)
    if packed:
        Gbd = torch.empty((Q, 8), device=R.device, dtype=torch.float32)      # (the kernel writes the two pad lanes itself)
        base = addr(Gbd)
        check(_lib.load().gn_quad_angles_bwd_ld_f32(ptr(g_ang), ptr(R), ptr(qc), ptr(qa), ptr(qb), ptr(qd), ptr(Gc), 3,
                                                    base, 8, base + 16, 8, Q, stream()), "gn_quad_angles_bwd_ld_f32")
        return Gc, Gbd
    Gb, Gd = torch.empty_like(Gc), torch.empty_like(Gc)
    check(_lib.load().gn_quad_angles_bwd_ld_f32(ptr(g_ang), ptr(R), ptr(qc), ptr(qa), ptr(qb), ptr(qd), ptr(Gc), 3,
                                                ptr(Gb), 3, ptr(Gd), 3, Q, stream()), "gn_quad_angles_bwd_ld_f32")
    return Gc, Gb, Gd


def quad_angles_jvp(R, tR, qc, qa, qb, qd):
    """tang (Q,4) = (dPhi_cab . tR, dTheta_cabd . tR, 0, 0): the tangents of the two quadruplet angles along the position
    tangent tR (A,3) — the double backward of `quad_angles_bwd` (gn_quad_angles_jvp_f32)."""
    require_device(R, tR, qc, qa, qb, qd)
    R, tR = _f32c(R), _f32c(tR)
    Q = qc.shape[0]
    tang = torch.empty((Q, 4), device=R.device, dtype=torch.float32)
    check(_lib.load().gn_quad_angles_jvp_f32(ptr(R), ptr(tR), ptr(qc), ptr(qa), ptr(qb), ptr(qd), ptr(tang), Q, stream()),
          "gn_quad_angles_jvp_f32")
    return tang


def bil_reduce_project_tan(ang, tang, x, tx, B, tB, Sm, sp, want_P=True):
    """Tangent sweep S3 of the quadruplet bilinear layer in ONE launch (gn_bil_reduce_project_ang_tan_f32):
    Smd[e] = sum_q (dY[q] (x) x[g(q)] + Y[q] (x) tx[g(q)]),  Pd[e] = B[e]^T Smd[e] + tB[e]^T Sm[e];  dY from the angle tangents
    `tang` (Q,4).  tang / tx / tB may be None (at least one of tang, tx) -> (Smd (E,S,C), Pd (E,I,C) | None)."""
    require_device(ang, x, B)
    assert tang is not None or tx is not None
    ang, x, B = _f32c(ang), _f32c(x), _f32c(B)
    tang, tx, tB, Sm = (None if t is None else _f32c(t) for t in (tang, tx, tB, Sm))
    S, C, I = B.shape[1], x.shape[1], B.shape[2]
    assert is_angle_form(ang, S) and (tang is None or tang.shape == ang.shape) and (tx is None or tx.shape == x.shape)
    assert tB is None or (tB.shape == B.shape and Sm is not None and Sm.shape == (sp.n_reduce, S, C))
    Smd = torch.empty((sp.n_reduce, S, C), device=x.device, dtype=torch.float32)
    Pd = torch.empty((sp.n_reduce, I, C), device=x.device, dtype=torch.float32) if want_P else None
    check(_lib.load().gn_bil_reduce_project_ang_tan_f32(ptr(ang), ptr(tang), ptr(x), ptr(tx), ptr(sp.expand.idx32),
                                                        ptr(sp.seg_off), ptr(B), ptr(tB), ptr(Sm), ptr(Smd), ptr(Pd),
                                                        sp.n_reduce, S, C, I, stream()), "gn_bil_reduce_project_ang_tan_f32")
    return Smd, Pd


def bil_reduce_t_tan(ang, tang, D1, D2, sp):
    """x-adjoint of the second adjoint S4 of the quadruplet bilinear layer: dx[j] = sum_{q: g(q) = j} (Y[q] D1[r(q)] + dY[q]
    D2[r(q)]) — per-quadruplet rows by gn_bil_expand_ang_tan_f32, then the CSR sum over the expand rows.  D1 may be None."""
    require_device(ang, tang, D2)
    ang, tang, D2 = _f32c(ang), _f32c(tang), _f32c(D2)
    D1 = None if D1 is None else _f32c(D1)
    S, C = D2.shape[1], D2.shape[2]
    assert is_angle_form(ang, S) and tang.shape == ang.shape and (D1 is None or D1.shape == D2.shape)
    if sp.size == 0:      # edges without a single quadruplet: nothing to expand (empty `ang` / `tang` have no address to hand over)
        return torch.zeros((sp.n_expand, C), device=ang.device, dtype=torch.float32)
    rg = sp.row_grid if (USE_ROW_GRID and C == 32 and sp.ROW_TILE == 64) else None
    if rg is not None:
        # one pass, no per-quadruplet rows in memory (csrc/bilinear_ang.hip: bil_expand_rows_ang_tan_kernel)
        a_perm, a_seg, j_off, qmap, g_off, task_atom, task_row0, n_tasks = rg
        dx = torch.empty((sp.n_expand, C), device=ang.device, dtype=torch.float32)
        check(_lib.load().gn_bil_expand_rows_ang_tan_f32(ptr(ang), ptr(tang), ptr(D1), ptr(D2), ptr(a_perm), ptr(a_seg), ptr(j_off),
                                                         ptr(qmap), ptr(g_off), ptr(task_atom), ptr(task_row0), int(n_tasks),
                                                         ptr(dx), S, C, sp.ROW_TILE, stream()), "gn_bil_expand_rows_ang_tan_f32")
        return dx
    dxt = torch.empty((sp.size, C), device=ang.device, dtype=torch.float32)
    check(_lib.load().gn_bil_expand_ang_tan_f32(ptr(ang), ptr(tang), ptr(D1), ptr(D2), ptr(sp.seg_off), ptr(dxt), sp.n_reduce,
                                                S, C, stream()), "gn_bil_expand_ang_tan_f32")
    permT, segT = sp.expand.csr
    return segsum(dxt, permT, segT, sp.n_expand)


def bil_ang_train_supported(S, C, I):
    """Shapes of the fused twice-differentiable quadruplet bilinear layer in angle form (ops_train._BilinearAng2)."""
    return (S, C, I) == (49, 32, 32)


def bil_dy_multi(dSm_list, x_list, sp, ang=None):
    """dY (T,S) = sum_b sum_c x_b[g(t),c] dSm_b[r(t),s,c] for the blocks b that share one tensor basis (one pass).
    With `ang` (the basis in angle form): the gradient w.r.t. the two angles, (T,4), instead."""
    require_device(*dSm_list, *x_list)
    dSm_list = [_f32c(t) for t in dSm_list]
    x_list = [_f32c(t) for t in x_list]
    nb = len(dSm_list)
    E, S, C = dSm_list[0].shape
    if ang is not None:
        ang = _f32c(ang)
        g_ang = torch.empty((sp.size, 4), device=ang.device, dtype=torch.float32)
        arr = ctypes.c_void_p * nb
        check(_lib.load().gn_bil_dy_multi_ang_f32(arr(*[addr(t) for t in dSm_list]), arr(*[addr(t) for t in x_list]),
                                                  nb, ptr(ang), ptr(sp.expand.idx32), ptr(sp.seg_off), ptr(g_ang), E, S, C,
                                                  GN_ANG_F16 if ANG_F16_MASK & 2 else 0, stream()), "gn_bil_dy_multi_ang_f32")
        return g_ang
    dY = torch.empty((sp.size, S), device=x_list[0].device, dtype=torch.float32)
    arr = ctypes.c_void_p * nb
    grp = sp.groups if USE_DY_ATOMS and (S, C) == (7, 64) and nb <= 4 else None
    if grp is not None and 0 < grp[4] * S * C * 4 <= 160 * 1024:      # (the condition of the grouped launches in bil_reduce_t)
        rows, off, _kseg, _rposT, max_rows = grp
        ent_off, ent_t, ent_bc = sp.group_entries
        check(_lib.load().gn_bil_dy_atoms_f32(arr(*[addr(t) for t in dSm_list]), arr(*[addr(t) for t in x_list]), nb,
                                              ptr(rows), ptr(off), ptr(ent_off), ptr(ent_t), ptr(ent_bc),
                                              ptr(sp.expand.idx32), ptr(sp.seg_off), ptr(dY), off.shape[0] - 1, max_rows, S, C,
                                              stream()), "gn_bil_dy_atoms_f32")
        return dY
    check(_lib.load().gn_bil_dy_multi_f32(arr(*[addr(t) for t in dSm_list]), arr(*[addr(t) for t in x_list]),
                                          nb, ptr(sp.expand.idx32), ptr(sp.seg_off), ptr(dY), E, S, C, stream()),
          "gn_bil_dy_multi_f32")
    return dY


def bil_project_bwd(dP, Sm, B, x, sp, dY_accum=None, want_dY=True, gB_accum=None, dSm_accum=None):
    """Fused adjoint of K2 and of K1 w.r.t. Y -> (gB (E,S,I), dSm (E,S,C), dY (T,S)); with `dY_accum` the Y
    gradient is ADDED into that (T,S) buffer (and returned) instead of written to a fresh one; `gB_accum` / `dSm_accum`
    likewise (the cross terms of the training step's second adjoint land on the first-order ones)."""
    require_device(dP, Sm, B, x)
    dP, Sm, B, x = _f32c(dP), _f32c(Sm), _f32c(B), _f32c(x)
    E, S, C = Sm.shape
    I = B.shape[2]
    if gB_accum is not None:
        assert gB_accum.shape == (E, S, I) and gB_accum.is_contiguous() and gB_accum.dtype == torch.float32
    gB = gB_accum if gB_accum is not None else torch.empty((E, S, I), device=x.device, dtype=torch.float32)
    if dSm_accum is not None:
        assert dSm_accum.shape == (E, S, C) and dSm_accum.is_contiguous() and dSm_accum.dtype == torch.float32
        assert (S, C, I) == (7, 64, 16), "dSm accumulation exists for the spherical-basis kernel only"
    dSm = dSm_accum if dSm_accum is not None else torch.empty((E, S, C), device=x.device, dtype=torch.float32)
    if dY_accum is not None:
        assert dY_accum.shape == (sp.size, S) and dY_accum.is_contiguous() and dY_accum.dtype == torch.float32
    if not want_dY:
        dY = None
    else:
        dY = dY_accum if dY_accum is not None else torch.empty((sp.size, S), device=x.device, dtype=torch.float32)
    flags = int(dY_accum is not None) | (2 if gB_accum is not None else 0) | (4 if dSm_accum is not None else 0)
    check(_lib.load().gn_bil_project_bwd_acc_f32(ptr(dP), ptr(Sm), ptr(B), ptr(x), ptr(sp.expand.idx32),
                                                 ptr(sp.seg_off), ptr(gB), ptr(dSm), ptr(dY), E, S, C, I,
                                                 flags, stream()),
          "gn_bil_project_bwd_acc_f32")
    return gB, dSm, dY


def bil_fused_bwd_supported(S, C, I, O):
    return (S, C, I, O) == (7, 64, 16, 64)


def bil_fused_bwd(g, W2, Sm, B, alpha=1.0, gB_accum=None, W2_planes=None, up=None):
    """Adjoint of the bilinear tail in one launch -> (gB (E,S,I), dSm (E,S,C)); W2 (I*C, O) = the bilinear weight
    (gn_bil_fused_bwd_f32: dP = alpha g W2^T stays in LDS).  `gB_accum`: running gradient gB is added to (and returned).
    W2_planes: pack_weight_split(W2, fmt=1) — the first product then runs on the fp16 matrix pipe with split operands.
    `up` = dict(planes=pack_weight_split(cat(W_ac^T, W_ca^T), fmt=1), inv=inverse swap (int32), z_ac, z_ca, act, alpha): `g`
    is then the tied gradient G (E,128) of the up-projection pair and the pair's adjoint runs as phase 0 of the launch
    (gn_bil_up_bwd_f32).  Needs W2_planes."""
    require_device(g, W2, Sm, B)
    g, W2, Sm, B = _f32c(g), _f32c(W2), _f32c(Sm), _f32c(B)
    E, S, C = Sm.shape
    I, O = B.shape[2], (g.shape[1] if up is None else W2.shape[1])
    assert tuple(W2.shape) == (I * C, O) and B.shape[:2] == (E, S) and g.shape[0] == E
    if gB_accum is not None:
        assert gB_accum.shape == (E, S, I) and gB_accum.is_contiguous() and gB_accum.dtype == torch.float32
    gB = gB_accum if gB_accum is not None else torch.empty((E, S, I), device=g.device, dtype=torch.float32)
    dSm = torch.empty((E, S, C), device=g.device, dtype=torch.float32)
    if up is not None:
        planes, act, N = up["planes"], bool(up["act"]), UP_PAIR_WIDTH
        if not (USE_K3_F16 and W2_planes is not None and getattr(W2_planes, "_gn_fmt", None) == 1
                and W2_planes.numel() == 64 * 2 * 2 * 64 * 16):
            raise RuntimeError("bil_fused_bwd(up=...): the pair adjoint phase needs the fp16 planes of the bilinear weight")
        assert getattr(planes, "_gn_fmt", None) == 1 and planes.numel() == 4 * 8 * 2 * 64 * 16
        inv, z_ac, z_ca = up["inv"], up["z_ac"], up["z_ca"]
        assert g.shape == (E, N) and inv.dtype == torch.int32 and inv.numel() == E and inv.is_contiguous()
        if act:
            assert all(z.shape == (E, N) and z.is_contiguous() and z.dtype == torch.float32 for z in (z_ac, z_ca))
        check(_lib.load().gn_bil_up_bwd_f32(ptr(g), ptr(inv), ptr(z_ac) if act else None, ptr(z_ca) if act else None,
                                            ptr(planes), ptr(W2_planes), ptr(Sm), ptr(B), ptr(gB), ptr(dSm), E, S, C, I, O, N,
                                            float(alpha), float(up["alpha"]), int(act),
                                            2 if gB_accum is not None else 0, stream()), "gn_bil_up_bwd_f32")
        return gB, dSm
    if W2_planes is not None:
        assert getattr(W2_planes, "_gn_fmt", None) == 1 and W2_planes.numel() == 64 * 2 * 2 * 64 * 16
    check(_lib.load().gn_bil_fused_bwd_f32(ptr(g), ptr(W2), ptr(W2_planes) if USE_K3_F16 else None, ptr(Sm), ptr(B), ptr(gB),
                                           ptr(dSm), E, S, C, I, O, float(alpha),
                                           2 if gB_accum is not None else 0, stream()), "gn_bil_fused_bwd_f32")
    return gB, dSm


def quad_basis_fwd(R, qc, qa, qb, qd, S):
    """-> Y (Q, S^2) = Y_lm(Phi_cab, Theta_cabd) from the 4 atoms of every quadruplet (gemnet.py:334-418)."""
    require_device(R, qc, qa, qb, qd)
    R = _f32c(R)
    Q = qc.shape[0]
    Y = torch.empty((Q, S * S), device=R.device, dtype=torch.float32)
    check(_lib.load().gn_quad_basis_fwd_f32(ptr(R), ptr(qc), ptr(qa), ptr(qb), ptr(qd), ptr(Y), Q, S, stream()),
          "gn_quad_basis_fwd_f32")
    return Y


def quad_basis_bwd(gY, R, qc, qa, qb, qd, S):
    """-> Gc, Gb, Gd (Q,3); dE/dR_a = -(Gc+Gb+Gd)."""
    require_device(gY, R)
    gY, R = _f32c(gY), _f32c(R)
    Q = qc.shape[0]
    Gc, Gb, Gd = (torch.empty((Q, 3), device=R.device, dtype=torch.float32) for _ in range(3))
    check(_lib.load().gn_quad_basis_bwd_f32(ptr(gY), ptr(R), ptr(qc), ptr(qa), ptr(qb), ptr(qd), ptr(Gc), ptr(Gb),
                                            ptr(Gd), Q, S, stream()), "gn_quad_basis_bwd_f32")
    return Gc, Gb, Gd


def quad_basis_bwd_packed(gY, R, qc, qa, qb, qd, S):
    """-> Gc (Q,3) and Gbd (Q,8) = [Gb xyz, 0, Gd xyz, 0] (one float4 segmented sum reduces both)."""
    require_device(gY, R)
    gY, R = _f32c(gY), _f32c(R)
    Q = qc.shape[0]
    Gc = torch.empty((Q, 3), device=R.device, dtype=torch.float32)
    Gbd = torch.zeros((Q, 8), device=R.device, dtype=torch.float32)
    base = addr(Gbd)
    check(_lib.load().gn_quad_basis_bwd_ld_f32(ptr(gY), ptr(R), ptr(qc), ptr(qa), ptr(qb), ptr(qd), ptr(Gc), 3,
                                               base, 8, base + 16, 8, Q, S, stream()), "gn_quad_basis_bwd_ld_f32")
    return Gc, Gbd
