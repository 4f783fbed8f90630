"""Periodic GemNet-Q test infrastructure (numpy): a brute-force image-aware quadruplet index build in the canonical order of
csrc/pbc_index_q.hip (include/gemnet_hip.h, gn_pbc_qindex_*) on top of the edge list of tests/pbc_common.py.

The reference's get_quadruplets (data_container.py:428-489) with every node identified by (atom, image): for a quadruplet
c -> a - b <- d, a sits in image 0, c in n_c = cell_offsets[ca], b in n_b = int_cell_offsets[ab], d in n_b + cell_offsets[db]."""
import numpy as np

import pbc_common as P
from oracle import index_oracle as IO

CUTOFF = P.CUTOFF
INT_CUTOFF = 3.0
KEYS_Q = IO.INDEX_KEYS_Q + ["int_cell_offsets"]


# ---- the fp64 cluster oracle with quadruplets --------------------------------------------------------------------------
# P.CFG with triplets_only=False and a short int_cutoff; CFG_ANG has the widths at which the model takes the angle form of the
# tensor basis (emb_size_quad = emb_size_sbf = 32)
CFG_Q = dict(P.CFG, triplets_only=False, int_cutoff=INT_CUTOFF)
CFG_ANG = dict(CFG_Q, emb_size_quad=32, emb_size_sbf=32)
CFGS = {"q": CFG_Q, "ang": CFG_ANG}
# receptive field of one block: the updated edge c -> a reaches d over a - b <- d (2 cutoff + int_cutoff from a), and the
# swapped-edge path adds one cutoff
RADIUS = 3 * CUTOFF + INT_CUTOFF + 0.5
GOLDEN_CASES = {"q": ("small", "triclinic", "slab", "bcc_pert", "thin"), "ang": ("small", "triclinic")}
FD_H = 1e-4


def make_params(cfg, seed=3):
    import os
    from conftest import ROOT
    from oracle import gemnet_oracle as GO
    return GO.make_params(cfg, seed, GO.load_scale_factors(os.path.join(ROOT, "gemnet_pytorch_amd", "scaling_factors.json")))


def cluster_energy(params, R, Z, cell, pbc, cfg, radius=RADIUS):
    """`pbc_common.cluster_energy` for a quadruplet model: E[0] of the finite cluster (central atoms = molecule 0) under the
    molecular fp64 oracle with the index arrays of `cfg` (cutoff, int_cutoff, triplets_only=False)."""
    import torch
    from oracle import gemnet_oracle as GO
    Rc, Zc = P.cluster(R, Z, cell, pbc, radius)
    n = len(R)
    idx = IO.build_indices(Rc, np.array([len(Rc)]), cfg["cutoff"], cfg["int_cutoff"], False)
    inputs = {k: torch.tensor(v) for k, v in idx.items()}
    bs = np.zeros(len(Rc), np.int64)
    bs[n:] = 1
    inputs.update(Z=torch.tensor(Zc).long(), R=torch.tensor(Rc), batch_seg=torch.tensor(bs), N=torch.tensor([n, len(Rc) - n]))
    E, _ = GO.forward(cfg, params, inputs, need_forces=False)
    return float(E[0, 0])


def fd_force(params, R, Z, cell, pbc, cfg, i, k, h=FD_H):
    Rp, Rm = np.array(R, np.float64), np.array(R, np.float64)
    Rp[i, k] += h
    Rm[i, k] -= h
    return -(cluster_energy(params, Rp, Z, cell, pbc, cfg) - cluster_energy(params, Rm, Z, cell, pbc, cfg)) / (2 * h)


def fd_stress(params, R, Z, cell, pbc, cfg, a, b, h=FD_H):
    eps = np.zeros((3, 3))
    eps[a, b] = h
    R, cell = np.asarray(R, np.float64), np.asarray(cell, np.float64)
    Ep = cluster_energy(params, R @ (np.eye(3) + eps), Z, cell @ (np.eye(3) + eps), pbc, cfg)
    Em = cluster_energy(params, R @ (np.eye(3) - eps), Z, cell @ (np.eye(3) - eps), pbc, cfg)
    return (Ep - Em) / (2 * h) / abs(np.linalg.det(cell))


def fd_forces_stress(params, R, Z, cell, pbc, cfg, h=FD_H):
    """The recipe of `pbc_common.fd_forces_stress` (central differences, all images of an atom moved together; cell and
    positions strained together) on the quadruplet cluster oracle."""
    F = np.array([[fd_force(params, R, Z, cell, pbc, cfg, i, k, h) for k in range(3)] for i in range(len(R))])
    S = np.array([[fd_stress(params, R, Z, cell, pbc, cfg, a, b, h) for b in range(3)] for a in range(3)])
    return F, S


def _lex_positive(n):
    return tuple(int(v) for v in n) > (0, 0, 0)


def interaction_edges(R, N, cell, pbc, int_cutoff):
    """-> int_a, int_b (n_int,), offsets (n_int,3): every (b -> a, n) with |R_a - (R_b + n cell)| <= int_cutoff except
    (b == a, n == 0), ordered by (a, b, n lexicographic).  The distance of a pair is evaluated on its canonical forward form
    (a < b, or a == b and n lexicographically positive) and mirrored, like the edge list."""
    R = np.asarray(R, np.float64)
    rows = []
    off = 0
    for b_, n in enumerate(N):
        Rm = R[off:off + n]
        imgs = np.array(P._image_grid(Rm, cell[b_], pbc[b_], int_cutoff), dtype=np.int64)
        shifts = imgs @ cell[b_]
        lexpos = np.array([_lex_positive(nn) for nn in imgs], dtype=bool)
        for i in range(n):
            for j in range(i, n):
                hit = np.linalg.norm(Rm[i] - (Rm[j] + shifts), axis=1) <= int_cutoff
                if j == i:
                    hit &= lexpos
                for nn in imgs[hit]:
                    rows.append((off + i, off + j, *nn))
                    rows.append((off + j, off + i, *(-nn)))
        off += n
    rows = np.array(sorted(rows), dtype=np.int64).reshape(-1, 5)
    return rows[:, 0], rows[:, 1], rows[:, 2:]


def brute_force_q(R, N, cell, pbc, cutoff=CUTOFF, int_cutoff=INT_CUTOFF):
    """-> dict of int64 arrays: the GemNet-T keys + cell_offsets of `pbc_common.brute_force_fast`, the reference's quadruplet
    keys and int_cell_offsets, in canonical order (fp64 distances)."""
    R = np.asarray(R, np.float64)
    cell = np.asarray(cell, np.float64).reshape(-1, 3, 3)
    pbc = np.broadcast_to(np.asarray(pbc, bool).reshape(-1, 3), (len(N), 3))
    out = P.brute_force_fast(R, N, cell, pbc, cutoff)
    id_a, id_c, offs = out["id_a"], out["id_c"], out["cell_offsets"].reshape(-1, 3)
    A = len(R)
    int_a, int_b, int_offs = interaction_edges(R, N, cell, pbc, int_cutoff)
    out["id4_int_a"], out["id4_int_b"], out["int_cell_offsets"] = int_a, int_b, int_offs
    # incoming edges per atom, ordered by (source atom, cell offset lexicographic)
    order_in = np.lexsort((offs[:, 2], offs[:, 1], offs[:, 0], id_c, id_a)) if len(id_a) else np.zeros(0, np.int64)
    in_ptr = np.concatenate([[0], np.cumsum(np.bincount(id_a, minlength=A))]).astype(np.int64)
    in_edges = lambda atom: order_in[in_ptr[atom]:in_ptr[atom + 1]]
    e = np.zeros(0, np.int64)
    nN_t = in_ptr[int_a + 1] - in_ptr[int_a]
    nN_s = in_ptr[int_b + 1] - in_ptr[int_b]
    red_intm_ca = np.concatenate([in_edges(a) for a in int_a] + [e]).astype(np.int64)
    exp_intm_db = np.concatenate([in_edges(b) for b in int_b] + [e]).astype(np.int64)
    out["id4_reduce_intm_ca"], out["id4_expand_intm_db"] = red_intm_ca, exp_intm_db
    out["id4_reduce_intm_ab"] = np.repeat(np.arange(len(int_a), dtype=np.int64), nN_t)
    out["id4_expand_intm_ab"] = np.repeat(np.arange(len(int_a), dtype=np.int64), nN_s)
    # the cross product of the two lists per interaction edge (data_container.py:446-462)
    reduce_cab = IO.repeat_blocks(nN_t, nN_s)
    expand_abd = np.repeat(np.arange(len(exp_intm_db), dtype=np.int64), np.repeat(nN_t, nN_s))
    reduce_ca = red_intm_ca[reduce_cab] if len(reduce_cab) else e
    expand_db = exp_intm_db[expand_abd] if len(expand_abd) else e
    k = out["id4_reduce_intm_ab"][reduce_cab] if len(reduce_cab) else e
    # nodes as (atom, image): a in 0, c in n_c, b in n_b, d in n_b + n_db
    c, a, b, d = id_c[reduce_ca], id_a[reduce_ca], id_a[expand_db], id_c[expand_db]
    n_c, n_b = offs[reduce_ca], int_offs[k]
    n_d = n_b + offs[expand_db]
    same = lambda x, nx, y, ny: (x == y) & (nx == ny).all(axis=1)
    keep = ~same(c, n_c, b, n_b) & ~same(a, np.zeros_like(n_d), d, n_d) & ~same(c, n_c, d, n_d)
    reduce_ca, expand_db, reduce_cab, expand_abd, k = (v[keep] for v in (reduce_ca, expand_db, reduce_cab, expand_abd, k))
    o = np.lexsort((k, expand_db, reduce_ca))
    out["id4_reduce_ca"], out["id4_expand_db"] = reduce_ca[o], expand_db[o]
    out["id4_reduce_cab"], out["id4_expand_abd"] = reduce_cab[o], expand_abd[o]
    out["Kidx4"] = IO._kidx(out["id4_reduce_ca"])
    return out


def cutoff_margins_ok(R, N, cell, pbc, cutoff=CUTOFF, int_cutoff=INT_CUTOFF, margin=1e-5):
    """No pair within `margin` of either cutoff (`pbc_common.cutoff_margin_ok` for both radii): float32 and float64 distances
    then give the same arrays."""
    if not P.cutoff_margin_ok(R, N, cell, pbc, cutoff, margin):
        return False
    pbc = np.broadcast_to(np.asarray(pbc, bool).reshape(-1, 3), (len(N), 3))
    cell = np.asarray(cell, np.float64).reshape(-1, 3, 3)
    ref = interaction_edges(R, N, cell, pbc, int_cutoff)
    return all(all(np.array_equal(x, y) for x, y in zip(ref, interaction_edges(R, N, cell, pbc, int_cutoff + d)))
               for d in (-margin, margin))


def quad_nodes(idx):
    """The four (atom, n0, n1, n2) nodes c, a, b, d of every quadruplet, read through the index arrays, as (Q,4) arrays."""
    id_a, id_c, offs = idx["id_a"], idx["id_c"], idx["cell_offsets"].reshape(-1, 3)
    ca, db = idx["id4_reduce_ca"], idx["id4_expand_db"]
    k = idx["id4_reduce_intm_ab"][idx["id4_reduce_cab"]]
    n_b = idx["int_cell_offsets"].reshape(-1, 3)[k]
    node = lambda atom, n: np.column_stack([atom, n])
    return (node(id_c[ca], offs[ca]), node(id_a[ca], np.zeros_like(n_b)), node(id_a[db], n_b), node(id_c[db], n_b + offs[db]))


def check_invariants(idx):
    """What must hold for any periodic quadruplet index dict (all keys int arrays)."""
    id_a, id_c = idx["id_a"], idx["id_c"]
    int_a, int_b, int_offs = idx["id4_int_a"], idx["id4_int_b"], idx["int_cell_offsets"].reshape(-1, 3)
    # interaction edges: sorted by (a, b, n), no (a, a, 0), both directions
    rows = [(int(a), int(b), *map(int, n)) for a, b, n in zip(int_a, int_b, int_offs)]
    assert rows == sorted(rows) and len(set(rows)) == len(rows)
    assert all(not (r[0] == r[1] and r[2:] == (0, 0, 0)) for r in rows)
    assert {(b, a, -n0, -n1, -n2) for a, b, n0, n1, n2 in rows} == set(rows)
    # intermediate triplets: id_a agrees across the index families (data_container.py:398-405)
    ica, idb = idx["id4_reduce_intm_ca"], idx["id4_expand_intm_db"]
    iab_r, iab_e = idx["id4_reduce_intm_ab"], idx["id4_expand_intm_ab"]
    assert np.array_equal(id_a[ica], int_a[iab_r]) and np.array_equal(id_a[idb], int_b[iab_e])
    ca, db, cab, abd = (idx[k] for k in ("id4_reduce_ca", "id4_expand_db", "id4_reduce_cab", "id4_expand_abd"))
    assert np.array_equal(ica[cab], ca) and np.array_equal(idb[abd], db)
    assert np.array_equal(iab_r[cab], iab_e[abd])                       # both halves hang on the same interaction edge
    k = iab_r[cab]
    assert np.array_equal(id_a[ca], int_a[k]) and np.array_equal(id_a[db], int_b[k])
    assert np.array_equal(id_c[ca], id_c[ica][cab]) and np.array_equal(id_c[db], id_c[idb][abd])
    # the four nodes: c != b, a != d, c != d as (atom, image); a != c and b != d hold by the edge list
    c, a, b, d = quad_nodes(idx)
    differ = lambda x, y: (x != y).any(axis=1)
    assert differ(c, b).all() and differ(a, d).all() and differ(c, d).all() and differ(a, c).all() and differ(b, d).all()
    # order: (reduce edge, expand edge, interaction edge), no row twice; Kidx4 the position inside a reduce segment
    key = np.column_stack([ca, db, k])
    assert np.array_equal(np.lexsort((k, db, ca)), np.arange(len(ca))) and len(np.unique(key, axis=0)) == len(key)
    assert np.array_equal(idx["Kidx4"], IO._kidx(ca))
