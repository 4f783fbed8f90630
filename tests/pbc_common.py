"""Periodic test infrastructure (numpy / fp64 oracle): a brute-force image neighbour list in the canonical order of
csrc/pbc.hip (include/gemnet_hip.h), and the cluster oracle — the periodic energy of GemNet-T as the energy of the central
cell's atoms inside a finite cluster of their images, evaluated by the molecular fp64 oracle."""
import itertools

import numpy as np
import torch

from oracle import gemnet_oracle as GO
from oracle import index_oracle as IO

# a small GemNet-T (receptive field ~ (num_blocks + 1) cutoff) so that the clusters stay small
CFG = dict(num_spherical=7, num_radial=6, num_blocks=1, emb_size_atom=16, emb_size_edge=16, emb_size_trip=8, emb_size_quad=8,
           emb_size_rbf=8, emb_size_cbf=8, emb_size_sbf=8, emb_size_bil_quad=8, emb_size_bil_trip=8, num_before_skip=1,
           num_after_skip=1, num_concat=1, num_atom=1, triplets_only=True, cutoff=2.6)
CUTOFF = 2.6
RADIUS = 3 * CUTOFF + 0.5        # cluster radius: above the receptive field of CFG


def heights(cell):
    cell = np.asarray(cell, np.float64)
    vol = abs(np.linalg.det(cell))
    return np.array([vol / np.linalg.norm(np.cross(cell[(k + 1) % 3], cell[(k + 2) % 3])) for k in range(3)])


def _image_grid(R, cell, pbc, radius):
    f = np.asarray(R, np.float64) @ np.linalg.inv(np.asarray(cell, np.float64))
    span = f.max(0) - f.min(0) if len(f) else np.zeros(3)
    ext = np.where(pbc, np.ceil(radius / heights(cell)) + np.ceil(span) + 1, 0).astype(int)
    return list(itertools.product(*[range(-e, e + 1) for e in ext]))


def brute_force(R, N, cell, pbc, cutoff):
    """-> dict of int64 arrays (GemNet-T keys + cell_offsets) in canonical order (fp64 distances)."""
    R = np.asarray(R, np.float64)
    cell = np.asarray(cell, np.float64).reshape(-1, 3, 3)
    pbc = np.broadcast_to(np.asarray(pbc, bool).reshape(-1, 3), (len(N), 3))
    fwd = []
    off = 0
    for b, n in enumerate(N):
        Rm = R[off:off + n]
        imgs = np.array(_image_grid(Rm, cell[b], pbc[b], cutoff), dtype=np.int64)     # lexicographic n0, n1, n2
        shifts = imgs @ cell[b]
        for i in range(n):
            for j in range(i, n):
                d = np.linalg.norm(Rm[i] - (Rm[j] + shifts), axis=1)
                for k in np.nonzero(d <= cutoff)[0]:
                    nn = imgs[k]
                    if j == i and not tuple(nn) > (0, 0, 0):
                        continue
                    fwd.append((off + i, off + j, *nn))
        off += n
    fwd = np.array(fwd, dtype=np.int64).reshape(-1, 5)
    H = len(fwd)
    out = {"batch_seg": np.repeat(np.arange(len(N)), N).astype(np.int64)}
    out["id_a"] = np.concatenate([fwd[:, 0], fwd[:, 1]])
    out["id_c"] = np.concatenate([fwd[:, 1], fwd[:, 0]])
    out["cell_offsets"] = np.concatenate([fwd[:, 2:], -fwd[:, 2:]])
    ind = np.arange(H, dtype=np.int64)
    out["id_undir"] = np.concatenate([ind, ind])
    out["id_swap"] = np.concatenate([ind + H, ind])
    E = 2 * H
    red, exp = [], []
    for r in range(E):
        x = np.nonzero(out["id_a"] == out["id_a"][r])[0]
        x = x[x != r]
        red.append(np.full(len(x), r, np.int64))
        exp.append(x)
    out["id3_reduce_ca"] = np.concatenate(red) if red else np.zeros(0, np.int64)
    out["id3_expand_ba"] = np.concatenate(exp) if exp else np.zeros(0, np.int64)
    out["Kidx3"] = IO._kidx(out["id3_reduce_ca"])
    return out


def edge_set(idx):
    return {(int(c), int(a), *map(int, o)) for c, a, o in zip(idx["id_c"], idx["id_a"], idx["cell_offsets"])}


def triplet_set(idx):
    """Triplets as ((c, a, n_c), (b, a, n_b)) edge pairs."""
    key = lambda e: (int(idx["id_c"][e]), int(idx["id_a"][e]), *map(int, idx["cell_offsets"][e]))
    return {(key(r), key(x)) for r, x in zip(idx["id3_reduce_ca"], idx["id3_expand_ba"])}


def cluster(R, Z, cell, pbc, radius):
    """Central atoms first, then every image (n != 0) within `radius` of a central atom."""
    R = np.asarray(R, np.float64)
    cell = np.asarray(cell, np.float64)
    Rs, Zs = [R], [np.asarray(Z)]
    for n in _image_grid(R, cell, pbc, radius):
        if n == (0, 0, 0):
            continue
        Ri = R + np.array(n, np.float64) @ cell
        d = np.linalg.norm(Ri[:, None, :] - R[None, :, :], axis=-1).min(1)
        keep = d <= radius
        Rs.append(Ri[keep])
        Zs.append(np.asarray(Z)[keep])
    return np.concatenate(Rs), np.concatenate(Zs)


def cluster_energy(params, R, Z, cell, pbc, radius=RADIUS, cfg=CFG):
    """Periodic energy of one structure (fp64): E[0] of the cluster with the central atoms as molecule 0, the ghosts as 1."""
    Rc, Zc = cluster(R, Z, cell, pbc, radius)
    n = len(R)
    idx = IO.build_indices(Rc, np.array([len(Rc)]), cfg["cutoff"], 10.0, True)
    inputs = {k: torch.tensor(v) for k, v in idx.items()}
    bs = np.zeros(len(Rc), np.int64)
    bs[n:] = 1
    inputs.update(Z=torch.tensor(Zc).long(), R=torch.tensor(Rc), batch_seg=torch.tensor(bs), N=torch.tensor([n, len(Rc) - n]))
    E, _ = GO.forward(cfg, params, inputs, need_forces=False)
    return float(E[0, 0])


def fd_forces_stress(params, R, Z, cell, pbc, h=1e-4, radius=RADIUS, richardson=False):
    """Central differences of the cluster energy: F (moving all images of an atom together) and the stress dE/d(strain)/|det|
    (straining cell and positions together).  `richardson` (opt-in; the default is what every stored golden was made with):
    (4 fd(h) - fd(2h)) / 3, which removes the h^2 term — on cells with image distances below 1 A (`skewed`: 0.93 A) the plain
    h = 1e-4 differences are ~1e-6 relative off, the extrapolated ones ~1e-10 (tests/test_pbc_train_cells_cpu.py)."""
    if richardson:
        F1, S1 = fd_forces_stress(params, R, Z, cell, pbc, h, radius)
        F2, S2 = fd_forces_stress(params, R, Z, cell, pbc, 2 * h, radius)
        return (4 * F1 - F2) / 3, (4 * S1 - S2) / 3
    R = np.asarray(R, np.float64)
    cell = np.asarray(cell, np.float64)
    F = np.zeros_like(R)
    for i in range(len(R)):
        for k in range(3):
            Rp, Rm = R.copy(), R.copy()
            Rp[i, k] += h
            Rm[i, k] -= h
            F[i, k] = -(cluster_energy(params, Rp, Z, cell, pbc, radius) - cluster_energy(params, Rm, Z, cell, pbc, radius)) / (2 * h)
    S = np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            eps = np.zeros((3, 3))
            eps[a, b] = h
            Ep = cluster_energy(params, R @ (np.eye(3) + eps), Z, cell @ (np.eye(3) + eps), pbc, radius)
            Em = cluster_energy(params, R @ (np.eye(3) - eps), Z, cell @ (np.eye(3) - eps), pbc, radius)
            S[a, b] = (Ep - Em) / (2 * h)
    return F, S / abs(np.linalg.det(cell))


def make_params(seed=3):
    import os
    from conftest import ROOT
    scale = GO.load_scale_factors(os.path.join(ROOT, "gemnet_pytorch_amd", "scaling_factors.json"))
    return GO.make_params(CFG, seed, scale)


PBC_VARIANTS = {"TFF": (True, False, False), "FTT": (False, True, True), "FFF": (False, False, False)}
# kinds whose cells are small, thin, sheared or left-handed (image ranges beyond |n| = 1, self-image edges, exactly collinear
# triplets), and 'triclinic' under the mixed / open boundary conditions of PBC_VARIANTS
NEW_KINDS = ["bcc", "bcc_pert", "thin", "skewed", "skewed_lh", "triclinic_TFF", "triclinic_FTT", "triclinic_FFF"]
OLD_KINDS = ["cubic1", "small", "triclinic", "slab"]
_TRICLINIC_F = np.array([[0.1, 0.1, 0.1], [0.5, 0.45, 0.55], [0.8, 0.2, 0.6]])


def structure(kind, seed=0):
    """(R, Z, cell, pbc) of small test structures.  kind: 'cubic1' (one atom), 'small' (cubic, 3 atoms), 'triclinic',
    'slab' (T, T, F); 'bcc' (a = 2.5: every lattice vector below the cutoff, self-image edges, collinear triplets), 'bcc_pert'
    (bcc moved off its symmetric positions), 'thin' (one height below cutoff / 2: images up to |n| = 2), 'skewed' (strongly
    sheared: heights 0.78 / 1.94 / 3.3 under vectors of 3.0 / 6.66 / 5.92, images up to |n| = 3), 'skewed_lh' (the same with
    rows 0 and 1 swapped: det < 0), 'triclinic_<TFF|FTT|FFF>' (the triclinic cell with those periodic axes)."""
    rs = np.random.RandomState(seed)
    all_t = np.array([True, True, True])
    if kind == "cubic1":
        return np.zeros((1, 3)), np.array([6]), np.eye(3) * 2.1, all_t
    if kind == "small":
        cell = np.eye(3) * 3.3
        R = np.array([[0.2, 0.3, 0.1], [1.4, 1.1, 0.9], [2.5, 2.2, 2.6]])
        return R + rs.uniform(-0.1, 0.1, R.shape), np.array([1, 6, 8]), cell, all_t
    if kind == "triclinic" or (kind.startswith("triclinic_") and kind[10:] in PBC_VARIANTS):
        cell = np.array([[3.4, 0.0, 0.0], [1.1, 3.2, 0.0], [0.6, 0.9, 3.5]])
        f = _TRICLINIC_F + rs.uniform(-0.03, 0.03, (3, 3))
        return f @ cell, np.array([8, 1, 6]), cell, np.array(PBC_VARIANTS[kind[10:]]) if kind != "triclinic" else all_t
    if kind == "slab":
        cell = np.array([[3.2, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, 0.0, 12.0]])
        R = np.array([[0.3, 0.2, 5.0], [1.7, 1.5, 5.8], [0.9, 2.2, 6.9]]) + rs.uniform(-0.1, 0.1, (3, 3))
        return R, np.array([6, 8, 1]), cell, np.array([True, True, False])
    if kind in ("bcc", "bcc_pert"):
        a = 2.5
        R = np.array([[0.0, 0.0, 0.0], [a / 2, a / 2, a / 2]])
        if kind == "bcc_pert":
            R = R + rs.uniform(-0.08, 0.08, R.shape)
        return R, np.array([6, 8]), np.eye(3) * a, all_t
    if kind == "thin":
        return np.array([[0.1, 0.2, 0.3], [0.7, 1.9, 2.0]]), np.array([8, 6]), np.diag([1.2, 3.4, 3.6]), all_t
    if kind in ("skewed", "skewed_lh"):
        cell = np.array([[3.0, 0.0, 0.0], [5.9, 3.1, 0.0], [-2.7, 4.1, 3.3]])
        if kind == "skewed_lh":
            cell = cell[[1, 0, 2]]
        return _TRICLINIC_F @ cell, np.array([8, 1, 6]), cell, all_t
    raise ValueError(kind)


# ------------------------------------------------------------------------------------- sizes beyond one wavefront / 1024 rows
def brute_force_fast(R, N, cell, pbc, cutoff):
    """`brute_force` (same dict, same canonical order, same fp64 distances) with the loops over partners, images and triplets
    vectorised: one numpy pass per atom.  tests/test_pbc_cpu.py holds it to the slow builder array for array."""
    R = np.asarray(R, np.float64)
    cell = np.asarray(cell, np.float64).reshape(-1, 3, 3)
    pbc = np.broadcast_to(np.asarray(pbc, bool).reshape(-1, 3), (len(N), 3))
    fwd = []
    off = 0
    for b, n in enumerate(N):
        Rm = R[off:off + n]
        imgs = np.array(_image_grid(Rm, cell[b], pbc[b], cutoff), dtype=np.int64)     # lexicographic n0, n1, n2
        shifts = imgs @ cell[b]
        # an image further from the origin than the structure's extent + cutoff (per Cartesian axis) holds no partner
        reach = (Rm.max(0) - Rm.min(0) if n else np.zeros(3)) + cutoff + 1e-6
        near = (np.abs(shifts) <= reach).all(1)
        imgs, shifts = imgs[near], shifts[near]
        lexpos = np.array([tuple(nn) > (0, 0, 0) for nn in imgs.tolist()], dtype=bool)
        for i in range(n):
            d = np.linalg.norm(Rm[i] - (Rm[i:, None, :] + shifts[None, :, :]), axis=-1)      # (partners j >= i, images)
            hit = d <= cutoff
            hit[0] &= lexpos
            j, k = np.nonzero(hit)                                                        # row-major: ascending (j, n)
            fwd.append(np.column_stack([np.full(len(j), off + i), off + i + j, imgs[k]]))
        off += n
    fwd = np.concatenate(fwd).astype(np.int64).reshape(-1, 5) if fwd else np.zeros((0, 5), np.int64)
    H = len(fwd)
    out = {"batch_seg": np.repeat(np.arange(len(N)), N).astype(np.int64)}
    out["id_a"] = np.concatenate([fwd[:, 0], fwd[:, 1]])
    out["id_c"] = np.concatenate([fwd[:, 1], fwd[:, 0]])
    out["cell_offsets"] = np.concatenate([fwd[:, 2:], -fwd[:, 2:]])
    ind = np.arange(H, dtype=np.int64)
    out["id_undir"] = np.concatenate([ind, ind])
    out["id_swap"] = np.concatenate([ind + H, ind])
    # triplets: every ordered pair (r, x != r) of edges into the same atom, by (r, x)
    E = 2 * H
    order = np.argsort(out["id_a"], kind="stable")               # edges grouped by target atom, ascending id inside a group
    deg = np.bincount(out["id_a"], minlength=len(R))[out["id_a"]] if E else np.zeros(0, np.int64)
    start = np.concatenate([[0], np.cumsum(np.bincount(out["id_a"], minlength=len(R)))])
    red = np.repeat(np.arange(E, dtype=np.int64), deg)
    within = np.arange(len(red), dtype=np.int64) - np.repeat(np.cumsum(deg) - deg, deg)
    exp = order[start[out["id_a"][red]] + within] if E else np.zeros(0, np.int64)
    keep = exp != red
    out["id3_reduce_ca"], out["id3_expand_ba"] = red[keep], exp[keep].astype(np.int64)
    out["Kidx3"] = IO._kidx(out["id3_reduce_ca"])
    return out


def arrays(structs):
    """-> R (A,3), Z (A,), N list, cell (B,3,3), pbc (B,3) of a list of structures."""
    return (np.concatenate([s[0] for s in structs]), np.concatenate([s[1] for s in structs]), [len(s[0]) for s in structs],
            np.stack([s[2] for s in structs]), np.stack([s[3] for s in structs]))


def f32_round(s):
    """The structure with positions and cell rounded through float32 (what a float32 builder sees, held in float64)."""
    R, Z, cell, pbc = s
    return np.asarray(R, np.float32).astype(np.float64), Z, np.asarray(cell, np.float32).astype(np.float64), pbc


def cutoff_margin_ok(R, N, cell, pbc, cutoff=CUTOFF, margin=1e-5):
    """No pair within `margin` of the cutoff: float32 and float64 distances then give the same list."""
    ref = brute_force_fast(R, N, cell, pbc, cutoff)
    return all(all(np.array_equal(ref[k], o[k]) for k in ref)
               for o in (brute_force_fast(R, N, cell, pbc, cutoff + d) for d in (-margin, margin)))


def gas():
    """1100 atoms of a random gas in a cubic 30 A cell, all periodic (float32-rounded): 3324 edges, 10 044 triplets — more atoms
    than one scan round (1024), more edges and triplets than several."""
    R = np.random.RandomState(0).uniform(0, 30.0, (1100, 3)).astype(np.float32).astype(np.float64)
    return R, np.tile(np.array([1, 6, 7, 8]), 275), np.eye(3) * 30.0, np.array([True, True, True])


def _gas_structure(n, rs, pbc, density=0.06, dmin=0.9):
    """n atoms at random in a cubic cell of n / density A^3, no two atoms (or images) closer than dmin."""
    L = (n / density) ** (1.0 / 3.0)
    imgs = np.array(list(itertools.product((-1, 0, 1), repeat=3)), np.float64) * L
    R = np.zeros((0, 3))
    while len(R) < n:
        x = rs.uniform(0, L, 3)
        if len(R) == 0 or np.linalg.norm(x - (R[:, None, :] + imgs[None]), axis=-1).min() >= dmin:
            R = np.concatenate([R, x[None]])
    return R, rs.choice([1, 6, 7, 8], n), np.eye(3) * L, np.array(pbc)


def isolated(n_structs=1):
    """Single atoms in 30 A cells: no edge at all."""
    return [(np.full((1, 3), 3.0 + b), np.array([6]), np.eye(3) * 30.0, np.array([True, True, True])) for b in range(n_structs)]


ZOO_GAS = [1, 2, 63, 64, 65, 130, 127, 128, 129, 66, 100, 31, 33, 5, 97, 7, 17, 11, 3, 45]
_ZOO_PBC = [(True, True, True), (True, True, False), (True, True, True), (False, True, True), (True, False, True),
            (True, True, True), (True, False, False), (False, False, False)]


def zoo():
    """One batch of 46 structures / 1090 atoms (float32-rounded): every small kind, random-gas structures of ZOO_GAS atoms
    (1, 2 and 63 / 64 / 65 / ~130 straddle the 64-lane partner loop of pbc_index.hip) under mixed periodic axes, a single atom
    without edges in the middle and one at the very end, and the small kinds again behind atom 1024 (the second scan round)."""
    rs = np.random.RandomState(5)
    kinds = OLD_KINDS + NEW_KINDS
    structs = [structure(k, seed=i) for i, k in enumerate(kinds)]
    for q, n in enumerate(ZOO_GAS):
        if q == 9:
            structs += isolated(1)
        structs.append(_gas_structure(n, rs, (True, True, True) if n <= 2 else _ZOO_PBC[q % len(_ZOO_PBC)]))
    assert sum(len(s[0]) for s in structs) > 1024
    structs += [structure(k, seed=20 + i) for i, k in enumerate(kinds)]
    structs += isolated(1)
    return [f32_round(s) for s in structs]


# ----------------------------------------------------------------------------------------------- image boxes (pbc.hip image_range)
def image_box(Ri, Rj, cell, pbc, cutoff=CUTOFF):
    """(lo, hi) per axis of the image range of the pair (i, j): `image_range` of csrc/pbc.hip restated — cofactors, signed
    determinant in the fractional difference, |det| in cutoff / height."""
    c = np.asarray(cell, np.float64)
    cof = np.array([np.cross(c[(k + 1) % 3], c[(k + 2) % 3]) for k in range(3)])
    det = float(c[0] @ cof[0])
    d0 = np.asarray(Rj, np.float64) - np.asarray(Ri, np.float64)
    lo, hi = np.zeros(3, int), np.zeros(3, int)
    for k in range(3):
        if not pbc[k]:
            continue
        f = float(d0 @ cof[k]) / det
        w = cutoff * np.linalg.norm(cof[k]) / abs(det)
        lo[k], hi[k] = int(np.floor(-f - w)), int(np.ceil(-f + w))
    return lo, hi
