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


def fd_forces_stress(params, R, Z, cell, pbc, h=1e-4, radius=RADIUS):
    """Central differences of the cluster energy: F (moving all images of an atom together) and the stress dE/d(strain)/|det|
    (straining cell and positions together)."""
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


def structure(kind, seed=0):
    """(R, Z, cell, pbc) of small test structures.  kind: 'cubic1' (one atom), 'small' (cubic, 3 atoms), 'triclinic',
    'slab' (T, T, F)."""
    rs = np.random.RandomState(seed)
    if kind == "cubic1":
        return np.zeros((1, 3)), np.array([6]), np.eye(3) * 2.1, np.array([True, True, True])
    if kind == "small":
        cell = np.eye(3) * 3.3
        R = np.array([[0.2, 0.3, 0.1], [1.4, 1.1, 0.9], [2.5, 2.2, 2.6]])
        return R + rs.uniform(-0.1, 0.1, R.shape), np.array([1, 6, 8]), cell, np.array([True, True, True])
    if kind == "triclinic":
        cell = np.array([[3.4, 0.0, 0.0], [1.1, 3.2, 0.0], [0.6, 0.9, 3.5]])
        f = np.array([[0.1, 0.1, 0.1], [0.5, 0.45, 0.55], [0.8, 0.2, 0.6]]) + rs.uniform(-0.03, 0.03, (3, 3))
        return f @ cell, np.array([8, 1, 6]), cell, np.array([True, True, True])
    if kind == "slab":
        cell = np.array([[3.2, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, 0.0, 12.0]])
        R = np.array([[0.3, 0.2, 5.0], [1.7, 1.5, 5.8], [0.9, 2.2, 6.9]]) + rs.uniform(-0.1, 0.1, (3, 3))
        return R, np.array([6, 8, 1]), cell, np.array([True, True, False])
    raise ValueError(kind)
