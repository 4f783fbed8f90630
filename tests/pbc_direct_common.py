"""Helpers of the periodic direct-force tests: an fp64 restatement of the force head (csrc/direct_force.hip), the literal
reference formulation it replaces, the derived error bound of the kernel test, two one-atom cells whose single atom has more
in-edges than one / two wavefronts, and the cluster oracle (tests/pbc_common.py) for a direct-force model."""
import functools

import numpy as np
import torch

import pbc_common as P
from oracle import gemnet_oracle as GO
from oracle import index_oracle as IO

DEV = "cuda"


# ------------------------------------------------------------------------------------------------ the force head in fp64
def direct_force_ref(terms, V, id_swap, id_a, n_atoms):
    """F (A,T,3) float64 of gn_direct_force_f32: terms (K,E,T), V (E,3) not normalised, id_swap (E) or None, id_a (E)."""
    terms, V = np.asarray(terms, np.float64), np.asarray(V, np.float64)
    c = terms.sum(0)
    if id_swap is not None:
        c = 0.5 * (c + c[np.asarray(id_swap)])
    u = V / np.linalg.norm(V, axis=1)[:, None]
    F = np.zeros((n_atoms, terms.shape[2], 3))
    np.add.at(F, np.asarray(id_a), c[:, :, None] * u[:, None, :])
    return F


def literal_ref(terms, V, id_undir, id_a, n_atoms):
    """The reference formulation (gemnet.py:586-596) in fp64: pairwise sum of the blocks' terms, scatter-mean over id_undir +
    gather when `id_undir` is given, product with the unit vectors, scatter-add over id_a."""
    terms, V = np.asarray(terms, np.float64), np.asarray(V, np.float64)
    F_ca = terms[0]
    for k in range(1, terms.shape[0]):
        F_ca = F_ca + terms[k]
    if id_undir is not None:
        id_undir = np.asarray(id_undir)
        half = np.zeros((len(id_undir) // 2, terms.shape[2]))
        np.add.at(half, id_undir, F_ca)
        F_ca = (half / 2.0)[id_undir]
    D = np.sqrt((V ** 2).sum(1))
    F_ji = F_ca[:, :, None] * (V / D[:, None])[:, None, :]
    F = np.zeros((n_atoms, terms.shape[2], 3))
    np.add.at(F, np.asarray(id_a), F_ji)
    return F


def error_bound(terms, id_swap, id_a, n_atoms):
    """(A,T) bound of |F - F_ref| per component of the fp32 kernel: (n_a + 2 K + 8) 2^-24 C_a — 2 K adds form c (K - 1 per
    direction, the coupling), a few ulp come from the normalisation and the product, n_a adds are in the sum; n_a = in-degree,
    C_a = sum over the atom's edges of sum_k |terms[k,e]| (coupled: the mean of that and the same at id_swap[e])."""
    K = terms.shape[0]
    mag = np.abs(np.asarray(terms, np.float64)).sum(0)
    if id_swap is not None:
        mag = 0.5 * (mag + mag[np.asarray(id_swap)])
    C = np.zeros((n_atoms, terms.shape[2]))
    np.add.at(C, np.asarray(id_a), mag)
    n = np.bincount(np.asarray(id_a), minlength=n_atoms).astype(np.float64)
    return (n[:, None] + 2 * K + 8) * 2.0 ** -24 * C


def edge_vectors_ref(R, idx, cell):
    """V (E,3) float64: R[a] - (R[c] + cell_offsets @ cell[b])."""
    R, cell = np.asarray(R, np.float64), np.asarray(cell, np.float64).reshape(-1, 3, 3)
    a, c = idx["id_a"], idx["id_c"]
    shift = np.einsum("ek,ekj->ej", idx["cell_offsets"].astype(np.float64), cell[idx["batch_seg"][a]])
    return R[a] - (R[c] + shift)


# -------------------------------------------------------------------------------------------------------- structures
def one_atom_cell(a):
    """One atom in a cubic cell of edge a, all axes periodic: every edge is a self-image edge into that atom."""
    return np.zeros((1, 3)), np.array([6]), np.eye(3) * a, np.array([True, True, True])


@functools.lru_cache(maxsize=None)
def kernel_case(name):
    """-> (idx (brute-force dict, int64), V (E,3) float32, n_atoms) of 'sc1' (80 in-edges of one atom), 'sc08' (146) or 'zoo'
    (1188 atoms in 46 structures, 4494 edges, in-degree <= 14, 25 atoms without an edge, atoms beyond row 1024)."""
    structs = {"sc1": [one_atom_cell(1.0)], "sc08": [one_atom_cell(0.8)]}[name] if name != "zoo" else P.zoo()
    R, Z, N, cell, pbc = P.arrays(structs)
    idx = P.brute_force_fast(R, N, cell, pbc, P.CUTOFF)
    V = edge_vectors_ref(R, idx, cell).astype(np.float32)
    return idx, V, int(len(R))


KINDS = ("small", "triclinic", "slab")


def moving_system(n_steps=3, seed=7):
    """-> Z, N, pbc, steps [(R float32 (A,3), cell float32 (B,3,3))]: a batch whose atoms move from step to step and whose cells
    strain once (tests/test_pbc_direct_cpu.py checks that the neighbour lists of the three steps differ)."""
    structs = [P.structure(k, seed=i) for i, k in enumerate(KINDS)]
    R, Z, N, cell, pbc = P.arrays(structs)
    rs = np.random.RandomState(seed)
    steps = []
    for s in range(n_steps):
        steps.append((R.astype(np.float32), cell.astype(np.float32)))
        R = R + rs.normal(0, 0.12, R.shape)
        if s == 0:
            cell = cell @ (np.eye(3) + rs.normal(0, 0.004, (3, 3)))
    return Z, N, pbc, steps


# ------------------------------------------------------------------------------------------------------------ model
def direct_cfg(coupled, **kw):
    return dict(P.CFG, direct_forces=True, forces_coupled=bool(coupled), **kw)


@functools.lru_cache(maxsize=None)
def direct_params(coupled, seed=3):
    import os
    from conftest import ROOT
    scale = GO.load_scale_factors(os.path.join(ROOT, "gemnet_pytorch_amd", "scaling_factors.json"))
    return GO.make_params(direct_cfg(coupled), seed, scale)


@functools.lru_cache(maxsize=None)
def cluster_reference(kind, coupled, radius=P.RADIUS):
    """(E, F (n,1,3)) of the structure's central atoms in fp64: the molecular direct-force oracle on the cluster of images within
    `radius` (central atoms = molecule 0, ghosts = molecule 1; P.RADIUS covers the receptive field and the reverse edges that
    the coupling reads)."""
    R, Z, cell, pbc = P.structure(kind)
    cfg, params = direct_cfg(coupled), direct_params(coupled)
    Rc, Zc = P.cluster(R, Z, cell, pbc, radius)
    n = len(R)
    idx = IO.build_indices(Rc, np.array([len(Rc)]), cfg["cutoff"], 10.0, True)
    inputs = {k: torch.tensor(v) for k, v in idx.items()}
    bs = np.zeros(len(Rc), np.int64)
    bs[n:] = 1
    inputs.update(Z=torch.tensor(Zc).long(), R=torch.tensor(Rc), batch_seg=torch.tensor(bs), N=torch.tensor([n, len(Rc) - n]))
    E, F = GO.forward(cfg, params, inputs)
    return float(E[0, 0]), F[:n].detach().numpy().copy()


def direct_model(coupled, switch=True, **kw):
    """The small direct-force GemNet-T of P.CFG on the device with the oracle's weights, in eval mode."""
    from conftest import SCALE_FILE
    from gemnet_pytorch_amd.model.gemnet import GemNet
    m = GemNet(**direct_cfg(coupled, **kw), scale_file=SCALE_FILE)
    if not kw:
        m.load_state_dict(GO.expand_to_reference_state_dict({k: v.float() for k, v in direct_params(coupled).items()}))
    m = m.to(DEV).eval()
    m.periodic_direct_forces = switch
    return m


def device_batch(structs, dtype=torch.float64):
    """A periodic batch on the device, neighbour list from PeriodicGraphBuilder."""
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder
    R, Z, N, cell, pbc = P.arrays(structs)
    b = PeriodicGraphBuilder(N, P.CUTOFF, pbc=pbc, device=DEV)
    idx = b(torch.tensor(R, dtype=dtype, device=DEV), torch.tensor(cell, dtype=dtype, device=DEV))
    inputs = dict(idx)
    inputs.update(R=torch.tensor(R, dtype=torch.float32, device=DEV), Z=torch.tensor(Z, device=DEV).long(),
                  N=torch.tensor(N, device=DEV), cell=torch.tensor(cell, dtype=torch.float32, device=DEV))
    return inputs


def run(model, structs):
    """E (B,1), F (A,1,3) of a list of structures as float64 numpy arrays."""
    E, F = model(device_batch(structs))
    torch.cuda.synchronize()
    return E.double().cpu().numpy(), F.double().cpu().numpy()
