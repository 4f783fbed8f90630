"""CPU: the periodic oracles — the brute-force image neighbour list on hand-countable cells, and the cluster oracle (converged
in the cluster radius; its central-difference forces and stress are the yardstick of tests/test_gpu_pbc.py)."""
import itertools

import numpy as np
import pytest

import pbc_common as P
from gemnet_pytorch_amd import pbc as PB


def lattice_points(cell, cutoff, pbc=(True, True, True)):
    rng = [range(-6, 7) if p else range(1) for p in pbc]
    return sum(1 for n in itertools.product(*rng) if n != (0, 0, 0) and np.linalg.norm(np.array(n) @ cell) <= cutoff)


@pytest.mark.parametrize("cutoff, expect", [(2.6, 6), (3.0, 18), (3.7, 26)])
def test_one_atom_cubic_cell_sees_its_lattice_points(cutoff, expect):
    cell = np.eye(3) * 2.1
    idx = P.brute_force(np.zeros((1, 3)), [1], cell, [True, True, True], cutoff)
    assert len(idx["id_a"]) == expect == lattice_points(cell, cutoff)
    assert (idx["id_a"] == 0).all() and (idx["id_c"] == 0).all()
    # every image pair once per direction: offsets of the swapped half are the negated forward offsets
    H = len(idx["id_a"]) // 2
    assert (idx["cell_offsets"][H:] == -idx["cell_offsets"][:H]).all()
    assert all(tuple(o) > (0, 0, 0) for o in idx["cell_offsets"][:H])
    # edge identity: an atom forms triplets with its own images, (E - 1) per reduce edge
    E = len(idx["id_a"])
    assert len(idx["id3_reduce_ca"]) == E * (E - 1)


def test_triclinic_cell_matches_lattice_count():
    cell = np.array([[2.0, 0.0, 0.0], [1.3, 1.8, 0.0], [0.4, 0.7, 2.2]])
    for cutoff in (2.1, 2.9, 3.6):
        idx = P.brute_force(np.array([[0.3, -0.2, 0.5]]), [1], cell, [True] * 3, cutoff)
        assert len(idx["id_a"]) == lattice_points(cell, cutoff)


def test_slab_has_no_images_along_the_open_axis():
    cell = np.array([[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 2.0]])
    idx = P.brute_force(np.zeros((1, 3)), [1], cell, [True, True, False], 2.9)
    assert len(idx["id_a"]) == lattice_points(cell, 2.9, (True, True, False)) == 8
    assert (idx["cell_offsets"][:, 2] == 0).all()


def test_large_cell_is_the_molecular_graph():
    from oracle import index_oracle as IO
    R, Z, _, _ = P.structure("small")
    idx = P.brute_force(R, [3], np.eye(3) * 40.0, [True] * 3, 2.6)
    ref = IO.build_indices(R, np.array([3]), 2.6, 10.0, True)
    for k in ref:
        assert np.array_equal(idx[k], ref[k]), k
    assert (idx["cell_offsets"] == 0).all()


def test_image_extent():
    ext = PB.image_extent(np.eye(3) * 2.0, [True, True, False], 5.0)
    assert ext.tolist() == [[3, 3, 0]]


@pytest.fixture(scope="module")
def params():
    return P.make_params()


@pytest.mark.parametrize("kind", ["small", "triclinic", "slab"])
def test_cluster_energy_converges_with_radius(params, kind):
    R, Z, cell, pbc = P.structure(kind)
    e1 = P.cluster_energy(params, R, Z, cell, pbc, radius=P.RADIUS)
    e2 = P.cluster_energy(params, R, Z, cell, pbc, radius=P.RADIUS + 2.0)
    assert abs(e1 - e2) <= 1e-10
    # a cluster below the receptive field is NOT converged (the check above has teeth)
    e0 = P.cluster_energy(params, R, Z, cell, pbc, radius=P.CUTOFF)
    assert abs(e0 - e1) > 1e-6


def test_cluster_energy_is_periodic(params):
    """Moving an atom by a lattice vector, translating everything, or tiling into a 2x1x1 supercell leaves the energy per cell."""
    R, Z, cell, pbc = P.structure("triclinic")
    e = P.cluster_energy(params, R, Z, cell, pbc)
    R2 = R.copy()
    R2[1] += cell[0] - cell[2]
    assert abs(P.cluster_energy(params, R2, Z, cell, pbc) - e) <= 1e-10
    assert abs(P.cluster_energy(params, R + np.array([0.37, -1.2, 0.8]), Z, cell, pbc) - e) <= 1e-10
    Rs = np.concatenate([R, R + cell[0]])
    cs = cell.copy()
    cs[0] *= 2
    assert abs(P.cluster_energy(params, Rs, np.concatenate([Z, Z]), cs, pbc) - 2 * e) <= 1e-9


def test_fd_stress_is_symmetric_and_forces_sum_to_zero(params):
    R, Z, cell, pbc = P.structure("small")
    F, S = P.fd_forces_stress(params, R, Z, cell, pbc)
    assert np.abs(F.sum(0)).max() <= 1e-7
    assert np.abs(S - S.T).max() <= 1e-7 * max(1.0, np.abs(S).max())
    assert np.abs(F).max() > 1e-3 and np.abs(S).max() > 1e-4


# ------------------------------------------------------------------ small / thin / sheared / left-handed cells, size cases
# kind: (E, T, self edges, max |n| per axis, exactly collinear triplets at pi, at 0) at cutoff 2.6, from `brute_force`
COUNTS = {
    "bcc": (28, 364, 12, (1, 1, 1), 28, 0),
    "bcc_pert": (28, 364, 12, None, None, None),
    "thin": (16, 112, 8, (2, 1, 0), 16, 8),
    "skewed": (14, 52, 0, (3, 1, 1), 0, 0),
    "skewed_lh": (16, 70, 0, (2, 3, 1), 0, 0),
    "triclinic_TFF": (6, 6, 0, (1, 0, 0), 0, 0),
    "triclinic_FTT": (6, 8, 0, (0, 1, 1), 0, 0),
    "triclinic_FFF": (2, 0, 0, (0, 0, 0), 0, 0),
}


def _collinear(R, cell, idx):
    V = R[idx["id_a"]] - (R[idx["id_c"]] + idx["cell_offsets"] @ cell)
    u, v = -V[idx["id3_reduce_ca"]], -V[idx["id3_expand_ba"]]
    flat = np.linalg.norm(np.cross(u, v), axis=1) < 1e-12
    dot = (u * v).sum(1)
    return int((flat & (dot < 0)).sum()), int((flat & (dot > 0)).sum())


@pytest.mark.parametrize("kind", sorted(COUNTS))
def test_new_structure_kinds_keep_their_counts(kind):
    """The recipes of pbc_common.structure cannot drift: edges, triplets, self-image edges, the largest image index per axis
    and the exactly collinear triplets (theta = pi between images +n and -n, theta = 0 between n and 2n) of every new kind; the
    nearest pair lies at least 7e-3 A from the cutoff, so float32 and float64 lists agree."""
    E, T, n_self, nmax, at_pi, at_0 = COUNTS[kind]
    R, Z, cell, pbc = P.structure(kind)
    idx = P.brute_force(R, [len(R)], cell, pbc, P.CUTOFF)
    assert (len(idx["id_a"]), len(idx["id3_reduce_ca"]), int((idx["id_a"] == idx["id_c"]).sum())) == (E, T, n_self)
    if nmax is not None:
        assert tuple(np.abs(idx["cell_offsets"]).max(0)) == nmax
        assert _collinear(R, cell, idx) == (at_pi, at_0)
    assert P.cutoff_margin_ok(R, [len(R)], cell, pbc, margin=7e-3)


def test_new_cells_are_the_ones_the_old_kinds_were_not():
    h = {k: P.heights(P.structure(k)[2]) for k in ("thin", "skewed", "skewed_lh", "bcc")}
    assert h["thin"].min() < P.CUTOFF / 2 and h["skewed"].min() < P.CUTOFF / 2
    assert np.allclose(h["skewed"], [0.78, 1.94, 3.3], atol=5e-3)
    assert np.allclose(np.linalg.norm(P.structure("skewed")[2], axis=1), [3.0, 6.66, 5.92], atol=5e-3)
    assert np.linalg.det(P.structure("skewed")[2]) > 0 > np.linalg.det(P.structure("skewed_lh")[2])
    assert np.linalg.norm(P.structure("bcc")[2], axis=1).max() < P.CUTOFF        # every lattice vector is an edge


@pytest.mark.parametrize("kind", P.OLD_KINDS + P.NEW_KINDS)
def test_fast_builder_equals_the_slow_one(kind):
    for seed in (0, 3):
        R, Z, cell, pbc = P.structure(kind, seed)
        if kind in ("thin", "skewed") and seed == 3:       # unwrapped positions
            R = R.copy()
            R[0] += 3 * cell[0] - 2 * cell[1]
            R[1] -= 5 * cell[0]
        a, b = P.brute_force(R, [len(R)], cell, pbc, P.CUTOFF), P.brute_force_fast(R, [len(R)], cell, pbc, P.CUTOFF)
        assert a.keys() == b.keys()
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (kind, k)


def test_fast_builder_equals_the_slow_one_on_batches():
    for structs in ([P.structure(k, seed=i) for i, k in enumerate(P.OLD_KINDS + P.NEW_KINDS)], P.zoo(), P.isolated(5)):
        R, Z, N, cell, pbc = P.arrays(structs)
        a, b = P.brute_force(R, N, cell, pbc, P.CUTOFF), P.brute_force_fast(R, N, cell, pbc, P.CUTOFF)
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert len(b["id_a"]) == 0 and len(b["id3_reduce_ca"]) == 0 and len(b["batch_seg"]) == 5      # the H = 0 batch


def test_every_edge_lies_in_the_image_box_of_its_pair():
    """`image_box` restates image_range of csrc/pbc.hip; no brute-force edge may fall outside it (a box computed with the signed
    determinant in cutoff / height is empty for 'skewed_lh' and would fail here)."""
    for kind in P.OLD_KINDS + P.NEW_KINDS:
        R, Z, cell, pbc = P.f32_round(P.structure(kind))
        idx = P.brute_force_fast(R, [len(R)], cell, pbc, P.CUTOFF)
        H = len(idx["id_a"]) // 2
        for i, j, n in zip(idx["id_a"][:H], idx["id_c"][:H], idx["cell_offsets"][:H]):
            lo, hi = P.image_box(R[i], R[j], cell, pbc)
            assert (lo <= n).all() and (n <= hi).all(), (kind, i, j, n)
    # 'thin' has pairs on both sides of the 64-cell threshold of pbc_index.hip's hit mask
    R, Z, cell, pbc = P.f32_round(P.structure("thin"))
    sizes = [int(np.prod(np.subtract(*P.image_box(R[i], R[j], cell, pbc)[::-1]) + 1)) for i in range(2) for j in range(i, 2)]
    assert min(sizes) <= 64 < max(sizes), sizes


def test_gas_and_zoo_are_what_the_gpu_tests_need():
    R, Z, cell, pbc = P.gas()
    g = P.brute_force_fast(R, [1100], cell, pbc, P.CUTOFF)
    H = len(g["id_a"]) // 2
    assert (H, len(g["id_a"]), len(g["id3_reduce_ca"])) == (1662, 3324, 10044)
    assert 1100 - len(np.unique(g["id_a"])) == 53                                  # atoms without an edge
    assert int((g["cell_offsets"][:H] != 0).any(1).sum()) == 170                    # image edges (undirected)
    assert P.cutoff_margin_ok(R, [1100], cell, pbc, margin=9e-5)                    # nearest pair: 9.8e-5 A from the cutoff
    zs = P.zoo()
    R, Z, N, cell, pbc = P.arrays(zs)
    assert len(zs) >= 40 and sum(N) > 1024
    assert np.array_equal(R, R.astype(np.float32).astype(np.float64)) and np.array_equal(cell, cell.astype(np.float32))
    assert {1, 2, 63, 64, 65, 130} <= set(N) and len({tuple(p) for p in pbc}) >= 6
    z = P.brute_force_fast(R, N, cell, pbc, P.CUTOFF)
    assert P.cutoff_margin_ok(R, N, cell, pbc, margin=1e-5)
    lonely = [b for b in range(len(N)) if N[b] == 1 and cell[b][0, 0] == 30.0]
    deg = np.bincount(z["id_a"], minlength=sum(N))
    off = np.concatenate([[0], np.cumsum(N)])
    assert len(lonely) >= 2 and lonely[-1] == len(N) - 1 and 0 < lonely[0] < len(N) - 1
    assert all(deg[off[b]] == 0 for b in lonely)
    assert off[lonely[0]] < 1024 < off[lonely[-1]]
    # structure boundaries and small cells with self-image edges on both sides of atom 1024
    self_atoms = z["id_a"][z["id_a"] == z["id_c"]]
    assert self_atoms.min() < 1024 < self_atoms.max()
    assert np.abs(z["cell_offsets"]).max() >= 3


# --------------------------------------------------------------------------------------- golden cluster-oracle fixture
GOLDEN_CASES = ("cubic1", "bcc", "bcc_pert", "thin", "skewed", "skewed_lh")


@pytest.fixture(scope="module")
def golden_pbc():
    import os
    from conftest import GOLDEN
    return dict(np.load(os.path.join(GOLDEN, "pbc_cases.npz")))


@pytest.mark.parametrize("kind", GOLDEN_CASES)
def test_golden_pbc_cases_are_the_cluster_oracle(params, golden_pbc, kind):
    """tests/golden/pbc_cases.npz (make_golden.golden_pbc_cases) against the oracle that wrote it: the inputs are the recipe's, the
    energy, one force component and one stress component are recomputed (1e-9), and the energy is converged in the cluster
    radius (1e-10)."""
    g = {k.split(".", 1)[1]: v for k, v in golden_pbc.items() if k.startswith(kind + ".")}
    R, Z, cell, pbc = P.structure(kind)
    assert np.array_equal(g["R"], R) and np.array_equal(g["Z"], Z) and np.array_equal(g["cell"], cell)
    assert np.array_equal(g["pbc"], pbc)
    e = P.cluster_energy(params, R, Z, cell, pbc)
    assert abs(e - float(g["E"])) <= 1e-9
    assert abs(e - P.cluster_energy(params, R, Z, cell, pbc, radius=P.RADIUS + 2.0)) <= 1e-10
    h = 1e-4
    i, k = len(R) - 1, 1
    Rp, Rm = R.copy(), R.copy()
    Rp[i, k] += h
    Rm[i, k] -= h
    f = -(P.cluster_energy(params, Rp, Z, cell, pbc) - P.cluster_energy(params, Rm, Z, cell, pbc)) / (2 * h)
    assert abs(f - g["F"][i, k]) <= 1e-9
    eps = np.zeros((3, 3))
    eps[0, 2] = h
    sp = P.cluster_energy(params, R @ (np.eye(3) + eps), Z, cell @ (np.eye(3) + eps), pbc)
    sm = P.cluster_energy(params, R @ (np.eye(3) - eps), Z, cell @ (np.eye(3) - eps), pbc)
    assert abs((sp - sm) / (2 * h) / abs(np.linalg.det(cell)) - g["S"][0, 2]) <= 1e-9
    assert g["F"].shape == R.shape and g["S"].shape == (3, 3)
    assert np.abs(g["S"] - g["S"].T).max() <= 1e-7 * max(1.0, np.abs(g["S"]).max())


def test_golden_pbc_cases_symmetry(golden_pbc):
    for kind in ("cubic1", "bcc"):
        assert np.abs(golden_pbc[kind + ".F"]).max() <= 1e-9
    S = golden_pbc["cubic1.S"]
    assert np.abs(np.diag(S) - 0.0672).max() <= 1e-4 and np.abs(np.diag(S) - S[0, 0]).max() <= 1e-9
    assert np.abs(S - np.diag(np.diag(S))).max() <= 1e-9
    assert np.abs(golden_pbc["bcc_pert.F"]).max() > 1e-2 and np.abs(golden_pbc["skewed.F"]).max() > 1e-1


# ------------------------------------------------------------- fp64 restatements of the first-order kernels of csrc/pbc.hip
def test_restatements_of_the_first_order_kernels_are_the_derivatives_of_the_oracle_formulas():
    import torch
    import cpu_kernels as CK
    from oracle import basis_oracle as B
    g = torch.Generator().manual_seed(1)
    E, T = 50, 120
    V = (torch.rand(E, 3, generator=g, dtype=torch.float64) - 0.5) * 5
    V[1], V[2] = 2 * V[0], -V[0]
    red = torch.randint(0, E, (T,), generator=g).int()
    exp = (red + 1 + torch.randint(0, E - 1, (T,), generator=g).int()) % E
    red[:2], exp[:2] = 0, torch.tensor([1, 2])
    z, nrm = torch.tensor(B.jn_zeros(7, 6)), torch.tensor(B.sph_bessel_normalizer(7, 6))
    freq = torch.arange(1, 7, dtype=torch.float64) * np.pi
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    gD, grbf, grad, gY = rnd(E), rnd(E, 6), rnd(E, 7, 6), rnd(T, 7)
    Vg = V.clone().requires_grad_(True)
    Dg = torch.sqrt((Vg * Vg).sum(1))
    tot = (gD * Dg).sum() + (grbf * B.bessel_rbf(Dg, freq, 6.0, 5)).sum() + (grad * B.sph_bessel_radial(Dg, 7, 6, 6.0, 5)).sum()
    (ref,) = torch.autograd.grad(tot, Vg)
    D, rbf, rad = CK.edge_basis_vec_fwd(V, freq, z, nrm, 6.0, 5)
    assert torch.allclose(rbf, B.bessel_rbf(D, freq, 6.0, 5), atol=1e-14) and rad.shape == (E, 7, 6)
    assert (CK.edge_basis_vec_bwd(gD, grbf, grad, V, freq, z, nrm, 6.0, 5) - ref).abs().max() <= 1e-12
    Y, th = CK.trip_basis_vec_fwd(V, red, exp, 7)
    assert th[0] < 1e-8 and abs(float(th[1]) - np.pi) < 1e-8
    u = (-V[red.long()]).clone().requires_grad_(True)
    v = (-V[exp.long()]).clone().requires_grad_(True)
    ru, rv = torch.autograd.grad((gY * B.real_sph_harm_l0(7, CK._angle_uv(u, v))).sum(), (u, v))
    Gu, Gv = CK.trip_basis_vec_bwd(gY, V, red, exp)
    assert (Gu - ru).abs().max() <= 1e-12 and (Gv - rv).abs().max() <= 1e-12
    assert torch.isfinite(Gu).all() and Gu[:2].abs().max() <= 1e-15                 # the clamped rows
    # edge vectors and stress against pbc_train_common's plan-based restatements on a real batch
    import types
    import pbc_train_common as PT
    structs = [P.structure(k, seed=i) for i, k in enumerate(P.NEW_KINDS)]
    R, Z, N, cell, pbc = P.arrays(structs)
    idx = {k: torch.tensor(a) for k, a in P.brute_force_fast(R, N, cell, pbc, P.CUTOFF).items()}
    w = lambda t: types.SimpleNamespace(idx32=t.int())                      # noqa: E731
    plan = types.SimpleNamespace(id_a=w(idx["id_a"]), id_c=w(idx["id_c"]), batch_seg=w(idx["batch_seg"]),
                                 cell_offsets=idx["cell_offsets"].int(), n_mol=len(N))
    Rt, ct = torch.tensor(R), torch.tensor(cell)
    Vb = CK.pbc_edge_vec(Rt, idx["id_c"], idx["id_a"], idx["batch_seg"], ct, idx["cell_offsets"])
    assert torch.equal(Vb, PT.edge_vectors(Rt, plan, ct))
    assert float(Vb.norm(dim=1).max()) <= P.CUTOFF and float(Vb.norm(dim=1).min()) > 0.5
    G = rnd(Vb.shape[0], 3)
    key = idx["batch_seg"][idx["id_a"]]
    perm = torch.argsort(key, stable=True).flip(0)                            # grouped by structure, unsorted inside
    perm = torch.cat([perm[key[perm] == b] for b in range(len(N))])
    seg = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(key, minlength=len(N)), 0)])
    assert (CK.pbc_stress(Vb, G, perm, seg, ct) - PT.stress(Vb, G, plan, ct)).abs().max() <= 1e-12
