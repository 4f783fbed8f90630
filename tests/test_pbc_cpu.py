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
