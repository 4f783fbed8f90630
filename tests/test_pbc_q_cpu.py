"""CPU: the brute-force periodic quadruplet index build of tests/pbc_q_common.py (the reference the device builder is held
to) against the molecular index oracle where no image exists, its invariants on small / thin / sheared cells, and the golden
cluster-oracle fixture tests/golden/pbc_q_cases.npz against the oracle that wrote it."""
import os

import numpy as np
import pytest

import pbc_common as P
import pbc_q_common as Q
from conftest import GOLDEN
from oracle import index_oracle as IO


def _gas(n, seed, density=0.12):
    return P._gas_structure(n, np.random.RandomState(seed), (False, False, False), density=density)


@pytest.mark.parametrize("structs", [[P.structure("small")], [_gas(24, 1)], [_gas(9, 2), P.structure("slab"), _gas(17, 3)]])
def test_without_images_the_brute_force_is_the_molecular_oracle(structs):
    R, _, N, cell, _ = P.arrays(structs)
    idx = Q.brute_force_q(R, N, cell, [(False, False, False)] * len(N))
    ref = IO.build_indices(R, np.array(N), Q.CUTOFF, Q.INT_CUTOFF, False)
    assert len(ref["id_a"]) > 0
    for k, v in ref.items():
        assert np.array_equal(idx[k], v), k
    assert not idx["cell_offsets"].any() and not idx["int_cell_offsets"].any()
    Q.check_invariants(idx)


def test_the_molecular_pin_has_quadruplets():
    R, _, N, cell, _ = P.arrays([_gas(24, 1)])
    assert len(Q.brute_force_q(R, N, cell, [(False,) * 3])["id4_reduce_ca"]) > 1000


@pytest.mark.parametrize("kind", ["bcc", "thin", "skewed"])
def test_invariants_with_images(kind):
    R, _, cell, pbc = P.structure(kind)
    idx = Q.brute_force_q(R, [len(R)], cell, pbc)
    Q.check_invariants(idx)
    assert len(idx["id4_reduce_ca"]) > 500 and np.abs(idx["int_cell_offsets"]).max() >= 1
    # self-image interaction edges, and quadruplets whose c and d (or a and d, c and b) are one atom in two images
    assert (idx["id4_int_a"] == idx["id4_int_b"]).any()
    c, a, b, d = Q.quad_nodes(idx)
    assert (c[:, 0] == d[:, 0]).any() and (a[:, 0] == d[:, 0]).any() and (c[:, 0] == b[:, 0]).any()
    # the triplet part is pbc_common's builder
    ref = P.brute_force(R, [len(R)], cell, pbc, Q.CUTOFF)
    for k, v in ref.items():
        assert np.array_equal(idx[k], v), k


# --------------------------------------------------------------------------------------- golden cluster-oracle fixture
@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "pbc_q_cases.npz")))


def test_golden_holds_every_case(golden):
    for tag, kinds in Q.GOLDEN_CASES.items():
        for kind in kinds:
            R, Z, cell, pbc = P.structure(kind)
            g = {k: golden[f"{tag}.{kind}.{k}"] for k in ("R", "Z", "cell", "pbc", "E", "F", "S")}
            assert np.array_equal(g["R"], R) and np.array_equal(g["Z"], Z) and np.array_equal(g["cell"], cell)
            assert np.array_equal(g["pbc"], pbc) and g["F"].shape == R.shape and g["S"].shape == (3, 3)
            assert np.abs(g["S"] - g["S"].T).max() <= 1e-7 * max(1.0, np.abs(g["S"]).max())


def test_golden_slab_is_recomputed_from_the_oracle(golden):
    """Energy, one force and one stress component of 'slab' (1e-9), as tests/test_pbc_cpu.py does for the GemNet-T fixture."""
    cfg = Q.CFGS["q"]
    params = Q.make_params(cfg)
    R, Z, cell, pbc = P.structure("slab")
    assert abs(Q.cluster_energy(params, R, Z, cell, pbc, cfg) - float(golden["q.slab.E"])) <= 1e-9
    assert abs(Q.fd_force(params, R, Z, cell, pbc, cfg, len(R) - 1, 1) - golden["q.slab.F"][-1, 1]) <= 1e-9
    assert abs(Q.fd_stress(params, R, Z, cell, pbc, cfg, 0, 1) - golden["q.slab.S"][0, 1]) <= 1e-9


@pytest.mark.parametrize("kind", ["small", "triclinic", "slab", "thin"])
def test_golden_energy_does_not_depend_on_the_cluster_radius(golden, kind):
    """The cluster radius 3 cutoff + int_cutoff + 0.5 covers the receptive field: 1.5 A more changes nothing."""
    cfg = Q.CFGS["q"]
    params = Q.make_params(cfg)
    R, Z, cell, pbc = P.structure(kind)
    e = Q.cluster_energy(params, R, Z, cell, pbc, cfg, radius=Q.RADIUS + 1.5)
    assert abs(e - float(golden[f"q.{kind}.E"])) <= 1e-10 * max(1.0, abs(e))
