"""GPU: the periodic GemNet-Q index build (pbc.PeriodicQuadGraphBuilder, csrc/pbc_index_q.hip) against the brute-force numpy
builder of tests/pbc_q_common.py, array for array, and — without images — against the molecular device builder."""
import numpy as np
import pytest
import torch

import pbc_common as P
import pbc_q_common as Q
from redzone import put, redzone  # noqa: F401  (autouse: every test of this module runs under the red-zone harness)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _device(structs, dtype=torch.float64, out=torch.int64):
    from gemnet_pytorch_amd.pbc import PeriodicQuadGraphBuilder
    R, _, N, cell, pbc = P.arrays(structs)
    b = PeriodicQuadGraphBuilder(N, Q.CUTOFF, Q.INT_CUTOFF, pbc=pbc, device=DEV)
    idx = b(put(torch.tensor(R, dtype=dtype)), put(torch.tensor(cell, dtype=dtype)), dtype=out)
    torch.cuda.synchronize()
    return idx, (R, N, cell, pbc)


def _assert_equal(idx, ref):
    assert set(idx) == set(ref)
    for k, v in ref.items():
        got = idx[k].cpu().numpy()
        assert got.shape == v.shape and np.array_equal(got, v), k


@pytest.mark.parametrize("kinds", [[k] for k in P.OLD_KINDS + P.NEW_KINDS] + [["small", "triclinic_TFF", "slab", "thin"]])
def test_device_builder_equals_brute_force(kinds):
    structs = [P.structure(k, seed=i) for i, k in enumerate(kinds)]
    idx, (R, N, cell, pbc) = _device(structs)
    ref = Q.brute_force_q(R, N, cell, pbc)
    _assert_equal(idx, ref)
    Q.check_invariants({k: v.cpu().numpy() for k, v in idx.items()})
    assert all(v.dtype == torch.int64 for v in idx.values())


def test_triplet_keys_are_the_triplet_builders_bit_for_bit():
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder
    structs = [P.structure(k, seed=i) for i, k in enumerate(["thin", "skewed", "slab"])]
    idx, (R, N, cell, pbc) = _device(structs, out=torch.int32)
    t = PeriodicGraphBuilder(N, Q.CUTOFF, pbc=pbc, device=DEV)(put(torch.tensor(R)), put(torch.tensor(cell)),
                                                                dtype=torch.int32)
    for k, v in t.items():
        assert v.dtype == idx[k].dtype == torch.int32 and torch.equal(v, idx[k]), k


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_without_images_equals_the_molecular_device_builder(dtype):
    """pbc = (F, F, F): every array is the molecular builder's (index_device.DeviceGraphBuilder), array for array — the pin
    of the order of the in-edge lists and of the quadruplets."""
    from gemnet_pytorch_amd.index_device import DeviceGraphBuilder
    rs = np.random.RandomState(1)
    fff = (False, False, False)
    structs = [P.f32_round(s) for s in (P._gas_structure(24, rs, fff, density=0.12), P.structure("small"),
                                         P._gas_structure(70, rs, fff, density=0.1))]
    structs = [(s[0], s[1], s[2], np.array(fff)) for s in structs]
    idx, (R, N, cell, pbc) = _device(structs, dtype=dtype)
    mol = DeviceGraphBuilder(N, Q.CUTOFF, Q.INT_CUTOFF, triplets_only=False, device=DEV)(put(torch.tensor(R, dtype=dtype)))
    assert len(mol["id4_reduce_ca"]) > 5000
    for k, v in mol.items():
        assert torch.equal(idx[k], v), k
    assert (idx["cell_offsets"] == 0).all() and (idx["int_cell_offsets"] == 0).all()


def test_unwrapped_positions():
    R, Z, cell, pbc = P.structure("triclinic")
    R2 = R.copy()
    R2[0] += 2 * cell[0] - cell[1] + 3 * cell[2]
    a, _ = _device([(R, Z, cell, pbc)])
    b, _ = _device([(R2, Z, cell, pbc)])
    assert all(len(a[k]) == len(b[k]) for k in a)
    _assert_equal(b, Q.brute_force_q(R2, [3], cell, pbc))


def test_float32_and_float64_positions_agree():
    # ('slab' and 'skewed' have a lattice vector of exactly int_cutoff = 3.0: a self-image on the boundary, no margin)
    structs = [P.f32_round(P.structure(k, seed=i)) for i, k in enumerate(["triclinic", "thin", "bcc_pert"])]
    R, _, N, cell, pbc = P.arrays(structs)
    assert Q.cutoff_margins_ok(R, N, cell, pbc)
    a, _ = _device(structs, dtype=torch.float64)
    b, _ = _device(structs, dtype=torch.float32)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("out", [torch.int64, torch.int32])
def test_no_edges_and_no_quadruplets_give_empty_arrays(out):
    # an isolated atom: nothing at all; 'triclinic_FFF': edges and interaction edges, but no quadruplet
    idx, _ = _device(P.isolated(1), out=out)
    for k in ["id_a", "cell_offsets", "id3_reduce_ca"] + Q.KEYS_Q:
        assert idx[k].shape[0] == 0 and idx[k].dtype == out, k
    assert idx["cell_offsets"].shape == (0, 3) and idx["int_cell_offsets"].shape == (0, 3)
    s = P.structure("triclinic_FFF")
    idx, (R, N, cell, pbc) = _device([s] + P.isolated(1), out=out)
    assert len(idx["id_a"]) == 2 and len(idx["id4_int_a"]) == 4 and len(idx["id4_reduce_intm_ca"]) == 3
    for k in ("id4_reduce_ca", "id4_expand_db", "id4_reduce_cab", "id4_expand_abd", "Kidx4"):
        assert idx[k].shape == (0,) and idx[k].dtype == out, k
    _assert_equal(idx, {k: v.astype(np.int32 if out == torch.int32 else np.int64)
                        for k, v in Q.brute_force_q(R, N, cell, pbc).items()})


def test_builder_refusals():
    from gemnet_pytorch_amd.pbc import MAX_IMAGES, PeriodicGraphBuilder, PeriodicQuadGraphBuilder
    with pytest.raises(NotImplementedError, match="PeriodicQuadGraphBuilder"):
        PeriodicGraphBuilder([3], Q.CUTOFF, triplets_only=False)
    # the image limit is applied with the larger radius: a height that int_cutoff / MAX_IMAGES exceeds, cutoff / MAX_IMAGES not
    h = 0.5 * (Q.CUTOFF + Q.INT_CUTOFF) / MAX_IMAGES
    cell = torch.tensor(np.diag([h, 4.0, 4.0])[None], device=DEV)
    R = torch.zeros((1, 3), dtype=torch.float64, device=DEV)
    PeriodicGraphBuilder([1], Q.CUTOFF, device=DEV).check_cell(cell.cpu().numpy())
    with pytest.raises(ValueError, match="images per side"):
        PeriodicQuadGraphBuilder([1], Q.CUTOFF, Q.INT_CUTOFF, device=DEV)(R, cell)
