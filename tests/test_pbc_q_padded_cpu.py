"""Padding of PERIODIC QUADRUPLET batches to fixed capacities (gemnet_pytorch_amd/padded.py with a cell and quad_caps; no GPU):
the pad rows behind the brute-force image quadruplet lists (tests/pbc_q_common.py) form a valid graph of their own on the dummy
atoms, both offset arrays are carried with zero pad rows, the runner's `_fill` writes what `pad_indices` constructs, the opt-in
is needed, and the new entry points are declared and bound."""
import os
import re

import numpy as np
import pytest
import torch

import pbc_common as P
import pbc_q_common as Q
import pbc_q_padded_common as C
from conftest import ROOT
from gemnet_pytorch_amd.padded import PaddedGraphRunner, pad_indices


class _M:       # the runner only looks at these attributes before a capture
    triplets_only, direct_forces = False, False
    periodic_quadruplets = periodic_quadruplets_dynamic = True


def _batch(kinds):
    structs = [P.structure(k, seed=i) for i, k in enumerate(kinds)]
    R, Z, N, cell, pbc = P.arrays(structs)
    ref = Q.brute_force_q(R, N, cell, pbc)
    return (ref, C.idx_tensors(ref), torch.tensor(R, dtype=torch.float32), torch.tensor(Z), torch.tensor(N),
            torch.tensor(cell, dtype=torch.float32), pbc)


@pytest.mark.parametrize("kinds", [["triclinic"], ["small", "triclinic", "slab", "bcc_pert"]])
def test_pad_rows_of_a_periodic_quadruplet_batch_form_a_valid_graph(kinds):
    ref, idx, R, Z, N, cell, pbc = _batch(kinds)
    A = int(Z.shape[0])
    n = C.sizes(ref)
    assert min(n) > 0
    # (edge padding, the four other paddings, dummy groups): nothing; one unit of six; uneven remainders behind one unit in
    # every family; several units over one and over three groups
    for pad, G in (((0, 0, 0, 0, 0), 1), ((6, 2, 2, 3, 5), 1), ((6, 0, 1, 1, 1), 1), ((8, 4, 3, 7, 11), 1), ((10, 6, 1, 5, 2), 1),
                   ((6, 0, 0, 0, 0), 1), ((6, 2, 0, 0, 0), 2), ((20, 10, 5, 9, 31), 1), ((44, 30, 9, 40, 333), 3)):
        caps = tuple(c + p for c, p in zip(n, pad))
        o = pad_indices(idx, A, caps[0], caps[1], G, quad_caps=caps[2:])
        assert set(o) == set(C.IDX_KEYS)
        assert o["cell_offsets"].shape == (caps[0], 3) and o["int_cell_offsets"].shape == (caps[2], 3)
        C.check_padded({k: v.numpy() for k, v in o.items()}, ref, A, caps, G)
    with pytest.raises(ValueError, match="unit of six"):
        pad_indices(idx, A, n[0] + 4, n[1], 1, quad_caps=(n[2], n[3] + 1, n[4]))


def test_periodic_quadruplet_runner_fill_equals_pad_indices():
    ref, idx, R, Z, N, cell, pbc = _batch(["small", "triclinic", "slab", "bcc_pert"])
    n = C.sizes(ref)
    n_mol = int(N.shape[0])
    caps = (n[0] + 42, n[1] + 60, n[2] + 9, n[3] + 17, n[4] + 101)
    runner = PaddedGraphRunner(_M(), Z, N, caps[0], caps[1], max_in_degree=2 * C.in_degree(ref), n_groups=3, quad_caps=caps[2:],
                               cell=cell, pbc=pbc)
    got = runner.padded_inputs()
    assert torch.equal(got["cell"][n_mol], torch.eye(3)) and torch.equal(got["cell"][:n_mol], cell)      # the dummy cell row
    assert got["int_cell_offsets"].shape == (caps[2], 3) and got["int_cell_offsets"].dtype == torch.int32
    assert got["cell_offsets"].shape == (caps[0], 3) and got["cell_offsets"].dtype == torch.int32
    # two smaller batches of other structures with the same atoms per structure would change the layout: shrink the batch by
    # recomputing the lists of the same atoms at shorter cutoffs instead — every family shrinks, stale rows must not survive
    structs = [P.structure(k, seed=i) for i, k in enumerate(["small", "triclinic", "slab", "bcc_pert"])]
    Rn, _, Nn, celln, pbcn = P.arrays(structs)
    fewer = C.idx_tensors(Q.brute_force_q(Rn, Nn, celln, pbcn, cutoff=2.2, int_cutoff=2.7))
    fewest = C.idx_tensors(Q.brute_force_q(Rn, Nn, celln, pbcn, cutoff=1.9, int_cutoff=2.3))
    assert all(a > b > c for a, b, c in zip(n, C.sizes(fewer), C.sizes(fewest)))
    assert bool(idx["cell_offsets"][C.sizes(fewest)[0]:].any()) and bool(idx["int_cell_offsets"][C.sizes(fewest)[2]:].any())
    cell2 = cell @ (torch.eye(3) + 0.01 * torch.arange(9.0).reshape(3, 3))
    cur = cell
    for batch, c in ((idx, None), (fewest, cell2), (fewer, None), (idx, None)):
        runner._fill(R, batch, cell=c)
        want = pad_indices(batch, runner.A, runner.e_cap, runner.t_cap, runner.G, quad_caps=runner.quad_caps)
        got = runner.padded_inputs()
        assert set(want) == set(C.IDX_KEYS)
        for k, v in want.items():
            assert torch.equal(got[k].to(torch.int64), v), k
        cur = c if c is not None else cur
        assert torch.equal(got["cell"][:n_mol], cur) and torch.equal(got["cell"][n_mol], torch.eye(3))
        assert torch.equal(got["R"][:runner.A], R)
    with pytest.raises(ValueError):       # a GemNet-T periodic dict in a quadruplet runner
        runner._fill(R, {k: v for k, v in idx.items() if k != "int_cell_offsets"})
    with pytest.raises(NotImplementedError):
        PaddedGraphRunner(_M(), Z, N, caps[0], caps[1], max_in_degree=16, quad_caps=caps[2:], a_cap=int(Z.shape[0]) + 4, cell=cell)


def test_without_the_opt_in_the_constructor_raises():
    ref, idx, R, Z, N, cell, pbc = _batch(["triclinic"])
    n = C.sizes(ref)
    for flags in ((False, False), (True, False), (False, True)):
        m = _M()
        m.periodic_quadruplets, m.periodic_quadruplets_dynamic = flags
        with pytest.raises(NotImplementedError, match="GemNet-Q"):
            PaddedGraphRunner(m, Z, N, n[0] + 12, n[1] + 2, max_in_degree=16, quad_caps=(n[2] + 4, n[3] + 4, n[4] + 4), cell=cell,
                              pbc=pbc)
    from gemnet_pytorch_amd.md import DeviceMolecule
    with pytest.raises(NotImplementedError, match="GemNet-Q"):
        DeviceMolecule(R.numpy(), Z.numpy(), Q.CUTOFF, Q.INT_CUTOFF, triplets_only=False, cell=cell[0].numpy())
    DeviceMolecule(R.numpy(), Z.numpy(), Q.CUTOFF, Q.INT_CUTOFF, triplets_only=False, cell=cell[0].numpy(), periodic_quadruplets=True)
    from gemnet_pytorch_amd.model.gemnet import GemNet
    from conftest import SCALE_FILE
    assert GemNet(**Q.CFG_Q, scale_file=SCALE_FILE).periodic_quadruplets_dynamic is False


def test_new_symbols_are_declared_and_bound():
    from gemnet_pytorch_amd import _lib, hbcheck, kernels
    text = open(os.path.join(ROOT, "include", "gemnet_hip.h")).read()
    assert re.search(r"\bint\s+gn_pbc_qindex_padded\s*\(", text) and re.search(r"\bint64_t\s+gn_pbc_qindex_ws_bytes\s*\(", text)
    funcs, _ = hbcheck.parse_header()
    for name in ("gn_pbc_qindex_padded", "gn_pbc_qindex_ws_bytes"):
        assert len(funcs[name]) == len(_lib.SIGNATURES[name]), name
    kinds = dict(funcs["gn_pbc_qindex_padded"])
    # what the happens-before checker and the red-zone harness derive from the const qualifiers
    assert all(kinds[k] == "r" for k in ("R", "cell", "pbc", "mol_off", "atom_mol"))
    assert all(kinds[k] == "w" for k in ("ws", "staging", "state"))
    assert kinds["arrays"] == "wa"                       # a host table of device pointers, every one of them written
    assert kinds["stream"] == "stream"
    assert callable(kernels.pbc_index_padded_q) and callable(kernels.pbc_qindex_ws_bytes)
    assert kernels.PADDED_QP_KEYS[:16] == kernels.PADDED_Q_KEYS and kernels.PADDED_QP_KEYS[16:] == ("cell_offsets", "int_cell_offsets")
    src = os.path.join(ROOT, "gemnet_pytorch_amd", "csrc", "pbc_index_qp.hip")
    body = open(src).read()
    assert 'extern "C" int gn_pbc_qindex_padded' in body and 'extern "C" int64_t gn_pbc_qindex_ws_bytes' in body
    assert _lib.SIGNATURES["gn_abi_version"] is not None


def test_trajectories_of_the_gpu_tests_are_well_posed():
    """The recipes the GPU tests rely on (the helper asserts margins, changing counts and an atom outside its cell)."""
    for args in (C.TRAJ_BATCH, C.TRAJ_THIN):
        Z, N, pbc, steps = C.trajectory(*args)
        assert len(steps) == C.STEPS and all(s[0].dtype == np.float32 and s[1].dtype == np.float32 for s in steps)
