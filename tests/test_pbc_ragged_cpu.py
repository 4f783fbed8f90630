"""Periodic batches with changing structure SIZES through one set of capacity buffers (no GPU): the layout reference
`padded.capacity_layout` against what the molecular `_fill` writes, a periodic runner's `_fill` with an atom capacity against
`pad_indices` on every batch of tests/pbc_ragged_common.py, the opt-in switch `model.periodic_atom_capacity` and the refusals that
stay word for word without it (the training step refuses an atom capacity either way), and the declarations of the two new entry
points."""
import os
import re

import numpy as np
import pytest
import torch

import pbc_common as P
import pbc_padded_train_common as C
import pbc_ragged_common as G
import pbc_train_common as PT
from conftest import ROOT
from gemnet_pytorch_amd.padded import PaddedGraphRunner, capacity_layout, pad_indices
from gemnet_pytorch_amd.training.periodic import PeriodicPaddedTrainStep
from test_model_cpu import build


class _M:       # the runner only looks at these attributes before a capture
    triplets_only, direct_forces = True, False


class _Mon(_M):
    periodic_atom_capacity = True


class _Q:
    triplets_only, direct_forces = False, False
    periodic_quadruplets = periodic_quadruplets_dynamic = periodic_atom_capacity = True


@pytest.mark.parametrize("N,a_cap", [([3, 3, 3, 1], 72), ([65, 3, 3, 1], 72), ([1], 1), ([2, 1, 5], 9), ([1] * 7, 30)])
def test_capacity_layout_is_what_the_molecular_fill_writes(N, a_cap):
    n_mol, A = len(N), sum(N)
    first = [a_cap - n_mol + 1] + [1] * (n_mol - 1)              # another layout first: every row is rewritten
    run = PaddedGraphRunner(_M(), torch.ones(a_cap, dtype=torch.int64), torch.tensor(first), 8, 2, max_in_degree=4, n_groups=2,
                            a_cap=a_cap)
    empty = {k: torch.zeros(0, dtype=torch.int64) for k in ("id_c", "id_a", "id_swap", "id_undir", "id3_reduce_ca", "id3_expand_ba")}
    run._fill(torch.zeros(A, 3), empty, Z=torch.ones(A, dtype=torch.int64), N=torch.tensor(N))
    lay = capacity_layout(torch.tensor(N), n_mol, a_cap, run.A_tot)
    got = run.padded_inputs()
    assert lay["N"].dtype == torch.int64 and torch.equal(lay["N"], got["N"]) and int(lay["N"][-1]) == run.A_tot - A
    assert lay["batch_seg"].dtype == torch.int64 and torch.equal(lay["batch_seg"], got["batch_seg"])
    assert lay["mol_off"].dtype == torch.int32 and lay["mol_off"].tolist() == [0] + list(np.cumsum(N)) + [a_cap]
    assert lay["atom_mol"].dtype == torch.int32 and torch.equal(lay["atom_mol"].long(), got["batch_seg"][:a_cap])
    assert lay["mask"].dtype == torch.float32 and lay["mask"].tolist() == [1.0] * A + [0.0] * (a_cap - A)
    with pytest.raises(ValueError):
        capacity_layout(torch.tensor(N + [1]), n_mol, a_cap, run.A_tot)


def _runner(model, b0, **kw):
    e_cap, t_cap, deg, groups = G.CAPS
    R, Z, N, cell, idx = G.tensors(b0, "cpu")
    return PaddedGraphRunner(model, Z, N, e_cap, t_cap, max_in_degree=deg, n_groups=groups, a_cap=G.A_CAP, cell=cell,
                             pbc=b0["pbc"], **kw)


def test_fill_with_a_cell_and_an_atom_capacity_equals_pad_indices():
    stream = G.stream()
    run = _runner(_Mon(), stream[0])
    assert run.variable_atoms and run.periodic and run.a_cap == G.A_CAP
    prev_A = None
    for s, b in enumerate(stream):
        R, Z, N, cell, idx = G.tensors(b, "cpu")
        A = int(Z.shape[0])
        run._fill(R, idx, Z, N, cell)
        got = run.padded_inputs()
        ref = pad_indices(idx, run.a_cap, run.e_cap, run.t_cap, run.G)       # the dummy groups sit behind the CAPACITY
        E = int(idx["id_c"].shape[0])
        for k, v in ref.items():
            assert torch.equal(got[k].to(torch.int64), v), (s, k)
        assert not got["cell_offsets"][E:].any()
        lay = capacity_layout(N, G.N_MOL, run.a_cap, run.A_tot)
        assert torch.equal(got["N"], lay["N"]) and torch.equal(got["batch_seg"], lay["batch_seg"])
        assert torch.equal(got["R"][:A], R) and torch.equal(got["Z"][:A], Z)
        # fillers: isolated atoms of the dummy structure at their own positions, Z = 1 — also the rows that were real before
        assert torch.equal(got["R"][A:run.a_cap], run._R_fill[A:]) and bool((got["Z"][A:] == 1).all()), (s, prev_A)
        for k in ("id_c", "id_a"):
            assert not bool(((got[k] >= A) & (got[k] < run.a_cap)).any()), (s, k)     # no filler atom in any list
        assert torch.equal(got["cell"][:G.N_MOL], cell) and torch.equal(got["cell"][G.N_MOL], torch.eye(3))
        prev_A = A
    R, Z, N, cell, idx = G.tensors(stream[1], "cpu")
    with pytest.raises(ValueError, match="the number of atoms changed"):
        run._fill(R, idx, cell=cell)                             # A changed, N / Z missing
    with pytest.raises(ValueError, match="changes the number of molecules"):
        run._fill(R, idx, Z, N[:3], cell)
    big = torch.zeros(G.A_CAP + 1, 3)
    with pytest.raises(ValueError, match=f"exceeds a_cap = {G.A_CAP}"):
        run._fill(big, idx, torch.ones(G.A_CAP + 1, dtype=torch.int64), torch.tensor([G.A_CAP - 2, 1, 1, 1]), cell)


def test_the_switch_and_the_refusals():
    b0 = G.stream()[0]
    R, Z, N, cell, idx = G.tensors(b0, "cpu")
    e_cap, t_cap, deg, groups = G.CAPS
    # off (absent or False): today's refusal, word for word
    for model in (_M(), type("_Off", (_M,), {"periodic_atom_capacity": False})()):
        with pytest.raises(NotImplementedError) as err:
            _runner(model, b0)
        assert str(err.value) == "periodic cells: fixed structure layout only (no a_cap)"
    # on: GemNet-Q with an atom capacity and a cell still raises, naming GemNet-Q
    with pytest.raises(NotImplementedError, match="GemNet-Q"):
        PaddedGraphRunner(_Q(), Z, N, e_cap, t_cap, max_in_degree=deg, n_groups=groups, a_cap=G.A_CAP, cell=cell,
                          quad_caps=(8, 8, 8))
    # a molecular runner with a_cap refuses attach_builder with today's text — also for a capacity builder
    mol = PaddedGraphRunner(_Mon(), Z, N, e_cap, t_cap, a_cap=G.A_CAP)
    for builder in (object(), _fake_capacity_builder()):
        with pytest.raises(NotImplementedError) as err:
            mol.attach_builder(builder)
        assert str(err.value) == "the in-graph index build needs a fixed molecule layout (no a_cap)"
    # a periodic runner with a_cap takes a capacity builder only, and only one of its own sizes
    run = _runner(_Mon(), b0)
    with pytest.raises(NotImplementedError) as err:
        run.attach_builder(object())
    assert str(err.value) == "the in-graph index build needs a fixed molecule layout (no a_cap)"
    with pytest.raises(RuntimeError, match="attach_builder"):
        run.run_positions(R, Z=Z, N=N, cell=cell)
    # the training step: constructing it with a_cap does not set the switch
    with C.emulate(direct=False):
        t = build(P.CFG, PT.make_params(P.CFG)).train()
        kw = dict(cell=cell, pbc=b0["pbc"], max_in_degree=deg, n_groups=groups, rho_force=PT.RHO_FORCE)
        with pytest.raises(NotImplementedError) as err:
            PeriodicPaddedTrainStep(t, Z, N, e_cap, t_cap, a_cap=G.A_CAP, **kw)
        assert str(err.value) == "periodic cells: fixed structure layout only (no a_cap)"
        assert not getattr(t, "periodic_atom_capacity", False)
        # with the switch on the step itself refuses: training keeps the fixed structure layout
        t.periodic_atom_capacity = True
        with pytest.raises(NotImplementedError, match="inference only"):
            PeriodicPaddedTrainStep(t, Z, N, e_cap, t_cap, a_cap=G.A_CAP, **kw)
        assert not getattr(t, "periodic_training", False)
        q = build(dict(P.CFG, triplets_only=False), PT.make_params(dict(P.CFG, triplets_only=False))).train()
        q.periodic_atom_capacity = True
        with pytest.raises(NotImplementedError, match="GemNet-Q"):
            PeriodicPaddedTrainStep(q, Z, N, e_cap, t_cap, a_cap=G.A_CAP, **kw)


def _fake_capacity_builder():
    """A capacity builder without touching a device: `attach_builder` of a molecular runner must refuse before it looks."""
    from gemnet_pytorch_amd.pbc import PeriodicCapacityGraphBuilder
    return PeriodicCapacityGraphBuilder.__new__(PeriodicCapacityGraphBuilder)


def test_new_symbols_are_declared_and_bound():
    from gemnet_pytorch_amd import _lib, hbcheck, kernels, pbc
    text = open(os.path.join(ROOT, "include", "gemnet_hip.h")).read()
    assert re.search(r"\bint\s+gn_pbc_layout\s*\(", text) and re.search(r"\bint\s+gn_pbc_index_padded_tv\s*\(", text)
    funcs, _ = hbcheck.parse_header()
    lay, tv, t = funcs["gn_pbc_layout"], funcs["gn_pbc_index_padded_tv"], funcs["gn_pbc_index_padded_t"]
    assert len(lay) == len(_lib.SIGNATURES["gn_pbc_layout"]) == 12
    assert len(tv) == len(_lib.SIGNATURES["gn_pbc_index_padded_tv"]) == len(t) - 1      # (B, A) -> n_mol
    kinds = dict(lay)
    assert all(kinds[k] == "r" for k in ("N", "n_atoms"))
    assert all(kinds[k] == "w" for k in ("mol_off", "atom_mol", "batch_seg", "N_pad", "mask", "state"))
    assert lay[-1] == ("stream", "stream")
    kinds = dict(tv)
    assert all(kinds[k] == "r" for k in ("R", "cell", "pbc", "mol_off", "atom_mol"))
    assert all(kinds[k] == "w" for k in ("ws", "staging", "id_c", "id_a", "id_swap", "id_undir", "cell_offsets", "id3_reduce_ca",
                                         "id3_expand_ba", "state"))
    assert tv[-1] == ("stream", "stream")
    # the fixed-layout entry keeps its signature
    assert [n for n, _ in t][:7] == ["R", "cell", "pbc", "mol_off", "atom_mol", "B", "A"]
    assert callable(kernels.pbc_layout) and callable(kernels.pbc_index_padded_tv) and callable(pbc.PeriodicCapacityGraphBuilder)
    src = open(os.path.join(ROOT, "gemnet_pytorch_amd", "csrc", "pbc_index.hip")).read()
    assert 'extern "C" int gn_pbc_layout' in src and 'extern "C" int gn_pbc_index_padded_tv' in src
    assert "gn_abi_version() == 16" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
