"""Padding of PERIODIC batches to fixed capacities (gemnet_pytorch_amd/padded.py with a cell; no GPU): the pad rows behind the
brute-force image neighbour list (tests/pbc_common.py) form a valid graph of their own on the dummy atoms, the runner's
`_fill` writes what `pad_indices` constructs (`cell_offsets` and the dummy molecule's cell row included), and the new entry
points are declared and bound."""
import os
import re

import numpy as np
import pytest
import torch

import pbc_common as P
from conftest import ROOT
from gemnet_pytorch_amd.padded import PaddedGraphRunner, pad_indices

KEYS = ("id_c", "id_a", "id_swap", "id_undir", "id3_reduce_ca", "id3_expand_ba", "cell_offsets")


class _M:       # the runner only looks at these attributes before a capture
    triplets_only, direct_forces = True, False


def _batch(kinds):
    structs = [P.structure(k, seed=i) for i, k in enumerate(kinds)]
    R = np.concatenate([s[0] for s in structs])
    Z = np.concatenate([s[1] for s in structs])
    N = [len(s[0]) for s in structs]
    cell = np.stack([s[2] for s in structs])
    pbc = np.stack([s[3] for s in structs])
    ref = P.brute_force(R, N, cell, pbc, P.CUTOFF)
    idx = {k: torch.tensor(ref[k]) for k in KEYS}
    return idx, torch.tensor(R, dtype=torch.float32), torch.tensor(Z), torch.tensor(N), torch.tensor(cell, dtype=torch.float32), pbc


@pytest.mark.parametrize("kinds", [["triclinic"], ["small", "triclinic", "slab", "cubic1"]])
def test_pad_rows_of_a_periodic_batch_form_a_valid_graph(kinds):
    idx, R, Z, N, cell, pbc = _batch(kinds)
    A = int(Z.shape[0])
    E, T = int(idx["id_c"].shape[0]), int(idx["id3_reduce_ca"].shape[0])
    deg = PaddedGraphRunner.in_degree_of(idx)
    for e_cap, t_cap, G in ((E + 8, T + 2, 1), (E + 40, T + 300, 3), (E + 4, T, 2), (E, T, 1), (E + 6, T + 4, 2), (E + 16, T + 2, 3),
                            (E + 20, T + 2, 2), (E + 38, T + 2, 3)):
        o = pad_indices(idx, A, e_cap, t_cap, G)
        assert o["cell_offsets"].shape == (e_cap, 3) and not o["cell_offsets"][E:].any()      # offsets 0 behind row E
        for k in KEYS:                                                                        # real rows first, untouched
            assert torch.equal(o[k][:idx[k].shape[0]], idx[k].to(torch.int64)), k
        sw = o["id_swap"]
        assert torch.equal(sw[sw], torch.arange(e_cap))
        assert torch.equal(o["id_c"][sw], o["id_a"]) and torch.equal(o["id_a"][sw], o["id_c"])
        assert torch.equal(o["cell_offsets"][sw], -o["cell_offsets"])
        assert torch.equal(o["id_undir"][sw], o["id_undir"])
        assert int(o["id_undir"].max()) == e_cap // 2 - 1 and torch.bincount(o["id_undir"]).eq(2).all()
        r, x = o["id3_reduce_ca"], o["id3_expand_ba"]
        assert bool((r[1:] >= r[:-1]).all()) and torch.equal(o["id_a"][r], o["id_a"][x]) and bool((r != x).all())
        pad_atoms = torch.cat([o["id_c"][E:], o["id_a"][E:]])
        assert pad_atoms.numel() == 0 or (int(pad_atoms.min()) >= A and int(pad_atoms.max()) < A + 3 * G)
        assert bool((r[T:] >= E).all()) and bool((x[T:] >= E).all())
        # in-degree of the dummy atoms: the runner predicts it EXACTLY (atom a takes both forward edges of a quad: 8 for 40 pad
        # edges over 3 groups, not ceil(20 / 3) = 7), and `fits` / `_fill` accept a padding only within the caller's bound —
        # the real list's in-degree, not a bound sized to the padding
        runner = PaddedGraphRunner(_M(), Z, N, e_cap, t_cap, max_in_degree=deg, n_groups=G, cell=cell, pbc=pbc)
        pad_deg = int(torch.bincount(o["id_a"][E:], minlength=A + 3 * G)[A:].max()) if e_cap > E else 0
        assert pad_deg == runner.pad_in_degree(e_cap - E)
        ok = pad_deg <= runner.pad_degree_bound()
        assert runner.fits((E, T)) == ok
        if ok:
            runner._fill(R, idx)
            assert int(torch.bincount(runner.padded_inputs()["id_a"].long()).max()) <= runner.pad_degree_bound()
        else:
            with pytest.raises(ValueError, match="in-degree"):
                runner._fill(R, idx)
    assert PaddedGraphRunner(_M(), Z, N, E + 40, T + 2, max_in_degree=7, n_groups=3, cell=cell, pbc=pbc).pad_in_degree(40) == 8


def test_periodic_runner_fill_equals_pad_indices():
    idx, R, Z, N, cell, pbc = _batch(["small", "triclinic", "slab", "cubic1"])
    E, T = PaddedGraphRunner.sizes_of(idx)
    n_mol = int(N.shape[0])
    runner = PaddedGraphRunner(_M(), Z, N, E + 42, T + 60, max_in_degree=16, n_groups=3, cell=cell, pbc=pbc)
    got = runner.padded_inputs()
    assert got["cell"].shape == (n_mol + 1, 3, 3) and got["cell"].dtype == torch.float32
    assert torch.equal(got["cell"][n_mol], torch.eye(3)) and torch.equal(got["cell"][:n_mol], cell)
    assert got["cell_offsets"].shape == (runner.e_cap, 3) and got["cell_offsets"].dtype == torch.int32
    fewer = {k: (v[:E - 4] if v.shape[0] == E else v) for k, v in idx.items()}        # stale offsets must not survive
    fewer["id3_reduce_ca"], fewer["id3_expand_ba"] = idx["id3_reduce_ca"][:0], idx["id3_expand_ba"][:0]
    cell2 = cell @ (torch.eye(3) + 0.01 * torch.arange(9.0).reshape(3, 3))
    cur = cell
    for batch, c in ((idx, None), (fewer, cell2), (idx, None)):
        runner._fill(R, batch, cell=c)
        ref = pad_indices(batch, runner.A, runner.e_cap, runner.t_cap, runner.G)
        got = runner.padded_inputs()
        for k, v in ref.items():
            assert torch.equal(got[k].to(torch.int64), v), k
        assert torch.equal(got["R"][:runner.A], R)
        cur = c if c is not None else cur
        assert torch.equal(got["cell"][:n_mol], cur)
        assert torch.equal(got["cell"][n_mol], torch.eye(3))
    assert torch.equal(runner.padded_inputs()["cell"][:n_mol], cell2)                  # the cell stays until another is given
    with pytest.raises(ValueError):       # a molecular dict in a periodic runner
        runner._fill(R, {k: v for k, v in idx.items() if k != "cell_offsets"})
    with pytest.raises(ValueError):
        runner._fill(R, idx, cell=cell[:2])


def test_in_degree_of_and_the_required_bound():
    for kinds in (["cubic1"], ["triclinic"], ["small", "triclinic", "slab", "cubic1"]):
        idx, R, Z, N, cell, pbc = _batch(kinds)
        want = int(np.bincount(idx["id_a"].numpy()).max())
        assert PaddedGraphRunner.in_degree_of(idx) == want
        if kinds == ["cubic1"]:
            assert want >= 6 > int(N.max()) - 1           # one atom, six images within 2.6 A: the molecular bound is wrong
    assert PaddedGraphRunner.in_degree_of({"id_a": torch.zeros(0, dtype=torch.int64)}) == 0
    E, T = PaddedGraphRunner.sizes_of(idx)
    with pytest.raises(ValueError, match="max_in_degree"):
        PaddedGraphRunner(_M(), Z, N, E + 8, T + 2, cell=cell, pbc=pbc)
    with pytest.raises(NotImplementedError):
        PaddedGraphRunner(_M(), Z, N, E + 8, T + 2, max_in_degree=8, a_cap=int(Z.shape[0]) + 4, cell=cell)
    PaddedGraphRunner(_M(), Z, N, E + 8, T + 2)            # molecular runners keep their default bound


def test_new_symbols_are_declared_and_bound():
    from gemnet_pytorch_amd import _lib, hbcheck, kernels
    text = open(os.path.join(ROOT, "include", "gemnet_hip.h")).read()
    assert re.search(r"\bint\s+gn_pbc_index_padded_t\s*\(", text) and re.search(r"\bint64_t\s+gn_pbc_index_ws_bytes\s*\(", text)
    funcs, _ = hbcheck.parse_header()
    sig = funcs["gn_pbc_index_padded_t"]
    assert len(sig) == len(_lib.SIGNATURES["gn_pbc_index_padded_t"])
    kinds = dict(sig)
    # what the happens-before checker derives from the const qualifiers: inputs read, buffers / workspace / state written
    assert all(kinds[k] == "r" for k in ("R", "cell", "pbc", "mol_off", "atom_mol"))
    assert all(kinds[k] == "w" for k in ("ws", "staging", "id_c", "id_a", "id_swap", "id_undir", "cell_offsets", "id3_reduce_ca",
                                         "id3_expand_ba", "state"))
    assert kinds["stream"] == "stream"
    assert callable(kernels.pbc_index_padded_t) and callable(kernels.pbc_index_ws_bytes)
    src = os.path.join(ROOT, "gemnet_pytorch_amd", "csrc", "pbc_index.hip")
    assert os.path.exists(src) and 'extern "C" int gn_pbc_index_padded_t' in open(src).read()
