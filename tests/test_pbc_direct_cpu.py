"""CPU: the fp64 restatement of the direct force head against the literal reference formulation, its momentum conservation
with coupled forces, the fixtures of the GPU kernel test, and the binding of gn_direct_force_f32."""
import os
import re

import numpy as np
import pytest

import pbc_common as P
import pbc_direct_common as D
from conftest import ROOT
from gemnet_pytorch_amd import _lib


def _terms(K, E, T, seed=0):
    return np.random.RandomState(seed).standard_normal((K, E, T))


@pytest.mark.parametrize("coupled", [False, True])
@pytest.mark.parametrize("K,T", [(1, 1), (5, 3)])
def test_ref_equals_the_literal_reference_formulation(coupled, K, T):
    idx, V, A = D.kernel_case("zoo")
    terms = _terms(K, len(V), T)
    F = D.direct_force_ref(terms, V, idx["id_swap"] if coupled else None, idx["id_a"], A)
    F_lit = D.literal_ref(terms, V, idx["id_undir"] if coupled else None, idx["id_a"], A)
    assert F.shape == (A, T, 3)
    assert np.abs(F - F_lit).max() <= 1e-12 * max(1.0, np.abs(F_lit).max())


def test_coupled_forces_sum_to_zero_per_fully_periodic_structure():
    structs = P.zoo()
    R, Z, N, cell, pbc = P.arrays(structs)
    idx, V, A = D.kernel_case("zoo")
    F = D.direct_force_ref(_terms(5, len(V), 3), V, idx["id_swap"], idx["id_a"], A)
    off, checked = 0, 0
    for n, p in zip(N, pbc):
        if p.all():
            assert np.abs(F[off:off + n].sum(0)).max() <= 1e-12 * max(1.0, np.abs(F[off:off + n]).max())
            checked += 1
        off += n
    assert checked >= 10
    # uncoupled forces do not: the property belongs to the coupling
    Fu = D.direct_force_ref(_terms(5, len(V), 3), V, None, idx["id_a"], A)
    assert np.abs(Fu[:N[0] + N[1]].sum(0)).max() > 1e-3


def test_kernel_fixtures():
    """What the GPU kernel test relies on: the in-degrees beyond one and two wavefronts, the zoo's sizes, no pair on the cutoff."""
    for name, a, edges in (("sc1", 1.0, 80), ("sc08", 0.8, 146)):
        idx, V, A = D.kernel_case(name)
        assert A == 1 and len(V) == edges and (idx["id_a"] == 0).all() and (idx["id_c"] == 0).all()
        assert np.array_equal(idx["id_swap"][idx["id_swap"]], np.arange(edges))
        R, Z, N, cell, pbc = P.arrays([D.one_atom_cell(a)])
        assert P.cutoff_margin_ok(R, N, cell, pbc)
    idx, V, A = D.kernel_case("zoo")
    deg = np.bincount(idx["id_a"], minlength=A)
    assert A == 1188 and len(V) == 4494 and deg.max() == 14 and (deg == 0).sum() == 25 and idx["id_a"].max() >= 1024
    assert np.linalg.norm(V, axis=1).min() > 0.5


def test_header_declares_and_lib_binds_the_entry_point():
    with open(os.path.join(ROOT, "include", "gemnet_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    decl = re.search(r"int\s+gn_direct_force_f32\s*\((.*?)\)\s*;", text, flags=re.S)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == len(_lib.SIGNATURES["gn_direct_force_f32"]) == 11
    # every input pointer is const (hbcheck derives read / write modes from the qualifiers); F is the only output
    ptrs = [a for a in args if "*" in a and not a.startswith("void")]
    assert [a.split()[-1].lstrip("*") for a in ptrs if not a.startswith("const")] == ["F"]
    assert len(ptrs) == 6


def test_runner_fixture_has_different_lists():
    """The moving, straining batch of the GPU runner tests: its steps have different neighbour lists, none with a pair on the
    cutoff (float32 and float64 distances give the same list)."""
    Z, N, pbc, steps = D.moving_system()
    sizes = []
    for R, cell in steps:
        ref = P.brute_force_fast(R, N, cell, pbc, P.CUTOFF)
        assert P.cutoff_margin_ok(R.astype(np.float64), N, cell.astype(np.float64), pbc)
        sizes.append((len(ref["id_c"]), len(ref["id3_reduce_ca"])))
    assert sizes[0] != sizes[1] and len(steps) == 3
