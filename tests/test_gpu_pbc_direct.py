"""GPU: direct-force GemNet-T on periodic structures (GemNet.periodic_direct_forces) — the force-head kernel against its fp64
restatement under a derived bound, the model against the cluster oracle and its invariances, the runners bit for bit against
the eager call, the captured step under the happens-before checker, and the switch with what it still refuses."""
import numpy as np
import pytest
import torch

import pbc_common as P
import pbc_direct_common as D
from conftest import SCALE_FILE
from oracle import gemnet_oracle as GO
from redzone import put, redzone_on_request  # noqa: F401  (the kernel-level tests below ask for `redzone`: they run under the red-zone harness)

pytestmark = pytest.mark.gpu
DEV = D.DEV


# ---------------------------------------------------------------------------------------------------------------- kernel
def _kernel_inputs(name, K_, T, seed=0):
    from gemnet_pytorch_amd import kernels as K
    idx, V, A = D.kernel_case(name)
    terms = np.random.RandomState(seed).standard_normal((K_, len(V), T)).astype(np.float32)
    dev = lambda x, dt: put(torch.tensor(np.ascontiguousarray(x), dtype=dt))
    id_a = dev(idx["id_a"], torch.int32)
    perm, seg = K.csr_build(id_a, A)
    return idx, V, A, terms, dev(terms, torch.float32), dev(V, torch.float32), dev(idx["id_swap"], torch.int32), perm, seg


def _launch(terms, V, swap, perm, seg, A):
    from gemnet_pytorch_amd import kernels as K
    F = torch.full((A, terms.shape[2], 3), float("nan"), device=DEV)
    K.direct_force(terms, V, swap, perm, seg, A, out=F)
    torch.cuda.synchronize()
    return F


CASES = [(n, c, k, t) for n in ("sc1", "sc08", "zoo") for c in (False, True) for k in (1, 5) for t in (1, 3)]


@pytest.mark.parametrize("name,coupled,K_,T", CASES)
def test_kernel_matches_fp64_reference(name, coupled, K_, T, redzone):
    idx, Vh, A, th, terms, V, swap, perm, seg = _kernel_inputs(name, K_, T)
    sw_h = idx["id_swap"] if coupled else None
    F = _launch(terms, V, swap if coupled else None, perm, seg, A)
    ref = D.direct_force_ref(th, Vh, sw_h, idx["id_a"], A)
    bound = D.error_bound(th, sw_h, idx["id_a"], A)
    Fh = F.double().cpu().numpy()
    err = np.abs(Fh - ref).max(-1)
    print(name, coupled, K_, T, "max err / bound", float((err / np.maximum(bound, 1e-300)).max()), "max |F|", np.abs(ref).max())
    assert np.isfinite(Fh).all()                                    # no NaN of the prefill is left: every row was written
    assert (err <= bound).all()
    empty = np.bincount(idx["id_a"], minlength=A) == 0
    assert (Fh[empty] == 0).all() and (name != "zoo" or empty.sum() == 25)
    assert torch.equal(F, _launch(terms, V, swap if coupled else None, perm, seg, A))       # bit-reproducible
    if A == 1:      # edges sorted by target atom: the CSR without a permutation sums in the same order
        seg1 = torch.tensor([0, len(Vh)], dtype=torch.int32, device=DEV)
        assert torch.equal(F, _launch(terms, V, swap if coupled else None, None, seg1, A))


@pytest.mark.parametrize("name,coupled,K_,T", CASES)
def test_kernel_rows_unchanged_by_pad_edges_of_dummy_atoms(name, coupled, K_, T, redzone):
    """Pad edges that end in additional dummy atoms (the layout of padded.py), the CSR extended: every original row keeps its
    bits."""
    from gemnet_pytorch_amd import kernels as K
    idx, Vh, A, th, terms, V, swap, perm, seg = _kernel_inputs(name, K_, T)
    F = _launch(terms, V, swap if coupled else None, perm, seg, A)
    E, ep, Ad = len(Vh), 10, 3
    rs = np.random.RandomState(1)
    k = np.arange(ep)
    id_a2 = put(torch.tensor(np.concatenate([idx["id_a"], A + (k // 2) % Ad]), dtype=torch.int32))
    swap2 = put(torch.tensor(np.concatenate([idx["id_swap"], E + (k ^ 1)]), dtype=torch.int32))
    V2 = put(torch.cat([V, torch.tensor(rs.uniform(0.5, 1.5, (ep, 3)), dtype=torch.float32, device=DEV)]))
    terms2 = put(torch.cat([terms, torch.tensor(rs.standard_normal((K_, ep, T)), dtype=torch.float32, device=DEV)], dim=1))
    perm2, seg2 = K.csr_build(id_a2, A + Ad)
    F2 = _launch(terms2, V2, swap2 if coupled else None, perm2, seg2, A + Ad)
    assert torch.equal(F2[:A], F) and bool(torch.isfinite(F2).all()) and bool((F2[A:] != 0).any())


# ----------------------------------------------------------------------------------------------------------------- model
@pytest.mark.parametrize("coupled", [False, True])
@pytest.mark.parametrize("kind", ["small", "triclinic", "slab"])
def test_energy_and_forces_match_cluster_oracle(kind, coupled):
    model = D.direct_model(coupled)
    E, F = D.run(model, [P.structure(kind)])
    E_ref, F_ref = D.cluster_reference(kind, coupled)
    assert F.shape == F_ref.shape == (3, 1, 3)
    scale = max(1.0, float(np.abs(F_ref).mean()))
    print(kind, coupled, E[0, 0], E_ref, np.abs(F - F_ref).mean(), np.abs(F - F_ref).max(), np.abs(F_ref).mean())
    assert abs(E[0, 0] - E_ref) <= 2e-5 * max(1.0, abs(E_ref))
    assert np.abs(F - F_ref).mean() <= 1e-5 * scale and np.abs(F - F_ref).max() <= 1e-4 * scale


def test_coupled_forces_conserve_momentum_and_batches_equal_single_runs():
    model = D.direct_model(True)
    structs = [P.structure(k, seed=i) for i, k in enumerate(["small", "triclinic", "slab"])]
    E, F = D.run(model, structs)
    off = 0
    for b, s in enumerate(structs):
        e, f = D.run(model, [s])
        n = len(s[0])
        assert abs(E[b, 0] - e[0, 0]) <= 1e-5 * max(1.0, abs(e[0, 0]))
        assert np.abs(F[off:off + n] - f).max() <= 1e-5 * max(1.0, np.abs(f).max())
        if s[3].all():      # fully periodic: every edge has its partner inside the structure
            assert np.abs(f.sum(0)).max() <= 5e-5 * max(1.0, np.abs(f).max())
            assert np.abs(F[off:off + n].sum(0)).max() <= 5e-5 * max(1.0, np.abs(F).max())
        off += n


@pytest.mark.parametrize("coupled", [False, True])
def test_invariances(coupled):
    model = D.direct_model(coupled)
    R, Z, cell, pbc = P.structure("triclinic")
    E, F = D.run(model, [(R, Z, cell, pbc)])
    tolE, tolF = 2e-5 * max(1.0, abs(E[0, 0])), 5e-5 * max(1.0, np.abs(F).max())
    R2 = R.copy()
    R2[2] += cell[1] - cell[0]
    for Rx in (R2, R + np.array([0.41, -0.73, 1.3])):      # an atom moved by a lattice vector, the whole cell translated
        e, f = D.run(model, [(Rx, Z, cell, pbc)])
        assert abs(e[0, 0] - E[0, 0]) <= tolE and np.abs(f - F).max() <= tolF
    shifts = [np.array(n) @ cell for n in np.ndindex(2, 2, 2)]      # 2x2x2 supercell: E x 8, tiled forces
    e, f = D.run(model, [(np.concatenate([R + t for t in shifts]), np.tile(Z, 8), 2 * cell, pbc)])
    assert abs(e[0, 0] - 8 * E[0, 0]) <= 8 * tolE
    assert np.abs(f - np.tile(F, (8, 1, 1))).max() <= tolF


@pytest.mark.parametrize("coupled", [False, True])
def test_large_cell_equals_the_molecular_direct_force_model(coupled):
    """No image within the cutoff: the same model on the molecular path (other launches: not bitwise)."""
    from gemnet_pytorch_amd.index_device import build_indices_device
    model = D.direct_model(coupled)
    R, Z, _, _ = P.structure("small")
    E1, F1 = D.run(model, [(R, Z, np.eye(3) * 30.0, np.array([True] * 3))])
    Rd = torch.tensor(R, dtype=torch.float32, device=DEV)
    mol = build_indices_device(Rd, np.array([3]), P.CUTOFF, 10.0, True)
    E0, F0 = model(dict(R=Rd, Z=torch.tensor(Z, device=DEV).long(), N=torch.tensor([3], device=DEV), **mol))
    E0, F0 = E0.detach().double().cpu().numpy(), F0.detach().double().cpu().numpy()
    assert F0.shape == F1.shape == (3, 1, 3)
    assert abs(E1[0, 0] - E0[0, 0]) <= 2e-5 * max(1.0, abs(E0[0, 0]))
    assert np.abs(F1 - F0).max() <= 5e-5 * max(1.0, np.abs(F0).max())


# --------------------------------------------------------------------------------------------------------------- runners
def test_force_graphs_replay_is_the_eager_call():
    from gemnet_pytorch_amd.runtime import ForceGraphs
    model = D.direct_model(True)
    batch = D.device_batch([P.structure(k, seed=i) for i, k in enumerate(["small", "triclinic"])])
    fg = ForceGraphs(model, [batch])
    g = torch.Generator(device=DEV).manual_seed(0)
    R2 = batch["R"] + 0.01 * torch.randn(batch["R"].shape, device=DEV, generator=g)
    cell2 = batch["cell"] @ (torch.eye(3, device=DEV) + 0.002 * torch.randn(3, 3, device=DEV, generator=g))
    fg.set_positions(0, R2)
    fg.set_cell(0, cell2)
    fg.replay()
    torch.cuda.synchronize()
    E, F = fg.energies_forces()
    ref = dict(batch, R=R2.clone(), cell=cell2.clone())
    ref.pop("_plan", None)
    E0, F0 = model(ref)
    torch.cuda.synchronize()
    assert F.shape == (6, 1, 3) and torch.equal(E, E0) and torch.equal(F, F0)
    with pytest.raises(ValueError, match="no stress"):
        fg.stress()


def _system():
    Z, N, pbc, steps = D.moving_system()
    return (torch.tensor(Z, device=DEV).long(), torch.tensor(N, device=DEV), N, pbc,
            [(torch.tensor(R, device=DEV), torch.tensor(c, device=DEV)) for R, c in steps])


def _eager(model, builder, Z, N, R, cell):
    idx = builder(R, cell, dtype=torch.int32)
    E, F = model(dict(Z=Z, N=N, R=R.clone(), cell=cell.clone(), **idx))
    torch.cuda.synchronize()
    return (E.clone(), F.clone()), idx


def _padded_runner(model, Z, N, pbc, lists, cell):
    from gemnet_pytorch_amd.padded import PaddedGraphRunner
    sizes = [PaddedGraphRunner.sizes_of(i) for i in lists]
    deg = max(PaddedGraphRunner.in_degree_of(i) for i in lists) + 2
    e_cap = int(max(s[0] for s in sizes) * 1.3) // 4 * 4 + 8
    t_cap = int(max(s[1] for s in sizes) * 1.3) // 2 * 2 + 2
    pad = e_cap - int(min(s[0] for s in sizes) * 0.8)
    n_groups = max(1, -(-(-(-pad // 4)) // max(deg // 2, 1)))
    return PaddedGraphRunner(model, Z, N, e_cap, t_cap, max_in_degree=deg, n_groups=n_groups, cell=cell, pbc=pbc)


@pytest.mark.parametrize("coupled", [False, True])
def test_padded_runner_equals_eager_on_the_unpadded_batch(coupled):
    """Eager fill with two different lists, then the list built inside the graph (attach_builder + run_positions), the captured
    step under the happens-before checker."""
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder
    model = D.direct_model(coupled)
    Z, N, Nh, pbc, steps = _system()
    builder = PeriodicGraphBuilder(Nh, P.CUTOFF, pbc=pbc, device=DEV)
    refs = [_eager(model, builder, Z, N, R, cell) for R, cell in steps]
    assert len({tuple(i["id_c"].shape) for _, i in refs}) + len({tuple(i["id3_reduce_ca"].shape) for _, i in refs}) >= 3
    run = _padded_runner(model, Z, N, pbc, [i for _, i in refs], steps[0][1])
    for (R, cell), ((E0, F0), idx) in zip(steps[:2], refs[:2]):
        E, F = run(R, idx, cell=cell)
        torch.cuda.synchronize()
        assert F.shape == F0.shape == (int(Z.shape[0]), 1, 3)
        assert torch.equal(E, E0) and torch.equal(F, F0)
    with pytest.raises(ValueError, match="no stress"):
        run.stress()
    run.attach_builder(builder)
    run.check = True
    for (R, cell), ((E0, F0), idx) in zip(steps, refs):
        E, F = run.run_positions(R, cell=cell)
        torch.cuda.synchronize()
        assert run.index_error() == 0 and run.index_sizes() == (idx["id_c"].shape[0], idx["id3_reduce_ca"].shape[0])
        assert torch.equal(E, E0) and torch.equal(F, F0)
    races, summary = run.hb.races(), run.hb.summary()
    print(run.hb.format(races))
    assert not races and summary["unrecorded_nodes"] == 0 and summary["unresolved_pointers"] == 0, summary
    assert not run.flag.tripped()


def test_padded_runner_poisons_a_step_that_outgrows_its_capacities():
    """Capacities that hold the first list only: a step with more edges returns NaN and reports, as for the autograd model."""
    from gemnet_pytorch_amd.padded import PaddedGraphRunner
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder
    model = D.direct_model(True)
    R0, Zh, cell, pbc = P.structure("small")
    Z, N = torch.tensor(Zh, device=DEV).long(), torch.tensor([3], device=DEV)
    builder = PeriodicGraphBuilder([3], P.CUTOFF, pbc=pbc[None], device=DEV)
    R = torch.tensor(R0, dtype=torch.float32, device=DEV)
    c0 = torch.tensor(cell[None], dtype=torch.float32, device=DEV)
    idx = builder(R, c0, dtype=torch.int32)
    E0, T0 = PaddedGraphRunner.sizes_of(idx)
    deg = PaddedGraphRunner.in_degree_of(idx) + 2
    run = PaddedGraphRunner(model, Z, N, E0 + 4, T0 + 2, max_in_degree=deg, n_groups=2, cell=c0, pbc=pbc[None])
    run._fill(R, idx, cell=c0)
    run.attach_builder(builder)
    E, F = run.run_positions(R)
    torch.cuda.synchronize()
    assert run.index_error() == 0 and bool(torch.isfinite(F).all())
    small = c0 * 0.8                     # a denser cell: more edges than e_cap
    assert builder(R * 0.8, small, dtype=torch.int32)["id_c"].shape[0] > run.e_cap
    E, F = run.run_positions(R * 0.8, cell=small)
    torch.cuda.synchronize()
    assert run.index_error() & 1 and bool(torch.isnan(E).all()) and bool(torch.isnan(F).all())


def test_dynamic_force_field_steps_equal_eager():
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder
    from gemnet_pytorch_amd.runtime import DynamicForceField
    model = D.direct_model(True)
    Z, N, Nh, pbc, steps = _system()
    builder = PeriodicGraphBuilder(Nh, P.CUTOFF, pbc=pbc, device=DEV)
    ff = DynamicForceField(model, Z, Nh, P.CUTOFF, 10.0, margin=0.4, cell=steps[0][1], pbc=pbc)
    for s, (R, cell) in enumerate(steps):
        (E0, F0), _ = _eager(model, builder, Z, N, R, cell)
        E, F = ff(R, cell=cell) if s != 2 else ff(R)          # (the last step keeps the cell of the one before)
        torch.cuda.synchronize()
        assert torch.equal(E, E0) and torch.equal(F, F0), s
        assert not ff.index_failed()
    assert ff.recaptures == 0 and ff.runner.builder is not None
    # exact=False: nothing waits; the same values once the caller has waited
    E, F = ff(steps[1][0], cell=steps[1][1], exact=False)
    torch.cuda.synchronize()
    (E0, F0), _ = _eager(model, builder, Z, N, *steps[1])
    assert torch.equal(E, E0) and torch.equal(F, F0) and not ff.index_failed()
    with pytest.raises(ValueError, match="no stress"):
        ff.stress()


def test_dynamic_force_field_resizes_when_the_list_outgrows_it():
    """A denser step than the capacities hold: exact=True re-sizes, captures anew and returns the eager result."""
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder
    from gemnet_pytorch_amd.runtime import DynamicForceField
    model = D.direct_model(True)
    R0, Zh, cell, pbc = P.structure("small")
    Z, N = torch.tensor(Zh, device=DEV).long(), torch.tensor([3], device=DEV)
    builder = PeriodicGraphBuilder([3], P.CUTOFF, pbc=pbc[None], device=DEV)
    R = torch.tensor(R0, dtype=torch.float32, device=DEV)
    c0 = torch.tensor(cell[None], dtype=torch.float32, device=DEV)
    ff = DynamicForceField(model, Z, [3], P.CUTOFF, 10.0, cell=c0, pbc=pbc[None])
    for f in (1.0, 0.8):                 # 12 edges / 36 triplets, then 30 / 272
        (E0, F0), _ = _eager(model, builder, Z, N, R * f, c0 * f)
        E, F = ff(R * f, cell=c0 * f)
        torch.cuda.synchronize()
        assert torch.equal(E, E0) and torch.equal(F, F0), f
    assert ff.recaptures == 1 and not ff.index_failed()


def test_device_molecule_predict():
    from gemnet_pytorch_amd.md import DeviceMolecule
    model = D.direct_model(True)
    R, Z, cell, pbc = P.structure("triclinic")
    mol = DeviceMolecule(R, Z, P.CUTOFF, 10.0, triplets_only=True, cell=cell, pbc=pbc)
    mol.to(DEV)
    E, F = model.predict(mol.get())
    e, f = D.run(model, [(R, Z, cell, pbc)])
    assert F.shape == (3, 1, 3)
    assert np.allclose(E.double().numpy(), e, atol=1e-6) and np.allclose(F.double().numpy(), f, atol=1e-6)
    with pytest.raises(ValueError, match="no stress"):
        model.predict(mol.get(), stress=True)
    assert not model.training


# ---------------------------------------------------------------------------------------------------- switch and refusals
def test_switch_and_refusals():
    batch = D.device_batch([P.structure("small")])
    with pytest.raises(NotImplementedError, match="not direct_forces"):
        D.direct_model(False, switch=False)(dict(batch))                       # the default: as before
    model = D.direct_model(False)
    E, F = model(dict(batch))
    assert F.shape == (3, 1, 3) and not F.requires_grad and not E.requires_grad
    with pytest.raises(NotImplementedError, match="no stress"):
        model(dict(batch), stress=True)
    with pytest.raises(NotImplementedError, match="inference only"):
        model.train()(dict(batch))
    model.eval()
    with pytest.raises(NotImplementedError, match="GemNet-Q"):
        D.direct_model(False, triplets_only=False)(dict(batch))
    with pytest.raises(NotImplementedError, match="one target"):
        D.direct_model(False, num_targets=2)(dict(batch))
    with pytest.raises(NotImplementedError, match="autograd graph"):
        model(dict(batch, R=batch["R"].clone().requires_grad_(True)))


def test_autograd_force_model_does_not_depend_on_the_switch():
    from gemnet_pytorch_amd.model.gemnet import GemNet
    params = P.make_params()
    m = GemNet(**P.CFG, scale_file=SCALE_FILE)
    m.load_state_dict(GO.expand_to_reference_state_dict({k: v.float() for k, v in params.items()}))
    m = m.to(DEV).eval()
    assert m.periodic_direct_forces is False
    batch = D.device_batch([P.structure("small"), P.structure("slab")])
    a = m(dict(batch), stress=True)
    m.periodic_direct_forces = True
    b = m(dict(batch), stress=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
