"""Molecular batches with changing molecule SIZES whose lists are built inside the replay (no GPU): the capacity builder's
`set_layout` (checks, shapes, the arrays it writes against `padded.capacity_layout` and the prefix sums of N^2), what
`attach_builder` accepts and refuses, the host checks of `run_positions`, the routing of `Trainer.enable_padded_eval`, and the
declarations of the new entry points.  Stream: tests/mol_ragged_common.py."""
import os
import re

import numpy as np
import pytest
import torch

import cpu_kernels
import mol_ragged_common as G
import pbc_common as P
import pbc_train_common as PT
from conftest import ROOT
from gemnet_pytorch_amd.index_device import DeviceCapacityGraphBuilder
from gemnet_pytorch_amd.padded import PaddedGraphRunner, capacity_layout, pad_indices
from gemnet_pytorch_amd.training.metrics import Metrics
from gemnet_pytorch_amd.training.trainer import Trainer
from test_model_cpu import build


class _M:       # the runner only looks at these attributes before a capture
    triplets_only, direct_forces = True, False


class _Q:
    triplets_only, direct_forces = False, False


def _builder(n_mol=G.N_MOL, a_cap=G.A_CAP, n_max=G.N_MAX):
    return DeviceCapacityGraphBuilder(n_mol, a_cap, n_max, G.CUTOFF, device="cpu")


def _sq_off(N):
    return [0] + list(np.cumsum(np.asarray(N, np.int64) ** 2))


# ---------------------------------------------------------------------------------------------------------------- the builder
def test_builder_shapes_and_constructor_checks():
    b = _builder()
    assert (b.B, b.a_cap, b.n_max, b.triplets_only) == (G.N_MOL, G.A_CAP, G.N_MAX, True)
    assert b.mol_off.shape == (G.N_MOL + 2,) and b.sq_off.shape == (G.N_MOL + 1,) and b.atom_mol.shape == (G.A_CAP,)
    assert b.N32.shape == (G.N_MOL,) and b.n_atoms.shape == (1,)
    assert all(t.dtype == torch.int32 for t in (b.mol_off, b.sq_off, b.atom_mol, b.N32, b.n_atoms))
    assert bool((b.atom_mol == G.N_MOL).all()) and not b.mol_off.any()         # before a layout: fillers only, empty molecules
    with pytest.raises(NotImplementedError, match="GemNet-Q"):
        DeviceCapacityGraphBuilder(G.N_MOL, G.A_CAP, G.N_MAX, G.CUTOFF, triplets_only=False, device="cpu")
    for n_mol, a_cap, n_max in ((0, 8, 4), (9, 8, 4), (2, 8, 0), (2, 8, 9)):
        with pytest.raises(ValueError):
            DeviceCapacityGraphBuilder(n_mol, a_cap, n_max, G.CUTOFF, device="cpu")
    with pytest.raises(ValueError, match="int32"):             # the adjacency blocks: a_cap * n_max bytes
        DeviceCapacityGraphBuilder(4, 1 << 16, 1 << 15, G.CUTOFF, device="cpu")


@pytest.mark.parametrize("N,a_cap,n_max", [([3, 1, 5, 2], 72, 66), ([66, 1, 3, 2], 72, 66), ([1], 1, 1), ([2, 1, 5], 9, 5),
                                           ([1] * 7, 30, 3)])
@pytest.mark.parametrize("as_tensor", [False, True])
def test_set_layout_writes_capacity_layout_and_the_prefix_sums_of_squares(N, a_cap, n_max, as_tensor):
    n_mol, A = len(N), sum(N)
    b = DeviceCapacityGraphBuilder(n_mol, a_cap, n_max, G.CUTOFF, device="cpu")
    assert b.set_layout(torch.tensor(N) if as_tensor else N) is b
    lay = capacity_layout(torch.tensor(N), n_mol, a_cap, a_cap)
    assert torch.equal(b.mol_off, lay["mol_off"]) and b.mol_off.tolist() == [0] + list(np.cumsum(N)) + [a_cap]
    assert torch.equal(b.atom_mol, lay["atom_mol"])
    assert b.sq_off.tolist() == _sq_off(N) and b.sq_off[-1] <= a_cap * n_max
    assert b.N32.tolist() == N and b.n_atoms.tolist() == [A] and b.A == A


def test_set_layout_checks():
    b = _builder()
    b.set_layout([3, 1, 5, 2])
    kept = (b.mol_off.clone(), b.sq_off.clone(), b.atom_mol.clone())
    with pytest.raises(ValueError, match=f"N must hold {G.N_MOL} molecule sizes"):
        b.set_layout([3, 1, 5])
    for bad, kw in (([3, 0, 5, 2], {}), ([67, 1, 1, 1], {}), ([66, 3, 3, 1], {}), ([3, 1, 5, 2], dict(n_atoms=12))):
        with pytest.raises(ValueError, match="do not fit"):
            b.set_layout(bad, **kw)
        assert all(torch.equal(a, k) for a, k in zip((b.mol_off, b.sq_off, b.atom_mol), kept)), bad
    # arrays=False leaves the three arrays to the layout kernel — which is the one that judges such sizes
    b.set_layout([67, 1, 1, 1], n_atoms=70, arrays=False)
    assert b.N32.tolist() == [67, 1, 1, 1] and b.n_atoms.tolist() == [70] and b.A == 70
    assert all(torch.equal(a, k) for a, k in zip((b.mol_off, b.sq_off, b.atom_mol), kept))
    # the host-sized build refuses positions for another layout before it touches a device
    b.set_layout([3, 1, 5, 2])
    with pytest.raises(ValueError, match="set_layout"):
        b(torch.zeros(10, 3))


# ----------------------------------------------------------------------------------------------------------------- the runner
def _runner(model=None, a_cap=G.A_CAP, **kw):
    e_cap, t_cap, deg, groups = G.CAPS
    R, Z, N, idx = G.tensors(G.stream()[0], "cpu")
    run = PaddedGraphRunner(model or _M(), Z, N, e_cap, t_cap, max_in_degree=deg, n_groups=groups, a_cap=a_cap, **kw)
    return run, (R, Z, N, idx)


def test_attach_builder_accepts_the_capacity_builder_on_a_molecular_runner_with_a_cap():
    run, (R, Z, N, idx) = _runner()
    with pytest.raises(RuntimeError, match="attach_builder"):
        run.attach_builder(_builder())                          # the buffers hold no batch yet
    run._fill(R, idx, Z, N)
    b = _builder()
    run.attach_builder(b)
    assert run.builder is b and run.graph is None
    assert b.N32.tolist() == G.stream()[0]["N"] and b.n_atoms.tolist() == [11]      # the batch the buffers hold
    assert run._staging.numel() == 4 * run.e_cap + 2 * run.t_cap and run._idx_state.numel() == 8
    assert run.index_error() == 0 and run.index_sizes() == (0, 0)
    # the fill of a later batch hands its sizes to the builder as well
    R2, Z2, N2, idx2 = G.tensors(G.stream()[2], "cpu")
    run._fill(R2, idx2, Z2, N2)
    assert b.N32.tolist() == G.stream()[2]["N"] and b.n_atoms.tolist() == [72]
    want = pad_indices(idx2, run.a_cap, run.e_cap, run.t_cap, run.G)
    assert all(torch.equal(run.padded_inputs()[k].long(), want[k]) for k in G.IDX_KEYS)


def test_attach_builder_refusals():
    e_cap, t_cap, deg, groups = G.CAPS
    R, Z, N, idx = G.tensors(G.stream()[0], "cpu")
    fixed = PaddedGraphRunner(_M(), Z, N, e_cap, t_cap, max_in_degree=deg, n_groups=groups)
    periodic = PaddedGraphRunner(_M(), Z, N, e_cap, t_cap, max_in_degree=deg, n_groups=groups, cell=torch.eye(3).repeat(4, 1, 1))
    quad = PaddedGraphRunner(_Q(), Z, N, e_cap, t_cap, max_in_degree=deg, n_groups=groups, a_cap=G.A_CAP, quad_caps=(8, 8, 8))
    for run in (fixed, periodic, quad):
        with pytest.raises(ValueError, match="different systems"):
            run.attach_builder(_builder())
    run, _ = _runner()
    run._fill(R, idx, Z, N)
    for other in (_builder(n_mol=3), _builder(a_cap=G.A_CAP + 1)):
        with pytest.raises(ValueError, match="different systems"):
            run.attach_builder(other)
    # every other object: today's refusal, word for word
    with pytest.raises(NotImplementedError) as err:
        run.attach_builder(object())
    assert str(err.value) == "the in-graph index build needs a fixed molecule layout (no a_cap)"
    assert run.builder is None


def test_host_checks_of_run_positions_come_before_any_copy():
    run, (R, Z, N, idx) = _runner()
    with pytest.raises(RuntimeError, match="attach_builder"):
        run.run_positions(R, Z=Z, N=N)
    run._fill(R, idx, Z, N)
    b = _builder()
    run.attach_builder(b)
    kept = {k: v.clone() for k, v in run.padded_inputs().items()}
    sizes = (b.N32.clone(), b.n_atoms.clone())
    R2, Z2, N2, _ = G.tensors(G.stream()[2], "cpu")
    big_R, big_Z = torch.cat([R2, R2[:1] + 0.5]), torch.cat([Z2, Z2[:1]])
    with pytest.raises(ValueError, match=f"exceeds a_cap = {G.A_CAP}"):
        run.run_positions(big_R, Z=big_Z, N=N2 + torch.tensor([0, 1, 0, 0]))
    with pytest.raises(ValueError, match="changes the number of molecules"):
        run.run_positions(R2, Z=Z2, N=N2[:3])
    with pytest.raises(ValueError, match="the number of atoms changed"):
        run.run_positions(R2)
    with pytest.raises(ValueError, match="Z must hold"):
        run.run_positions(R2, Z=Z2[:5], N=N2)
    with pytest.raises(TypeError, match="positions must be"):
        run.run_positions(R2.double(), Z=Z2, N=N2)
    with pytest.raises(ValueError, match="without a cell"):
        run.run_positions(R2, Z=Z2, N=N2, cell=torch.eye(3).repeat(4, 1, 1))
    with pytest.raises(ValueError, match="periodic runner"):
        run.run_positions(R2, Z=Z2, N=N2, pbc=[True, True, True])
    assert all(torch.equal(v, kept[k]) for k, v in run.padded_inputs().items()) and run.A == 11
    assert torch.equal(b.N32, sizes[0]) and torch.equal(b.n_atoms, sizes[1])


# ---------------------------------------------------------------------------------------------------------------- the Trainer
def _batch(b):
    from gemnet_pytorch_amd.training.data_container import build_indices
    idx = build_indices(b["R"], np.array(b["N"]), G.CUTOFF, G.CUTOFF, True)
    inputs = {k: torch.tensor(v) for k, v in idx.items()}
    inputs.update(R=torch.tensor(b["R"]).double(), Z=torch.tensor(b["Z"]), N=torch.tensor(b["N"]))
    Et, Ft = G.targets(b)
    return inputs, {"E": torch.tensor(Et), "F": torch.tensor(Ft)}


def test_enable_padded_eval_routes_what_does_not_fit_to_the_plain_path():
    """On the host emulation of the launchers (float64).  None of these batches may take the graph: too many atoms, a molecule
    above n_max, another number of molecules, a quadruplet / direct-force / mve trainer — the metrics are those of the plain
    path and no runner is built."""
    e_cap, t_cap, deg, groups = G.CAPS
    stream = G.stream()
    with cpu_kernels.emulate():
        model = build(P.CFG, PT.make_params(P.CFG)).eval()
        plain, routed = Trainer(model), Trainer(model)
        for t in (plain, routed):
            t.dict2device = lambda d, device=None: d                # float64 CPU emulation
        assert routed._eval_caps is None
        for caps, s in ((dict(a_cap=71, n_max=66), 2), (dict(a_cap=72, n_max=65), 2), (dict(a_cap=72, n_max=66, n_mol=5), 0)):
            routed.enable_padded_eval(e_cap=e_cap, t_cap=t_cap, max_in_degree=deg, n_groups=groups, **caps)
            m0, m1 = Metrics("val", plain.tracked_metrics), Metrics("val", routed.tracked_metrics)
            l0 = plain.test_on_batch(iter([_batch(stream[s])]), m0)
            l1 = routed.test_on_batch(iter([_batch(stream[s])]), m1)
            assert float(l0) == float(l1) and m0.result() == m1.result() and routed._erun is None, caps
            (E1, F1), _ = routed.eval_on_batch(iter([_batch(stream[s])]))
            (E0, F0), _ = plain.eval_on_batch(iter([_batch(stream[s])]))
            assert torch.equal(E0, E1) and torch.equal(F0, F1) and routed._erun is None
            E1, _, F1, _ = routed.predict_on_batch(iter([_batch(stream[s])]))
            assert torch.equal(E0, E1) and torch.equal(F0, F1) and routed._erun is None
        routed.enable_padded_eval(a_cap=72, e_cap=e_cap, t_cap=t_cap, max_in_degree=deg, n_max=66, n_groups=groups)
        inputs, _ = _batch(stream[0])
        n_host = inputs["N"]
        assert routed._eval_fits(inputs, n_host)                    # this one would take the graph ...
        assert not routed._eval_fits(inputs, None)                  # ... but not without its sizes,
        assert not routed._eval_fits(dict(inputs, Z=inputs["Z"][:-1]), n_host)     # with sizes that do not add up,
        for attr, val in (("triplets_only", False), ("direct_forces", True)):      # or for a family the runner does not serve
            saved = getattr(model, attr)
            setattr(model, attr, val)
            assert not routed._eval_fits(inputs, n_host)
            setattr(model, attr, saved)
        routed.mve = True
        assert not routed._eval_fits(inputs, n_host)
        routed.mve = False
        # the evaluation graph is per-process execution state, never part of a checkpoint
        state = routed.state_dict()
        assert not {"_eval_caps", "_erun", "_erun_key"} & set(state)
        routed.load_state_dict(dict(_eval_caps=None, _erun="stale"))
        assert routed._eval_caps is not None and routed._erun is None


# ------------------------------------------------------------------------------------------------------------ declarations
def test_new_symbols_are_declared_and_bound():
    from gemnet_pytorch_amd import _lib, hbcheck, kernels
    text = open(os.path.join(ROOT, "include", "gemnet_hip.h")).read()
    for name in ("gn_index_gpu_layout", "gn_index_gpu_padded_tv"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
    funcs, _ = hbcheck.parse_header()
    lay, pbc_lay = funcs["gn_index_gpu_layout"], funcs["gn_pbc_layout"]
    tv, t = funcs["gn_index_gpu_padded_tv"], funcs["gn_index_gpu_padded_t"]
    assert len(lay) == len(_lib.SIGNATURES["gn_index_gpu_layout"]) == len(pbc_lay) + 2          # + n_max, sq_off
    assert len(tv) == len(_lib.SIGNATURES["gn_index_gpu_padded_tv"]) == len(t) - 1              # + atom_mol; (B, A, sum_n2) -> n_mol
    kinds = dict(lay)
    assert all(kinds[k] == "r" for k in ("N", "n_atoms"))
    assert all(kinds[k] == "w" for k in ("mol_off", "sq_off", "atom_mol", "batch_seg", "N_pad", "mask", "state"))
    kinds = dict(tv)
    assert all(kinds[k] == "r" for k in ("R", "mol_off", "sq_off", "atom_mol"))
    assert all(kinds[k] == "w" for k in ("ws", "staging", "id_c", "id_a", "id_swap", "id_undir", "id3_reduce_ca", "id3_expand_ba",
                                         "state"))
    assert lay[-1] == tv[-1] == ("stream", "stream")
    # the fixed-layout entries keep their signatures
    assert [n for n, _ in t][:8] == ["R", "r_is_f64", "mol_off", "sq_off", "B", "A", "nmax", "sum_n2"]
    assert len(pbc_lay) == 12
    assert callable(kernels.index_layout) and callable(kernels.index_padded_tv) and callable(kernels.index_cap_ws_bytes)
    src = open(os.path.join(ROOT, "gemnet_pytorch_amd", "csrc", "index_gpu.hip")).read()
    assert 'extern "C" int gn_index_gpu_layout' in src and 'extern "C" int gn_index_gpu_padded_tv' in src
    # the workspace of the capacity shapes: the triplets-only workspace with the adjacency blocks at their upper bound
    lib = _lib.load()
    assert kernels.index_cap_ws_bytes(72, 66) == lib.gn_index_gpu_ws_bytes(72, 72 * 66, 1) >= lib.gn_index_gpu_ws_bytes(72, 66 * 66 + 14, 1)
    with pytest.raises(ValueError, match="int32"):
        kernels.index_cap_ws_bytes(1 << 16, 1 << 15)
    assert "gn_abi_version() == 16" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
