"""GemNet-Q on molecular batches with changing molecule SIZES, lists built inside the replay (no GPU): the quadruplet capacity
builder's shapes and constructor checks, what `attach_builder` accepts and refuses, the host checks of `run_positions`, the routing
of `Trainer.enable_padded_eval(quad_caps=)` and the declaration of the new entry point.  Stream: tests/mol_ragged_q_common.py."""
import os
import re

import pytest
import torch

import cpu_kernels
import mol_ragged_q_common as GQ
import pbc_q_common as Q
from conftest import ROOT
from gemnet_pytorch_amd.index_device import DeviceCapacityGraphBuilder, DeviceCapacityQuadGraphBuilder
from gemnet_pytorch_amd.padded import PaddedGraphRunner, pad_indices
from gemnet_pytorch_amd.training.metrics import Metrics
from gemnet_pytorch_amd.training.trainer import Trainer
from test_model_cpu import build

CFG = dict(Q.CFG_Q, int_cutoff=GQ.INT_CUTOFF)


class _M:       # the runner only looks at these attributes before a capture
    triplets_only, direct_forces = True, False


class _Q:
    triplets_only, direct_forces = False, False


def _builder(n_mol=GQ.N_MOL, a_cap=GQ.A_CAP, n_max=GQ.N_MAX):
    return DeviceCapacityQuadGraphBuilder(n_mol, a_cap, n_max, GQ.CUTOFF, GQ.INT_CUTOFF, device="cpu")


# ---------------------------------------------------------------------------------------------------------------- the builder
def test_builder_shapes_and_constructor_checks():
    b = _builder()
    assert isinstance(b, DeviceCapacityGraphBuilder)
    assert (b.B, b.a_cap, b.n_max, b.triplets_only) == (GQ.N_MOL, GQ.A_CAP, GQ.N_MAX, False)
    assert (b.cutoff, b.int_cutoff) == (GQ.CUTOFF, GQ.INT_CUTOFF)
    assert b.mol_off.shape == (GQ.N_MOL + 2,) and b.sq_off.shape == (GQ.N_MOL + 1,) and b.atom_mol.shape == (GQ.A_CAP,)
    assert b.N32.shape == (GQ.N_MOL,) and b.n_atoms.shape == (1,)
    assert all(t.dtype == torch.int32 for t in (b.mol_off, b.sq_off, b.atom_mol, b.N32, b.n_atoms))
    assert bool((b.atom_mol == GQ.N_MOL).all()) and not b.mol_off.any()        # before a layout: fillers only, empty molecules
    for n_max in (1, 0, -3):
        with pytest.raises(ValueError, match="n_max >= 2"):
            _builder(n_mol=1, a_cap=8, n_max=n_max)
    for n_mol, a_cap, n_max in ((0, 8, 4), (9, 8, 4), (2, 8, 9)):
        with pytest.raises(ValueError):
            _builder(n_mol, a_cap, n_max)
    with pytest.raises(ValueError, match="int32"):             # the adjacency blocks: a_cap * n_max bytes
        _builder(4, 1 << 16, 1 << 15)
    # the triplets-only class keeps refusing quadruplet models, word for word
    with pytest.raises(NotImplementedError) as err:
        DeviceCapacityGraphBuilder(GQ.N_MOL, GQ.A_CAP, GQ.N_MAX, GQ.CUTOFF, triplets_only=False, device="cpu")
    assert str(err.value) == ("DeviceCapacityGraphBuilder: triplets-only models (GemNet-T) only, not GemNet-Q "
                              "(quadruplet lists with an atom capacity are not built inside the graph)")
    # the layout is the base class's
    b.set_layout([3, 1, 5, 2])
    assert b.mol_off.tolist() == [0, 3, 4, 9, 11, 72] and b.sq_off.tolist() == [0, 9, 10, 35, 39] and b.A == 11
    with pytest.raises(ValueError, match="set_layout"):
        b(torch.zeros(10, 3))


# ----------------------------------------------------------------------------------------------------------------- the runner
def _runner(model=None, a_cap=GQ.A_CAP, quad=True, **kw):
    (e_cap, t_cap, *qc), deg, groups = GQ.CAPS, GQ.DEG, GQ.GROUPS
    R, Z, N, idx = GQ.tensors(GQ.stream()[0], "cpu")
    if quad:
        kw["quad_caps"] = tuple(qc)
    run = PaddedGraphRunner(model or (_Q() if quad else _M()), Z, N, e_cap, t_cap, max_in_degree=deg, n_groups=groups, a_cap=a_cap,
                            **kw)
    return run, (R, Z, N, idx)


def test_attach_builder_accepts_the_quadruplet_capacity_builder():
    run, (R, Z, N, idx) = _runner()
    with pytest.raises(RuntimeError, match="attach_builder"):
        run.attach_builder(_builder())                          # the buffers hold no batch yet
    run._fill(R, idx, Z, N)
    b = _builder()
    run.attach_builder(b)
    assert run.builder is b and run.graph is None
    assert b.N32.tolist() == GQ.stream()[0]["N"] and b.n_atoms.tolist() == [11]     # the batch the buffers hold
    assert run._staging.numel() == 4 * run.e_cap + 2 * run.quad_caps[0] and not run._staging.any()
    assert run._idx_state.numel() == 8 and run._idx_host.numel() == 8
    assert run.index_error() == 0 and run.index_sizes() == (0, 0, 0, 0, 0)
    # the fill of a later batch hands its sizes to the builder as well
    R2, Z2, N2, idx2 = GQ.tensors(GQ.stream()[2], "cpu")
    run._fill(R2, idx2, Z2, N2)
    assert b.N32.tolist() == GQ.stream()[2]["N"] and b.n_atoms.tolist() == [72]
    want = pad_indices(idx2, run.a_cap, run.e_cap, run.t_cap, run.G, quad_caps=run.quad_caps)
    assert all(torch.equal(run.padded_inputs()[k].long(), want[k]) for k in GQ.KEYS)


def test_attach_builder_refusals():
    (e_cap, t_cap, *qc), deg, groups = GQ.CAPS, GQ.DEG, GQ.GROUPS
    R, Z, N, idx = GQ.tensors(GQ.stream()[0], "cpu")
    kw = dict(max_in_degree=deg, n_groups=groups)
    triplets = PaddedGraphRunner(_M(), Z, N, e_cap, t_cap, a_cap=GQ.A_CAP, **kw)
    fixed = PaddedGraphRunner(_Q(), Z, N, e_cap, t_cap, quad_caps=tuple(qc), **kw)
    periodic = PaddedGraphRunner(_M(), Z, N, e_cap, t_cap, cell=torch.eye(3).repeat(4, 1, 1), **kw)
    for run in (triplets, fixed, periodic):
        with pytest.raises(ValueError, match="different systems"):
            run.attach_builder(_builder())
        assert run.builder is None
    run, _ = _runner()
    run._fill(R, idx, Z, N)
    # a triplets-only capacity builder on a quadruplet runner; a mismatch in n_mol or a_cap
    others = (DeviceCapacityGraphBuilder(GQ.N_MOL, GQ.A_CAP, GQ.N_MAX, GQ.CUTOFF, device="cpu"), _builder(n_mol=3),
              _builder(a_cap=GQ.A_CAP + 1))
    for other in others:
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
    R2, Z2, N2, _ = GQ.tensors(GQ.stream()[2], "cpu")
    big_R, big_Z = torch.cat([R2, R2[:1] + 0.5]), torch.cat([Z2, Z2[:1]])
    with pytest.raises(ValueError, match=f"exceeds a_cap = {GQ.A_CAP}"):
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
    # the sticky report of an earlier step names all five capacities and all five sizes
    run._idx_host[0], run._idx_host[6] = 64, 99
    with pytest.raises(ValueError, match=rf"quad_caps \({GQ.CAPS[2]}, {GQ.CAPS[3]}, {GQ.CAPS[4]}\).*bits 64, sizes \(0, 0, 0, 0, 99\)"):
        run.run_positions(R2, Z=Z2, N=N2)
    run.reset_index_state()
    assert run.index_error() == 0 and run.A == 11


# ---------------------------------------------------------------------------------------------------------------- the Trainer
def _batch(b):
    inputs = {k: torch.tensor(v) for k, v in b["ref"].items()}
    inputs.update(R=torch.tensor(b["R"]).double(), Z=torch.tensor(b["Z"]), N=torch.tensor(b["N"]))
    Et, Ft = GQ.targets(b)
    return inputs, {"E": torch.tensor(Et), "F": torch.tensor(Ft)}


def test_enable_padded_eval_routes_quadruplet_models():
    """On the host emulation of the launchers (float64).  Without `quad_caps` a quadruplet model never builds a runner, whatever
    the batch; with them a batch that does not fit on the host (atoms, a molecule above n_max, another number of molecules) takes
    the plain path as well — the plain path's metrics, no runner.  A batch that fits would take the graph; direct-force models and
    mve never do."""
    (e_cap, t_cap, *qc), deg, groups = GQ.CAPS, GQ.DEG, GQ.GROUPS
    stream = GQ.stream()
    kw = dict(e_cap=e_cap, t_cap=t_cap, max_in_degree=deg, n_groups=groups)
    with cpu_kernels.emulate():
        model = build(CFG, Q.make_params(CFG)).eval()
        assert not model.triplets_only and float(model.cbf_basis.cutoff) == GQ.INT_CUTOFF
        plain, routed = Trainer(model), Trainer(model)
        for t in (plain, routed):
            t.dict2device = lambda d, device=None: d                # float64 CPU emulation
        cases = ((dict(a_cap=72, n_max=66), 0), (dict(a_cap=72, n_max=66), 1),                          # no quad_caps
                 (dict(a_cap=10, n_max=66, quad_caps=qc), 0), (dict(a_cap=72, n_max=4, quad_caps=qc), 0),
                 (dict(a_cap=72, n_max=66, n_mol=5, quad_caps=qc), 1))
        for caps, s in cases:
            routed.enable_padded_eval(**kw, **caps)
            m0, m1 = Metrics("val", plain.tracked_metrics), Metrics("val", routed.tracked_metrics)
            l0 = plain.test_on_batch(iter([_batch(stream[s])]), m0)
            l1 = routed.test_on_batch(iter([_batch(stream[s])]), m1)
            assert float(l0) == float(l1) and m0.result() == m1.result() and routed._erun is None, caps
            (E1, F1), _ = routed.eval_on_batch(iter([_batch(stream[s])]))
            (E0, F0), _ = plain.eval_on_batch(iter([_batch(stream[s])]))
            assert torch.equal(E0, E1) and torch.equal(F0, F1) and routed._erun is None
            E1, _, F1, _ = routed.predict_on_batch(iter([_batch(stream[s])]))
            assert torch.equal(E0, E1) and torch.equal(F0, F1) and routed._erun is None
        inputs, _ = _batch(stream[0])
        n_host = inputs["N"]
        routed.enable_padded_eval(a_cap=72, n_max=66, **kw)
        assert routed._eval_caps["quad_caps"] is None and not routed._eval_fits(inputs, n_host)
        routed.enable_padded_eval(a_cap=72, n_max=66, quad_caps=qc, **kw)
        assert routed._eval_caps["quad_caps"] == tuple(qc)
        assert routed._eval_fits(inputs, n_host)                    # this one would take the graph ...
        assert not routed._eval_fits(inputs, None)                  # ... but not without its sizes,
        assert not routed._eval_fits(dict(inputs, Z=inputs["Z"][:-1]), n_host)     # with sizes that do not add up,
        model.direct_forces = True                                   # for a direct-force model
        assert not routed._eval_fits(inputs, n_host)
        model.direct_forces = False
        routed.mve = True                                            # or with mve
        assert not routed._eval_fits(inputs, n_host)
        routed.mve = False
        # single atoms with n_max = 1: the quadruplet builder has no room for a pair, the batch takes the plain path
        ones = dict(inputs, Z=inputs["Z"][:4], R=inputs["R"][:4], N=torch.ones(4, dtype=torch.int64))
        routed.enable_padded_eval(a_cap=72, n_max=1, quad_caps=qc, **kw)
        assert not routed._eval_fits(ones, ones["N"])
        routed.enable_padded_eval(a_cap=72, n_max=2, quad_caps=qc, **kw)
        assert routed._eval_fits(ones, ones["N"])
        with pytest.raises(ValueError, match="quad_caps"):
            routed.enable_padded_eval(a_cap=72, n_max=66, quad_caps=(8, 8), **kw)


# ------------------------------------------------------------------------------------------------------------ declarations
def test_new_symbol_is_declared_bound_and_classified():
    from gemnet_pytorch_amd import _lib, hbcheck, kernels
    text = open(os.path.join(ROOT, "include", "gemnet_hip.h")).read()
    assert re.search(r"\bint\s+gn_index_gpu_padded_qv\s*\(", text)
    funcs, _ = hbcheck.parse_header()
    qv, q = funcs["gn_index_gpu_padded_qv"], funcs["gn_index_gpu_padded_q"]
    assert len(qv) == len(_lib.SIGNATURES["gn_index_gpu_padded_qv"]) == len(q) - 1          # + atom_mol; (B, A, sum_n2) -> n_mol
    kinds = dict(qv)
    assert all(kinds[k] == "r" for k in ("R", "mol_off", "sq_off", "atom_mol"))
    assert all(kinds[k] == "w" for k in ("ws", "staging", "state")) and kinds["arrays"] == "wa" == dict(q)["arrays"]
    assert all(kinds[k] is None for k in ("n_mol", "n_max", "cutoff", "int_cutoff", "e_cap", "t_cap", "eint_cap", "i_cap", "q_cap",
                                          "a_cap", "n_groups", "deg_bound"))
    assert qv[-1] == ("stream", "stream")
    # the fixed-layout entry keeps its signature
    assert [n for n, _ in q][:10] == ["R", "r_is_f64", "mol_off", "sq_off", "B", "A", "nmax", "sum_n2", "cutoff", "int_cutoff"]
    assert callable(kernels.index_padded_qv) and tuple(kernels.PADDED_Q_KEYS) == tuple(GQ.KEYS)
    src = open(os.path.join(ROOT, "gemnet_pytorch_amd", "csrc", "index_gpu.hip")).read()
    assert 'extern "C" int gn_index_gpu_padded_qv' in src and "static int idx_run_padded_q" in src
    # the workspace of the quadruplet capacity shapes; the triplets-only default is unchanged
    lib = _lib.load()
    assert kernels.index_cap_ws_bytes(72, 66, quad=True) == lib.gn_index_gpu_ws_bytes(72, 72 * 66, 0)
    assert kernels.index_cap_ws_bytes(72, 66) == kernels.index_cap_ws_bytes(72, 66, quad=False) == lib.gn_index_gpu_ws_bytes(72, 72 * 66, 1)
    assert kernels.index_cap_ws_bytes(72, 66, quad=True) >= lib.gn_index_gpu_ws_bytes(72, 66 * 66 + 14, 0)
    with pytest.raises(ValueError, match="int32"):
        kernels.index_cap_ws_bytes(1 << 16, 1 << 15, quad=True)
    assert "gn_abi_version() == 16" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
