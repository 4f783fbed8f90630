"""GPU: molecular batches whose molecule SIZES change from replay to replay of ONE captured graph, the lists built inside the
replay — the layout kernel (gn_index_gpu_layout) against padded.capacity_layout and the prefix sums of N^2, the index entry sized
by the capacities (gn_index_gpu_padded_tv) against index_device.DeviceGraphBuilder, the host builder and `pad_indices`, inference
bit for bit against the eager model on the unpadded batch (lists built inside the replay / handed in), a batch that outgrows
the capacities, the happens-before check of the capture and `Trainer.enable_padded_eval`.

Stream: tests/mol_ragged_common.py — 11, 6, 72 (= a_cap) and again 11 atoms in four molecules; the 66-atom molecule takes the
64-lane loop of the triplet writer into a second round and 18 blocks of the adjacency grid, one molecule has no edge, atoms that
were real become fillers."""
import numpy as np
import pytest
import torch

import mol_ragged_common as G
import pbc_common as P
import pbc_padded_train_common as C
import pbc_train_common as PT
from conftest import SCALE_FILE
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd.index_device import DeviceCapacityGraphBuilder, DeviceGraphBuilder
from gemnet_pytorch_amd.model.gemnet import GemNet
from gemnet_pytorch_amd.padded import PaddedGraphRunner, capacity_layout, pad_indices
from gemnet_pytorch_amd.training.data_container import build_indices
from gemnet_pytorch_amd.training.metrics import Metrics
from gemnet_pytorch_amd.training.trainer import Trainer
from oracle import gemnet_oracle as GO
from redzone import put, redzone_on_request  # noqa: F401  (the kernel tests ask for `redzone`: they run under the red-zone harness)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFGS = {"cfg": dict(P.CFG, num_blocks=2), "wide": dict(PT.CFG_WIDE, num_blocks=2)}
I32, I64 = torch.int32, torch.int64


# ------------------------------------------------------------------------------------------------------------ layout kernel
def _layout_buffers(n_mol, a_cap, a_tot):
    """Output arrays of gn_index_gpu_layout filled with values no layout produces."""
    return dict(mol_off=torch.full((n_mol + 2,), -7, dtype=I32, device=DEV), sq_off=torch.full((n_mol + 1,), -7, dtype=I32, device=DEV),
                atom_mol=torch.full((a_cap,), -7, dtype=I32, device=DEV), batch_seg=torch.full((a_tot,), -7, dtype=I64, device=DEV),
                N=torch.full((n_mol + 1,), -7, dtype=I64, device=DEV), mask=torch.full((a_cap,), -7.0, dtype=torch.float32, device=DEV))


def _run_layout(N, n_atoms, n_mol, a_cap, a_tot, n_max, out, state):
    K.index_layout(put(torch.tensor(N, dtype=I32)), put(torch.tensor([n_atoms], dtype=I32)), n_mol, a_cap, a_tot, n_max,
                   out["mol_off"], out["sq_off"], out["atom_mol"], out["batch_seg"], out["N"], out["mask"], state)
    torch.cuda.synchronize()


def _sizes_for(n_mol, a_cap, exact):
    """n_mol sizes >= 1 that end exactly at a_cap, or well below it (all ones where nothing lower exists)."""
    N = [1] * n_mol
    extra = (a_cap - n_mol) if exact else (a_cap - n_mol) // 3
    for k in range(extra):
        N[(7 * k) % n_mol] += 1
    return N


def _layout_reference(N, n_mol, a_cap, a_tot):
    ref = capacity_layout(torch.tensor(N), n_mol, a_cap, a_tot)
    ref["sq_off"] = torch.tensor([0] + list(np.cumsum(np.asarray(N, np.int64) ** 2)), dtype=I32)
    return ref


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("n_mol,a_cap", [(1, 1), (4, 72), (1025, 1100)])
def test_layout_kernel_equals_capacity_layout_and_the_prefix_sums_of_squares(n_mol, a_cap, exact, redzone):
    """mol_off, sq_off, atom_mol, batch_seg, N and the mask, integer arrays with torch.equal; 1025 molecules need a second round
    of the one-block scan (both carries); a valid layout resets state[3] and keeps the sticky word."""
    N = [66, 1, 3, 2] if (n_mol, exact) == (4, True) else [3, 1, 5, 2] if n_mol == 4 else _sizes_for(n_mol, a_cap, exact)
    A, a_tot, n_max = sum(N), a_cap + 6, max(N)
    assert (A == a_cap) == (exact or n_mol == a_cap) and len(N) == n_mol
    out = _layout_buffers(n_mol, a_cap, a_tot)
    state = torch.zeros(8, dtype=I32, device=DEV)
    state[0], state[3] = 2, 128                                 # an earlier step's report
    _run_layout(N, A, n_mol, a_cap, a_tot, n_max, out, state)
    ref = _layout_reference(N, n_mol, a_cap, a_tot)
    assert sorted(ref) == sorted(out)
    for k, v in ref.items():
        assert out[k].dtype == v.dtype and torch.equal(out[k].cpu(), v), k
    assert state.tolist() == [2, 0, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("case", ["sum != n_atoms", "a size of 0", "sum > a_cap", "a size > n_max"])
def test_layout_kernel_refuses_sizes_that_do_not_fit(case, redzone):
    """Each sets bit 128 (state[0] sticky, state[3]) and leaves every output array as it was.  Handled paths: nothing faults."""
    n_mol, a_cap, a_tot, n_max = 4, 72, 78, 66
    N, n_atoms = {"sum != n_atoms": ([3, 1, 5, 2], 12), "a size of 0": ([3, 0, 6, 2], 11), "sum > a_cap": ([66, 3, 3, 1], 73),
                  "a size > n_max": ([67, 1, 1, 1], 70)}[case]
    out = _layout_buffers(n_mol, a_cap, a_tot)
    state = torch.zeros(8, dtype=I32, device=DEV)
    _run_layout([66, 1, 3, 2], 72, n_mol, a_cap, a_tot, n_max, out, state)       # a valid layout first
    kept = {k: v.clone() for k, v in out.items()}
    state[0], state[1], state[2] = 1, 42, 146
    _run_layout(N, n_atoms, n_mol, a_cap, a_tot, n_max, out, state)
    assert state.tolist() == [129, 42, 146, 128, 0, 0, 0, 0]
    assert all(torch.equal(out[k], kept[k]) for k in out)
    _run_layout([3, 1, 5, 2], 11, n_mol, a_cap, a_tot, n_max, out, state)        # the next valid layout: the sticky word stays
    assert state.tolist()[:4] == [129, 42, 146, 0]
    ref = _layout_reference([3, 1, 5, 2], n_mol, a_cap, a_tot)
    assert all(torch.equal(out[k].cpu(), ref[k]) for k in ref)


# -------------------------------------------------------------------------------------------------------------- index entry
def _index_buffers(e_cap, t_cap):
    bufs = {k: torch.full((e_cap,), -1, dtype=I32, device=DEV) for k in ("id_c", "id_a", "id_swap", "id_undir")}
    bufs.update({k: torch.full((t_cap,), -1, dtype=I32, device=DEV) for k in ("id3_reduce_ca", "id3_expand_ba")})
    return bufs


def _fixed_builder(b):
    return DeviceGraphBuilder(b["N"], G.CUTOFF, G.CUTOFF, triplets_only=True, device=DEV)


def test_index_entry_sized_by_the_capacities(redzone):
    """Every batch of the stream through ONE set of buffers: real rows = DeviceGraphBuilder(N)(R) and the host builder's arrays
    with torch.equal, state[:4] = (0, E, T, 0), all rows = pad_indices, no filler atom in any array.  The filler rows of R are NOT
    reset: behind the 72-atom batch they hold the positions of real atoms, and still pair with nothing.  The capacity builder's
    own host-sized build returns the same dict.  A batch beyond e_cap reports bit 1, a layout the step refused bit 128: neither
    writes an array."""
    e_cap, t_cap, deg, groups = G.CAPS
    n_mol, a_cap = G.N_MOL, G.A_CAP
    a_tot = a_cap + 3 * groups
    cb = DeviceCapacityGraphBuilder(n_mol, a_cap, G.N_MAX, G.CUTOFF, device=DEV)
    assert cb.ws.numel() >= K.index_cap_ws_bytes(a_cap, G.N_MAX) > 0
    bufs = _index_buffers(e_cap, t_cap)
    lay = _layout_buffers(n_mol, a_cap, a_tot)
    staging = torch.zeros(4 * e_cap + 2 * t_cap, dtype=I32, device=DEV)
    state = torch.zeros(8, dtype=I32, device=DEV)
    Rbuf = torch.zeros(a_cap, 3, dtype=torch.float32, device=DEV)       # fillers at the origin: next to the batch's first atoms

    def step(N, A, bufs=bufs, staging=staging, state=state, caps=(e_cap, t_cap, groups, deg)):
        cb.set_layout(N, n_atoms=A, arrays=False)
        K.index_layout(cb.N32, cb.n_atoms, n_mol, a_cap, a_tot, cb.n_max, cb.mol_off, cb.sq_off, cb.atom_mol, lay["batch_seg"],
                       lay["N"], lay["mask"], state)
        K.index_padded_tv(cb, Rbuf, caps[0], caps[1], a_cap, caps[2], caps[3], staging, bufs, state)
        torch.cuda.synchronize()

    for s, b in enumerate(G.stream()):
        R, Z, N, _ = G.tensors(b, DEV)
        A = int(Z.shape[0])
        Rbuf[:A].copy_(R)
        step(b["N"], A)
        ref = _fixed_builder(b)(R, dtype=I32)
        host = build_indices(b["R"], np.array(b["N"]), G.CUTOFF, G.CUTOFF, True)
        E, T, _ = G.sizes(b)
        assert (ref["id_c"].shape[0], ref["id3_reduce_ca"].shape[0]) == (E, T), s
        assert state.tolist()[:4] == [0, E, T, 0], (s, state.tolist())
        want = pad_indices({k: ref[k] for k in G.IDX_KEYS}, a_cap, e_cap, t_cap, groups, dtype=I32)
        for k in G.IDX_KEYS:
            n = T if k.startswith("id3") else E
            assert torch.equal(bufs[k][:n], ref[k]), (s, k)                                     # the real rows
            assert np.array_equal(bufs[k][:n].cpu().numpy(), host[k]), (s, k)
            assert np.array_equal(host[k], b["ref"][k]), (s, k)
            assert torch.equal(bufs[k], want[k]), (s, k)                                        # pad rows; no stale row
        for k in ("id_c", "id_a"):
            assert not bool(((bufs[k] >= A) & (bufs[k] < a_cap)).any()), (s, k)                 # no filler atom
        ref_lay = _layout_reference(b["N"], n_mol, a_cap, a_tot)
        assert torch.equal(lay["N"].cpu(), ref_lay["N"]) and torch.equal(cb.sq_off.cpu(), ref_lay["sq_off"])
        # the builder's host-sized build for the layout the kernel wrote, and for one it writes itself
        for arrays in (False, True):
            if arrays:
                cb.set_layout(torch.tensor(b["N"], device=DEV))
            own = cb(R, dtype=I32)
            assert own.keys() == ref.keys() and all(torch.equal(own[k], ref[k]) for k in ref), (s, arrays)
    # sizes that do not add up: bit 128 from the layout, and the entry writes neither the arrays nor state[]
    kept = {k: v.clone() for k, v in bufs.items()}
    before = state.tolist()
    step([3, 1, 5, 3], 11)
    assert state.tolist() == [128] + before[1:3] + [128] + before[4:], state.tolist()
    assert all(torch.equal(bufs[k], kept[k]) for k in bufs)
    # more edges than e_cap: buffers sized for batch 0 alone take batch 0, then report bit 1 for the 72-atom batch
    stream = G.stream()
    small = C.capacities([G.frame(stream[0])])
    E2 = G.sizes(stream[2])[0]
    assert E2 > small[0]
    bufs2, staging2 = _index_buffers(small[0], small[1]), torch.zeros(4 * small[0] + 2 * small[1], dtype=I32, device=DEV)
    state2 = torch.zeros(8, dtype=I32, device=DEV)
    for s, expect in ((0, [0, G.sizes(stream[0])[0], G.sizes(stream[0])[1], 0]), (2, [1, E2, 0, 1])):
        R, Z, N, _ = G.tensors(stream[s], DEV)
        Rbuf[:len(Z)].copy_(R)
        if s == 2:
            kept = {k: v.clone() for k, v in bufs2.items()}
        step(stream[s]["N"], len(Z), bufs2, staging2, state2, (small[0], small[1], small[3], small[2]))
        assert state2.tolist()[:4] == expect, (s, state2.tolist())
    assert all(torch.equal(bufs2[k], kept[k]) for k in bufs2)


# ---------------------------------------------------------------------------------------------------------------- inference
_PARAMS = {}


def _model(tag):
    cfg = CFGS[tag]
    if tag not in _PARAMS:
        _PARAMS[tag] = PT.make_params(cfg)
    m = GemNet(**cfg, scale_file=SCALE_FILE)
    m.load_state_dict(GO.expand_to_reference_state_dict({k: v.float() for k, v in _PARAMS[tag].items()}))
    return m.to(DEV)


def _runner(model, caps=None):
    e_cap, t_cap, deg, groups = caps or G.CAPS
    R, Z, N, _ = G.tensors(G.stream()[0], DEV)
    return PaddedGraphRunner(model, Z, N, e_cap, t_cap, max_in_degree=deg, n_groups=groups, a_cap=G.A_CAP)


def _attach_runner(run):
    b0 = G.stream()[0]
    R, Z, N, _ = G.tensors(b0, DEV)
    run._fill(R, _fixed_builder(b0)(R, dtype=I32), Z, N)
    cb = DeviceCapacityGraphBuilder(G.N_MOL, G.A_CAP, G.N_MAX, G.CUTOFF, device=DEV)
    run.attach_builder(cb.set_layout(b0["N"]))
    return run


@pytest.mark.parametrize("tag", ["cfg", "wide"])
def test_replays_equal_the_eager_model_on_the_unpadded_batch(tag):
    """ONE runner with the lists built inside the replay, one capture, every batch of the stream: E and F torch.equal to the
    eager model on the unpadded batch and to a runner of the same configuration that is handed the lists."""
    model = _model(tag).eval()
    run, handed = _attach_runner(_runner(model)), _runner(model)
    graph = None
    for s, b in enumerate(G.stream()):
        R, Z, N, _ = G.tensors(b, DEV)
        idx = _fixed_builder(b)(R, dtype=I32)
        ref = tuple(t.detach().clone() for t in model(dict(Z=Z, N=N, R=R.clone(), **idx)))
        E1, F1 = (t.clone() for t in handed(R, {k: idx[k] for k in G.IDX_KEYS}, Z=Z, N=N))
        E, F = run.run_positions(R, Z=Z, N=N)
        torch.cuda.synchronize()
        assert E.shape == ref[0].shape and F.shape == ref[1].shape and F.shape[0] == len(b["Z"]), s
        assert torch.equal(E, ref[0]) and torch.equal(F, ref[1]), (s, float((F - ref[1]).abs().max()))
        assert torch.equal(E, E1) and torch.equal(F, F1), s
        assert run.index_error() == 0 and run.index_sizes() == G.sizes(b)[:2], s
        graph = graph or run.graph
        assert run.graph is graph and graph is not None
    assert not run.flag.tripped() and not handed.flag.tripped()


def test_the_capture_is_race_free():
    """The capture (layout + in-graph lists + plan + model) under the happens-before checker."""
    model = _model("cfg").eval()
    run = _attach_runner(_runner(model))
    run.check = True
    b = G.stream()[2]
    R, Z, N, _ = G.tensors(b, DEV)
    E, F = run.run_positions(R, Z=Z, N=N)
    torch.cuda.synchronize()
    races, summary = run.hb.races(), run.hb.summary()
    print(run.hb.format(races))
    assert not races and summary["unrecorded_nodes"] == 0 and summary["unresolved_pointers"] == 0, summary
    E0, F0 = model(dict(Z=Z, N=N, R=R.clone(), **_fixed_builder(b)(R, dtype=I32)))
    assert torch.equal(E, E0) and torch.equal(F, F0)


def test_outgrowing_the_capacities_is_reported_not_computed_on():
    """Capacities that fit batch 0 but not the 66-atom batch: that step returns NaN, reports bit 1 with the edge count, keeps the
    arrays of the step before, and the NEXT call raises ValueError naming capacities, bits and sizes; after reset_index_state()
    the runner serves again.  A molecule above n_max and sizes that do not add up to the atoms handed in are reported the same
    way (bit 128).  Handled paths: nothing faults."""
    stream = G.stream()
    caps = C.capacities([G.frame(stream[0])])                   # sized for batch 0 alone
    assert G.sizes(stream[0])[0] <= caps[0] - 4 and G.sizes(stream[0])[1] <= caps[1]
    E2 = G.sizes(stream[2])[0]
    assert E2 > caps[0]
    model = _model("cfg").eval()
    run = _attach_runner(_runner(model, caps=caps))
    ref = {}
    for s in (0, 3):
        R, Z, N, _ = G.tensors(stream[s], DEV)
        E, F = run.run_positions(R, Z=Z, N=N)
        torch.cuda.synchronize()
        assert run.index_error() == 0 and bool(torch.isfinite(E).all()) and bool(torch.isfinite(F).all()), s
        ref[s] = (E.clone(), F.clone())
    kept = {k: run.padded_inputs()[k].clone() for k in G.IDX_KEYS}
    graph = run.graph
    R, Z, N, _ = G.tensors(stream[2], DEV)
    E, F = run.run_positions(R, Z=Z, N=N)
    torch.cuda.synchronize()
    assert run.index_error() == 1 and int(run._idx_host[3]) == 1 and run.index_sizes() == (E2, 0)
    assert F.shape[0] == 72 and torch.isnan(E).all() and torch.isnan(F).all()
    assert all(torch.equal(run.padded_inputs()[k], kept[k]) for k in G.IDX_KEYS)      # nothing was written
    R, Z, N, _ = G.tensors(stream[3], DEV)
    with pytest.raises(ValueError, match=rf"e_cap {caps[0]}, t_cap {caps[1]}, a_cap {G.A_CAP}, n_max {G.N_MAX}") as err:
        run.run_positions(R, Z=Z, N=N)
    assert "bits 1" in str(err.value) and f"sizes ({E2}, 0)" in str(err.value)
    run.reset_index_state()
    E, F = run.run_positions(R, Z=Z, N=N)
    torch.cuda.synchronize()
    assert run.index_error() == 0 and torch.equal(E, ref[3][0]) and torch.equal(F, ref[3][1]) and run.graph is graph
    # bit 128 from the layout kernel: sizes that do not add up to the atoms handed in, and a molecule above n_max
    kept = {k: v.clone() for k, v in run.padded_inputs().items() if k not in ("R", "Z")}
    R0, Z0, N0, _ = G.tensors(stream[0], DEV)
    wrong = N0 + torch.tensor([0, 0, 1, 0], device=DEV)         # 12 atoms announced, 11 handed in
    R67 = torch.cat([G.tensors(stream[2], DEV)[0][:66], R0[:4] + 50.0])
    cases = ((R0, Z0, wrong), (R67, torch.ones(70, dtype=I64, device=DEV), torch.tensor([67, 1, 1, 1], device=DEV)))
    for Rb, Zb, Nb in cases:
        E, F = run.run_positions(Rb, Z=Zb, N=Nb)
        torch.cuda.synchronize()
        assert run.index_error() == 128 and int(run._idx_host[3]) == 128
        assert torch.isnan(E).all() and torch.isnan(F).all()
        assert all(torch.equal(run.padded_inputs()[k], kept[k]) for k in kept)
        with pytest.raises(ValueError, match="index error bits 128"):
            run.run_positions(R0, Z=Z0, N=N0)
        run.reset_index_state()
    E, F = run.run_positions(R0, Z=Z0, N=N0)
    torch.cuda.synchronize()
    assert run.index_error() == 0 and torch.equal(E, ref[0][0]) and torch.equal(F, ref[0][1])


# ------------------------------------------------------------------------------------------------------------------ Trainer
def _loader_batch(b, with_lists):
    """What a loader hands out, on the host: Z, R, N (and the host builder's lists), targets E (4,1) and F (A,3)."""
    inputs = dict(R=torch.tensor(b["R"]), Z=torch.tensor(b["Z"]), N=torch.tensor(b["N"]))
    if with_lists:
        inputs.update({k: torch.tensor(v) for k, v in build_indices(b["R"], np.array(b["N"]), G.CUTOFF, G.CUTOFF, True).items()})
    Et, Ft = G.targets(b)
    return inputs, {"E": torch.tensor(Et, dtype=torch.float32), "F": torch.tensor(Ft, dtype=torch.float32)}


def test_trainer_evaluates_the_stream_through_one_graph():
    """`test_on_batch` over the stream with `enable_padded_eval` (batches of R, Z, N alone) gives the metric values of the plain
    path (batches with their lists) to the bit; `eval_on_batch` / `predict_on_batch` the plain path's energies and forces.  With
    capacities sized for batch 0 the 72-atom batch does not fit: a_cap too small routes it on the host, lists beyond e_cap are
    found inside the replay and the step is repeated on the plain path — same numbers, index state reset."""
    model = _model("cfg")
    e_cap, t_cap, deg, groups = G.CAPS
    stream = G.stream()
    plain, padded = Trainer(model), Trainer(model)
    padded.enable_padded_eval(a_cap=G.A_CAP, e_cap=e_cap, t_cap=t_cap, max_in_degree=deg, n_max=G.N_MAX, n_groups=groups,
                              n_mol=G.N_MOL)
    m0, m1 = Metrics("val", plain.tracked_metrics), Metrics("val", padded.tracked_metrics)
    for s, b in enumerate(stream):
        l0 = plain.test_on_batch(iter([_loader_batch(b, True)]), m0)
        l1 = padded.test_on_batch(iter([_loader_batch(b, False)]), m1)
        assert float(l0) == float(l1), (s, float(l0), float(l1))
        assert padded._erun is not None and padded._erun.index_sizes() == G.sizes(b)[:2], s
    r0, r1 = m0.result(), m1.result()
    assert r0.keys() == r1.keys() and all(float(r0[k]) == float(r1[k]) for k in r0), (r0, r1)
    graph = padded._erun.graph
    (E0, F0), _ = plain.eval_on_batch(iter([_loader_batch(stream[2], True)]))
    (E1, F1), _ = padded.eval_on_batch(iter([_loader_batch(stream[2], False)]))
    E2, _, F2, _ = padded.predict_on_batch(iter([_loader_batch(stream[0], False)]))
    E3, _, F3, _ = plain.predict_on_batch(iter([_loader_batch(stream[0], True)]))
    assert torch.equal(E0, E1) and torch.equal(F0, F1) and torch.equal(E2, E3) and torch.equal(F2, F3)
    assert padded._erun.graph is graph and graph is not None
    # batches that do not fit take the plain path (the batch then carries its lists, as a loader's does)
    small = C.capacities([G.frame(stream[0])])
    for a_cap in (G.A_CAP - 1, G.A_CAP):
        t = Trainer(model)
        t.enable_padded_eval(a_cap=a_cap, e_cap=small[0], t_cap=small[1], max_in_degree=small[2], n_max=G.N_MAX, n_groups=small[3])
        ma, mb = Metrics("val", t.tracked_metrics), Metrics("val", plain.tracked_metrics)
        for s in (0, 2, 3):
            la = t.test_on_batch(iter([_loader_batch(stream[s], True)]), ma)
            lb = plain.test_on_batch(iter([_loader_batch(stream[s], True)]), mb)
            assert float(la) == float(lb) and np.isfinite(float(la)), (a_cap, s)
            assert t._erun is not None and t._erun.index_error() == 0, (a_cap, s)
        assert t._erun.index_sizes() == G.sizes(stream[3])[:2]      # batch 3 went through the graph again
        ra, rb = ma.result(), mb.result()
        assert all(float(ra[k]) == float(rb[k]) for k in rb), (a_cap, ra, rb)


def test_trainer_captures_again_when_the_parameters_change():
    """The evaluation graph reads the parameters' derived forms by address: after an in-place update of the parameters (an
    optimizer step, the EMA swap) and after a train() / eval() round trip (the model drops its cache of derived weights) the next
    padded evaluation captures anew and equals the plain path on the NEW parameters."""
    model = _model("cfg")
    e_cap, t_cap, deg, groups = G.CAPS
    plain, padded = Trainer(model), Trainer(model)
    padded.enable_padded_eval(a_cap=G.A_CAP, e_cap=e_cap, t_cap=t_cap, max_in_degree=deg, n_max=G.N_MAX, n_groups=groups)
    b = G.stream()[0]

    def both():
        (E0, F0), _ = plain.eval_on_batch(iter([_loader_batch(b, True)]))
        (E1, F1), _ = padded.eval_on_batch(iter([_loader_batch(b, False)]))
        assert torch.equal(E0, E1) and torch.equal(F0, F1)
        return E0, padded._erun.graph

    E_a, g_a = both()
    assert both()[1] is g_a                                     # nothing changed: the same graph
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.01)
    E_b, g_b = both()
    assert g_b is not g_a and not torch.equal(E_b, E_a)
    model.train()                                               # eval_on_batch switches back: the cache of derived weights is new
    E_c, g_c = both()
    assert g_c is not g_b and torch.equal(E_c, E_b)
