"""GPU: periodic batches whose structure SIZES change from replay to replay of ONE captured graph (the atom capacity of
padded.PaddedGraphRunner(a_cap=, cell=) behind `model.periodic_atom_capacity`) — the layout kernel (gn_pbc_layout) against
padded.capacity_layout, the index entry sized by the atom capacity (gn_pbc_index_padded_tv) against pbc.PeriodicGraphBuilder and
`pad_indices`, inference bit for bit against the eager model on the unpadded batch (lists handed in / built inside the replay), a
batch that outgrows the capacities, the host checks and the happens-before check of the capture.

Stream: tests/pbc_ragged_common.py — 10, 6, 72 (= a_cap) and again 10 atoms in four structures; the 65-atom structure crosses
the 64-lane partner loop of the pair search, the slab changes its slot, atoms that were real become fillers."""
import numpy as np
import pytest
import torch

import pbc_common as P
import pbc_direct_train_common as DT
import pbc_padded_train_common as C
import pbc_ragged_common as G
import pbc_train_common as PT
from conftest import SCALE_FILE
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd.model.gemnet import GemNet
from gemnet_pytorch_amd.padded import PaddedGraphRunner, capacity_layout, pad_indices
from gemnet_pytorch_amd.pbc import PeriodicCapacityGraphBuilder, PeriodicGraphBuilder
from gemnet_pytorch_amd.training.periodic import PeriodicPaddedTrainStep
from oracle import gemnet_oracle as GO
from redzone import put, redzone_on_request  # noqa: F401  (the kernel tests ask for `redzone`: they run under the red-zone harness)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFGS = {"cfg": dict(P.CFG, num_blocks=2), "wide": dict(PT.CFG_WIDE, num_blocks=2)}
I32, I64 = torch.int32, torch.int64


# ------------------------------------------------------------------------------------------------------------ layout kernel
def _layout_buffers(n_mol, a_cap, a_tot):
    """Output arrays of gn_pbc_layout filled with values no layout produces."""
    return dict(mol_off=torch.full((n_mol + 2,), -7, dtype=I32, device=DEV), atom_mol=torch.full((a_cap,), -7, dtype=I32, device=DEV),
                batch_seg=torch.full((a_tot,), -7, dtype=I64, device=DEV), N=torch.full((n_mol + 1,), -7, dtype=I64, device=DEV),
                mask=torch.full((a_cap,), -7.0, dtype=torch.float32, device=DEV))


def _run_layout(N, n_atoms, n_mol, a_cap, a_tot, out, state):
    K.pbc_layout(put(torch.tensor(N, dtype=I32)), put(torch.tensor([n_atoms], dtype=I32)), n_mol, a_cap, a_tot, out["mol_off"],
                 out["atom_mol"], out["batch_seg"], out["N"], out["mask"], state)
    torch.cuda.synchronize()


def _sizes_for(n_mol, a_cap, exact):
    """n_mol sizes >= 1 that end exactly at a_cap, or well below it (all ones where nothing lower exists)."""
    N = [1] * n_mol
    extra = (a_cap - n_mol) if exact else (a_cap - n_mol) // 3
    for k in range(extra):
        N[(7 * k) % n_mol] += 1
    return N


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("n_mol,a_cap", [(1, 1), (4, 72), (1025, 1100)])
def test_layout_kernel_equals_capacity_layout(n_mol, a_cap, exact, redzone):
    """mol_off, atom_mol, batch_seg, N and the mask, integer arrays with torch.equal; 1025 structures need a second round of the
    one-block scan; a valid layout resets state[3] and keeps the sticky word."""
    N = [65, 3, 3, 1] if (n_mol, exact) == (4, True) else [3, 3, 3, 1] if n_mol == 4 else _sizes_for(n_mol, a_cap, exact)
    A, a_tot = sum(N), a_cap + 6
    assert (A == a_cap) == (exact or n_mol == a_cap) and len(N) == n_mol
    out = _layout_buffers(n_mol, a_cap, a_tot)
    state = torch.zeros(8, dtype=I32, device=DEV)
    state[0], state[3] = 2, 128                                 # an earlier step's report
    _run_layout(N, A, n_mol, a_cap, a_tot, out, state)
    ref = capacity_layout(torch.tensor(N), n_mol, a_cap, a_tot)
    for k, v in ref.items():
        assert out[k].dtype == v.dtype and torch.equal(out[k].cpu(), v), k
    assert state.tolist() == [2, 0, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("case", ["sum != n_atoms", "a size of 0", "sum > a_cap"])
def test_layout_kernel_refuses_sizes_that_do_not_add_up(case, redzone):
    """Each sets bit 128 (state[0] sticky, state[3]) and leaves every output array as it was.  Handled paths: nothing faults."""
    n_mol, a_cap, a_tot = 4, 72, 78
    N, n_atoms = {"sum != n_atoms": ([3, 3, 3, 1], 11), "a size of 0": ([3, 0, 6, 1], 10), "sum > a_cap": ([65, 3, 3, 2], 73)}[case]
    out = _layout_buffers(n_mol, a_cap, a_tot)
    state = torch.zeros(8, dtype=I32, device=DEV)
    _run_layout([65, 3, 3, 1], 72, n_mol, a_cap, a_tot, out, state)       # a valid layout first
    kept = {k: v.clone() for k, v in out.items()}
    state[0], state[1], state[2] = 1, 42, 146
    _run_layout(N, n_atoms, n_mol, a_cap, a_tot, out, state)
    assert state.tolist() == [129, 42, 146, 128, 0, 0, 0, 0]
    assert all(torch.equal(out[k], kept[k]) for k in out)
    _run_layout([3, 3, 3, 1], 10, n_mol, a_cap, a_tot, out, state)        # the next valid layout: the sticky word stays
    assert state.tolist()[:4] == [129, 42, 146, 0]
    assert torch.equal(out["N"].cpu(), capacity_layout(torch.tensor([3, 3, 3, 1]), n_mol, a_cap, a_tot)["N"])


# -------------------------------------------------------------------------------------------------------------- index entry
def test_index_entry_sized_by_the_atom_capacity(redzone):
    """Every batch of the stream through ONE set of buffers: real rows = PeriodicGraphBuilder(N)(R, cell) with torch.equal, state =
    (0, E, T, 0, largest in-degree), pad rows = pad_indices, no filler atom in any array.  The filler rows of R are NOT reset:
    behind the 72-atom batch they hold real positions inside real cells, and still pair with nothing.  The capacity builder's own
    host-sized build returns the same dict.  A layout the step refused lets the entry write nothing."""
    e_cap, t_cap, deg, groups = G.CAPS
    n_mol, a_cap = G.N_MOL, G.A_CAP
    a_tot = a_cap + 3 * groups
    cb = PeriodicCapacityGraphBuilder(n_mol, a_cap, G.CUTOFF, device=DEV)
    bufs = {k: torch.full((e_cap,), -1, dtype=I32, device=DEV) for k in ("id_c", "id_a", "id_swap", "id_undir")}
    bufs.update({k: torch.full((t_cap,), -1, dtype=I32, device=DEV) for k in ("id3_reduce_ca", "id3_expand_ba")})
    bufs["cell_offsets"] = torch.full((e_cap, 3), -1, dtype=I32, device=DEV)
    lay = _layout_buffers(n_mol, a_cap, a_tot)
    ws = torch.zeros(K.pbc_index_ws_bytes(a_cap, e_cap), dtype=torch.uint8, device=DEV)
    staging = torch.zeros(7 * e_cap, dtype=I32, device=DEV)
    state = torch.zeros(8, dtype=I32, device=DEV)
    Rbuf = torch.zeros(a_cap, 3, dtype=torch.float32, device=DEV)       # fillers at the origin: inside every cell
    cellbuf = torch.ones(n_mol + 1, 3, 3, dtype=torch.float32, device=DEV)
    cellbuf[n_mol] = torch.eye(3, device=DEV)

    def step(N, A, pbc):
        cb.set_layout(N, pbc, n_atoms=A, arrays=False)
        K.pbc_layout(cb.N32, cb.n_atoms, n_mol, a_cap, a_tot, cb.mol_off, cb.atom_mol, lay["batch_seg"], lay["N"], lay["mask"], state)
        K.pbc_index_padded_tv(cb, Rbuf, cellbuf, e_cap, t_cap, a_cap, groups, deg, ws, staging, bufs, state)
        torch.cuda.synchronize()

    for s, b in enumerate(G.stream()):
        R, Z, N, cell, _ = G.tensors(b, DEV)
        A = int(Z.shape[0])
        Rbuf[:A].copy_(R)
        cellbuf[:n_mol].copy_(cell)
        step(b["N"], A, b["pbc"])
        ref = PeriodicGraphBuilder(b["N"], G.CUTOFF, pbc=b["pbc"], device=DEV)(R, cell, dtype=I32)
        E, T, dmax = G.sizes(b)
        assert (ref["id_c"].shape[0], ref["id3_reduce_ca"].shape[0]) == (E, T), s
        assert state.tolist()[:5] == [0, E, T, 0, dmax], (s, state.tolist())
        want = pad_indices({k: ref[k] for k in G.IDX_KEYS}, a_cap, e_cap, t_cap, groups, dtype=I32)
        for k in G.IDX_KEYS:
            n = T if k.startswith("id3") else E
            assert torch.equal(bufs[k][:n], ref[k].reshape(bufs[k][:n].shape)), (s, k)          # the real rows
            assert np.array_equal(bufs[k][:n].cpu().numpy(), np.asarray(b["ref"][k]).reshape(bufs[k][:n].shape)), (s, k)
            assert torch.equal(bufs[k], want[k].reshape(bufs[k].shape)), (s, k)                 # pad rows; no stale row
        for k in ("id_c", "id_a"):
            assert not bool(((bufs[k] >= A) & (bufs[k] < a_cap)).any()), (s, k)                 # no filler atom
        assert torch.equal(lay["N"].cpu(), capacity_layout(torch.tensor(b["N"]), n_mol, a_cap, a_tot)["N"])
        # the builder's host-sized build for the layout the kernel wrote, and for one it writes itself
        for arrays in (False, True):
            if arrays:
                cb.set_layout(torch.tensor(b["N"], device=DEV), torch.tensor(b["pbc"], device=DEV))
            own = cb(R, cell, dtype=I32)
            assert own.keys() == ref.keys() and all(torch.equal(own[k], ref[k]) for k in ref), (s, arrays)
    # sizes that do not add up: bit 128 from the layout, and the entry writes neither the arrays nor state[]
    kept = {k: v.clone() for k, v in bufs.items()}
    before = state.tolist()
    step([3, 3, 3, 2], 10, G.stream()[0]["pbc"])
    assert state.tolist() == [128] + before[1:3] + [128] + before[4:], state.tolist()
    assert all(torch.equal(bufs[k], kept[k]) for k in bufs)


# ---------------------------------------------------------------------------------------------------------------- inference
_PARAMS = {}


def _model(tag, direct=False, switch=True):
    cfg = DT.direct_cfg(CFGS[tag], True) if direct else CFGS[tag]
    if (tag, direct) not in _PARAMS:
        _PARAMS[tag, direct] = PT.make_params(cfg)
    m = GemNet(**cfg, scale_file=SCALE_FILE)
    m.load_state_dict(GO.expand_to_reference_state_dict({k: v.float() for k, v in _PARAMS[tag, direct].items()}))
    if switch:
        m.periodic_atom_capacity = True
    return m.to(DEV)


def _host_builder(b):
    return PeriodicGraphBuilder(b["N"], G.CUTOFF, pbc=b["pbc"], device=DEV)


def _runner(model, caps=None):
    e_cap, t_cap, deg, groups = caps or G.CAPS
    b0 = G.stream()[0]
    R, Z, N, cell, _ = G.tensors(b0, DEV)
    return PaddedGraphRunner(model, Z, N, e_cap, t_cap, max_in_degree=deg, n_groups=groups, a_cap=G.A_CAP, cell=cell, pbc=b0["pbc"])


def _attach_runner(run):
    b0 = G.stream()[0]
    R, Z, N, cell, _ = G.tensors(b0, DEV)
    run._fill(R, _host_builder(b0)(R, cell, dtype=I32), Z, N, cell)
    cb = PeriodicCapacityGraphBuilder(G.N_MOL, G.A_CAP, G.CUTOFF, device=DEV)
    cb.set_layout(b0["N"], b0["pbc"])
    run.attach_builder(cb)
    return run


@pytest.mark.parametrize("mode", ["call", "positions"])
@pytest.mark.parametrize("direct", [False, True])
def test_replays_equal_the_eager_model_on_the_unpadded_batch(mode, direct):
    """ONE runner, one capture, every batch of the stream: E, F and S torch.equal to model(batch, stress=True) on the unpadded
    batch (GemNet-dT: E, F) — lists handed in (`__call__`) and built inside the replay (`run_positions`)."""
    model = _model("cfg", direct).eval()
    if direct:
        model.periodic_direct_forces = True
    run = _runner(model)
    if mode == "positions":
        _attach_runner(run)
    graph = None
    for s, b in enumerate(G.stream()):
        R, Z, N, cell, _ = G.tensors(b, DEV)
        idx = _host_builder(b)(R, cell, dtype=I32)
        kw = {} if direct else dict(stress=True)
        ref = tuple(t.clone() for t in model(dict(Z=Z, N=N, R=R.clone(), cell=cell.clone(), **idx), **kw))
        if mode == "call":
            E, F = run(R, idx, Z=Z, N=N, cell=cell, pbc=b["pbc"])
        else:
            E, F = run.run_positions(R, Z=Z, N=N, cell=cell, pbc=b["pbc"])
        torch.cuda.synchronize()
        assert E.shape == ref[0].shape and F.shape == ref[1].shape and F.shape[0] == len(b["Z"]), s
        assert torch.equal(E, ref[0]) and torch.equal(F, ref[1]), s
        if not direct:
            assert torch.equal(run.stress(), ref[2]), s
        if mode == "positions":
            assert run.index_error() == 0 and run.index_sizes() == G.sizes(b)[:2] and run.index_in_degree() == G.sizes(b)[2], s
        graph = graph or run.graph
        assert run.graph is graph and graph is not None
    assert not run.flag.tripped()


def test_host_checks_come_before_any_copy():
    """A batch with more atoms than a_cap, another number of structures, or a new atom count without N / Z raise ValueError on
    the host; the buffers keep the batch they held."""
    run = _attach_runner(_runner(_model("cfg").eval()))
    kept = {k: v.clone() for k, v in run.padded_inputs().items()}
    b2 = G.stream()[2]
    R, Z, N, cell, idx = G.tensors(b2, DEV)
    big_R, big_Z = torch.cat([R, R[:1] + 0.5]), torch.cat([Z, Z[:1]])
    big_N = N + torch.tensor([1, 0, 0, 0], device=DEV)
    for call in (lambda: run.run_positions(big_R, Z=big_Z, N=big_N, cell=cell), lambda: run(big_R, idx, Z=big_Z, N=big_N, cell=cell)):
        with pytest.raises(ValueError, match=f"exceeds a_cap = {G.A_CAP}"):
            call()
    with pytest.raises(ValueError, match="changes the number of molecules"):
        run.run_positions(R, Z=Z, N=N[:3], cell=cell)
    with pytest.raises(ValueError, match="the number of atoms changed"):
        run.run_positions(R, cell=cell)
    torch.cuda.synchronize()
    assert all(torch.equal(v, kept[k]) for k, v in run.padded_inputs().items())
    # without the switch: the parent's refusal
    with pytest.raises(NotImplementedError, match=r"periodic cells: fixed structure layout only \(no a_cap\)"):
        _runner(_model("cfg", switch=False).eval())


def test_the_capture_is_race_free():
    """The capture (layout + in-graph neighbour list + plan + periodic model) under the happens-before checker."""
    model = _model("cfg").eval()
    run = _attach_runner(_runner(model))
    run.check = True
    b = G.stream()[2]
    R, Z, N, cell, _ = G.tensors(b, DEV)
    E, F = run.run_positions(R, Z=Z, N=N, cell=cell, pbc=b["pbc"])
    torch.cuda.synchronize()
    races, summary = run.hb.races(), run.hb.summary()
    print(run.hb.format(races))
    assert not races and summary["unrecorded_nodes"] == 0 and summary["unresolved_pointers"] == 0, summary
    idx = _host_builder(b)(R, cell, dtype=I32)
    E0, F0, S0 = model(dict(Z=Z, N=N, R=R.clone(), cell=cell.clone(), **idx), stress=True)
    assert torch.equal(E, E0) and torch.equal(F, F0) and torch.equal(run.stress(), S0)


def test_outgrowing_the_capacities_is_reported_not_computed_on():
    """Capacities that fit batch 0 but not the 65-atom batch: that step returns NaN, reports bit 1 with the edge count, keeps the
    arrays of the step before, and the NEXT call raises ValueError naming capacities, bits and sizes.  Sizes that do not add up to
    the atom count are reported the same way (bit 128).  Handled paths: nothing faults."""
    stream = G.stream()
    caps = C.capacities([G.frame(stream[0])])                   # sized for batch 0 alone
    assert G.sizes(stream[0])[0] <= caps[0] - 4 and G.sizes(stream[0])[1] <= caps[1]
    E2 = G.sizes(stream[2])[0]
    assert E2 > caps[0]
    model = _model("cfg").eval()
    run = _attach_runner(_runner(model, caps=caps))
    for s in (0, 3):
        R, Z, N, cell, _ = G.tensors(stream[s], DEV)
        E, F = run.run_positions(R, Z=Z, N=N, cell=cell, pbc=stream[s]["pbc"])
        torch.cuda.synchronize()
        assert run.index_error() == 0 and bool(torch.isfinite(E).all()) and bool(torch.isfinite(F).all()), s
    kept = {k: run.padded_inputs()[k].clone() for k in G.IDX_KEYS}
    graph = run.graph
    R, Z, N, cell, _ = G.tensors(stream[2], DEV)
    E, F = run.run_positions(R, Z=Z, N=N, cell=cell, pbc=stream[2]["pbc"])
    torch.cuda.synchronize()
    assert run.index_error() == 1 and int(run._idx_host[3]) == 1 and run.index_sizes() == (E2, 0)
    assert F.shape[0] == 72 and torch.isnan(E).all() and torch.isnan(F).all() and torch.isnan(run.stress()).all()
    assert all(torch.equal(run.padded_inputs()[k], kept[k]) for k in G.IDX_KEYS)      # nothing was written
    R, Z, N, cell, _ = G.tensors(stream[3], DEV)
    with pytest.raises(ValueError, match=rf"capacities \({caps[0]}, {caps[1]}, None\)") as err:
        run.run_positions(R, Z=Z, N=N, cell=cell, pbc=stream[3]["pbc"])
    assert "bits 1" in str(err.value) and f"sizes ({E2}, 0)" in str(err.value)
    assert run.graph is graph
    # sizes that do not add up to the atoms handed in: bit 128 from the layout kernel, same report
    run = _attach_runner(_runner(model))
    R, Z, N, cell, _ = G.tensors(stream[0], DEV)
    E, F = run.run_positions(R, Z=Z, N=N, cell=cell, pbc=stream[0]["pbc"])
    torch.cuda.synchronize()
    assert run.index_error() == 0
    kept = {k: v.clone() for k, v in run.padded_inputs().items()}
    wrong = N + torch.tensor([0, 0, 1, 0], device=DEV)          # 11 atoms announced, 10 handed in
    E, F = run.run_positions(R, Z=Z, N=wrong, cell=cell, pbc=stream[0]["pbc"])
    torch.cuda.synchronize()
    assert run.index_error() == 128 and int(run._idx_host[3]) == 128
    assert torch.isnan(E).all() and torch.isnan(F).all() and torch.isnan(run.stress()).all()
    assert all(torch.equal(run.padded_inputs()[k], kept[k]) for k in ("N", "batch_seg") + tuple(G.IDX_KEYS))
    with pytest.raises(ValueError, match="index error bits 128"):
        run.run_positions(R, Z=Z, N=N, cell=cell, pbc=stream[0]["pbc"])


def test_the_training_step_refuses_an_atom_capacity():
    """Training keeps the fixed structure layout: with the switch on the step raises before it builds anything."""
    b0 = G.stream()[0]
    R, Z, N, cell, _ = G.tensors(b0, DEV)
    e_cap, t_cap, deg, groups = G.CAPS
    kw = dict(cell=cell, pbc=b0["pbc"], max_in_degree=deg, n_groups=groups)
    with pytest.raises(NotImplementedError, match="inference only"):
        PeriodicPaddedTrainStep(_model("cfg"), Z, N, e_cap, t_cap, a_cap=G.A_CAP, **kw)
    with pytest.raises(NotImplementedError, match=r"periodic cells: fixed structure layout only \(no a_cap\)"):
        PeriodicPaddedTrainStep(_model("cfg", switch=False), Z, N, e_cap, t_cap, a_cap=G.A_CAP, **kw)
