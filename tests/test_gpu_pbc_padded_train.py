"""GPU: training on a new periodic batch every step from ONE captured graph (training.periodic.PeriodicPaddedTrainStep) — the
one-launch loss kernel against its float64 restatement, the padded step against the eager PeriodicTrainStep on the unpadded
batch, the image neighbour list built inside the replay against lists handed in (bit for bit), a direct-force model, a step that
outgrows the capacities (the optimizer must not move), and the happens-before check of the capture.

Trajectory: tests/pbc_padded_train_common.py (the recipe of tests/test_gpu_pbc_padded.py); 2-block models of the widths of
pbc_common.CFG (composite closure on the device) and pbc_train_common.CFG_WIDE (fused sweeps)."""
import copy
import warnings

import numpy as np
import pytest
import torch

import pbc_common as P
import pbc_direct_train_common as DT
import pbc_padded_train_common as C
import pbc_train_common as PT
from conftest import SCALE_FILE
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd.model.gemnet import GemNet
from gemnet_pytorch_amd.training.periodic import PeriodicPaddedTrainStep, PeriodicTrainStep
from oracle import gemnet_oracle as GO
from redzone import put, redzone_on_request  # noqa: F401  (the kernel test asks for `redzone`: it runs under the red-zone harness)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFGS = {"cfg": dict(P.CFG, num_blocks=2), "wide": dict(PT.CFG_WIDE, num_blocks=2)}
RHO_F, RHO_S = PT.RHO_FORCE, PT.RHO_STRESS


# ------------------------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("A", [1, 37, 1025])
@pytest.mark.parametrize("B", [1, 4])
def test_periodic_loss_kernel(B, A, masked, redzone):
    """gn_periodic_loss_f32 against the float64 composite (pbc_padded_train_common.periodic_loss on the same float32 operands):
    loss, gE, gF, gS to 1e-6 relative (float32 differences, products and one square root and divide per row: a few ulp of 6e-8;
    the sum itself runs in double); nE = B in {1, 4}, A in {1, 37, 1025} straddles the 1024-thread stride; a structure with
    S_b == St_b gets gS_b == 0; S = NULL is gn_force_loss_f32 bit for bit."""
    g = torch.Generator().manual_seed(100 * B + A)
    rnd = lambda *s: torch.randn(*s, generator=g).float()      # noqa: E731
    E, Et, F, Ft, S, St = rnd(B, 1), rnd(B, 1), rnd(A, 3), rnd(A, 3), rnd(B, 3, 3), rnd(B, 3, 3)
    St[B - 1] = S[B - 1]                                       # a structure on its target: zero norm
    mask = dev_w = None
    w_f = RHO_F / A
    if masked:
        mask = (torch.rand(A, generator=g) < 0.7).float()
        mask[0] = 1.0
        dev_w = torch.tensor(1.0 / float(mask.sum()))
        w_f = RHO_F
    w_e, w_s = (1 - RHO_F) / B, RHO_S / B
    d = lambda t: None if t is None else put(t)                # noqa: E731
    out = K.periodic_loss(d(E), d(Et), d(F), d(Ft), w_e, w_f, S=d(S), St=d(St), w_s=w_s, mask=d(mask), w_f_dev=d(dev_w))
    f64 = lambda t: None if t is None else t.double()          # noqa: E731
    ref = C.periodic_loss(f64(E), f64(Et), f64(F), f64(Ft), w_e, w_f, S=f64(S), St=f64(St), w_s=w_s, mask=f64(mask),
                          w_f_dev=f64(dev_w))
    for name, got, want in zip(("loss", "gE", "gF", "gS"), out, ref):
        assert got.dtype == torch.float32 and got.shape == want.shape, name
        torch.testing.assert_close(got.cpu().double(), want, rtol=1e-6, atol=0.0, msg=lambda m, n=name: f"{n}: {m}")
    assert float(out[3][B - 1].abs().max()) == 0.0
    if masked:
        assert float(out[2][put(mask) == 0].abs().sum()) == 0.0
    # S = NULL: the force loss, bit for bit; and bit-repeatable with S
    loss0, gE0, gF0, gS0 = K.periodic_loss(d(E), d(Et), d(F), d(Ft), w_e, w_f, mask=d(mask), w_f_dev=d(dev_w))
    loss1, gE1, gF1 = K.force_loss(d(E), d(Et), d(F), d(Ft), w_e, w_f, mask=d(mask), w_f_dev=d(dev_w))
    assert gS0 is None and torch.equal(loss0, loss1) and torch.equal(gE0, gE1) and torch.equal(gF0, gF1)
    again = K.periodic_loss(d(E), d(Et), d(F), d(Ft), w_e, w_f, S=d(S), St=d(St), w_s=w_s, mask=d(mask), w_f_dev=d(dev_w))
    assert all(torch.equal(a, b) for a, b in zip(out, again))


# ------------------------------------------------------------------------------------------------------------------- steps
_PARAMS = {}


def _model(tag, direct=False):
    cfg = DT.direct_cfg(CFGS[tag], True) if direct else CFGS[tag]
    if (tag, direct) not in _PARAMS:
        _PARAMS[tag, direct] = PT.make_params(cfg)
    m = GemNet(**cfg, scale_file=SCALE_FILE)
    m.load_state_dict(GO.expand_to_reference_state_dict({k: v.float() for k, v in _PARAMS[tag, direct].items()}))
    return m.to(DEV)


def _builder(N, pbc):
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder
    return PeriodicGraphBuilder(N, P.CUTOFF, pbc=pbc, device=DEV)


def _targets(n_mol, n_atoms):
    return tuple(torch.tensor(t, dtype=torch.float32, device=DEV) for t in C.targets(n_mol, n_atoms))


def _frame(frame):
    return torch.tensor(frame[0], device=DEV), torch.tensor(frame[1], device=DEV)


def _padded_step(model, Z, N, pbc, frames, caps=None, direct=False, fused=True):
    e_cap, t_cap, deg, G = caps or C.capacities(frames)
    return PeriodicPaddedTrainStep(model, torch.tensor(Z, device=DEV).long(), torch.tensor(N, device=DEV), e_cap, t_cap,
                                   cell=torch.tensor(frames[0][1], device=DEV), pbc=pbc, max_in_degree=deg, n_groups=G,
                                   rho_force=RHO_F, rho_stress=0.0 if direct else RHO_S, fused_optimizer=fused)


def _attach(ts, builder, frame):
    R, cell = _frame(frame)
    ts.pad._fill(R, builder(R, cell, dtype=torch.int32), cell=cell)
    ts.attach_builder(builder)
    return ts


@pytest.mark.parametrize("tag,direct", [("wide", False), ("cfg", False), ("wide", True), ("cfg", True)])
def test_padded_step_equals_the_eager_step_on_the_unpadded_batch(tag, direct):
    """6 frames (3 for a direct-force model) with different list sizes through ONE graph, step_optimizer=False: loss and flat
    gradient of `step` against the eager PeriodicTrainStep on the unpadded batch, at the bars of the molecular twin
    (tests/test_gpu_padded.py: loss 2e-5, flat gradient 1e-5 of its norm — the weight-gradient contraction is split differently
    over the padded rows); then three optimizer steps on both sides: the trajectories stay together (the molecular test's bars)."""
    Z, N, pbc, frames = C.trajectory(C.BATCH, 3 if direct else C.FRAMES)
    base = _model(tag, direct)
    ts = _padded_step(copy.deepcopy(base), Z, N, pbc, frames, direct=direct)
    eager = PeriodicTrainStep(copy.deepcopy(base), rho_force=RHO_F, rho_stress=0.0 if direct else RHO_S, fused_optimizer=True)
    builder = _builder(N, pbc)
    Et, Ft, St = _targets(len(N), len(Z))
    tgt = dict(E=Et, F=Ft) if direct else dict(E=Et, F=Ft, S=St)
    Zd, Nd = torch.tensor(Z, device=DEV).long(), torch.tensor(N, device=DEV)
    graph, worst_g, worst_l = None, 0.0, 0.0
    for step_opt, use in ((False, frames), (True, frames[:3])):
        for s, frame in enumerate(use):
            R, cell = _frame(frame)
            idx = builder(R, cell, dtype=torch.int32)
            assert (idx["id_c"].shape[0], idx["id3_reduce_ca"].shape[0]) == C.sizes(frame)[:2]
            la = ts.step(R, idx, cell, Et, Ft, None if direct else St, step_optimizer=step_opt)
            ga = ts.buf.flat.clone()
            lb = eager(dict(Z=Zd, N=Nd, R=R.clone(), cell=cell.clone(), **idx), tgt, step_optimizer=step_opt)
            gb = eager.buf.flat.clone()
            torch.cuda.synchronize()
            graph = graph or ts._graph
            assert ts._graph is graph and graph is not None
            la, lb = float(la), float(lb)
            if step_opt:
                assert abs(la - lb) <= 2e-3 * abs(lb), (s, la, lb)
            else:
                rel = float((ga - gb).norm() / gb.norm())
                worst_g, worst_l = max(worst_g, rel), max(worst_l, abs(la - lb) / abs(lb))
                print(f"{tag} direct={direct} frame {s} sizes {C.sizes(frame)}: loss {la:.8f} / {lb:.8f}, |g - g_eager| / |g| = {rel:.2e}")
                assert float(gb.norm()) > 0 and bool(torch.isfinite(ga).all())
                assert abs(la - lb) <= 2e-5 * abs(lb), (s, la, lb)
                assert rel <= 1e-5, (s, rel)
    assert not ts.flag.tripped() and not eager.flag.tripped()
    pa = torch.cat([p.detach().reshape(-1) for p in ts.model.parameters()])
    pb = torch.cat([p.detach().reshape(-1) for p in eager.model.parameters()])
    drift = float((pa - pb).abs().max())
    print(f"{tag} direct={direct}: worst gradient deviation {worst_g:.2e}, worst loss deviation {worst_l:.2e}, parameters after three "
          f"optimizer steps differ by at most {drift:.2e}")
    assert any(not torch.equal(p, q) for p, q in zip(ts.model.parameters(), base.parameters()))      # the optimizer stepped
    # AdamW moves an entry by ~lr per step whatever the gradient's size: an entry whose gradient is fp32 noise may go the other
    # way on the two sides (2 x 3 steps x lr 1e-3 at most, tests/test_gpu_padded.py)
    assert drift <= 6.5e-3


@pytest.mark.parametrize("tag,direct", [("wide", False), ("wide", True)])
def test_in_graph_list_equals_handed_in_lists_bit_for_bit(tag, direct):
    """Two steps on copies of one model, the same frames: `step_positions` (list built inside the replay, no read-back) against
    `step` with the builder's own lists — torch.equal on the loss and the flat gradient at every frame; the build reports no
    error and the sizes of the CPU list."""
    Z, N, pbc, frames = C.trajectory(C.BATCH, 3 if direct else C.FRAMES)
    base = _model(tag, direct)
    builder = _builder(N, pbc)
    handed = _padded_step(copy.deepcopy(base), Z, N, pbc, frames, direct=direct)
    inside = _attach(_padded_step(copy.deepcopy(base), Z, N, pbc, frames, direct=direct), builder, frames[0])
    Et, Ft, St = _targets(len(N), len(Z))
    St = None if direct else St
    graph = None
    for s, frame in enumerate(frames):
        R, cell = _frame(frame)
        l0 = handed.step(R, builder(R, cell, dtype=torch.int32), cell, Et, Ft, St, step_optimizer=False)
        l1 = inside.step_positions(R, cell, Et, Ft, St, step_optimizer=False)
        torch.cuda.synchronize()
        assert inside.pad.index_error() == 0 and inside.pad.index_sizes() == C.sizes(frame)[:2], s
        assert bool(torch.isfinite(l1)) and float(handed.buf.flat.norm()) > 0
        assert torch.equal(l0, l1) and torch.equal(handed.buf.flat, inside.buf.flat), s
        graph = graph or inside._graph
        assert inside._graph is graph
    assert not inside.flag.tripped()


@pytest.mark.parametrize("fused", [True, False])
def test_outgrowing_the_capacities_does_not_move_the_parameters(fused):
    """Capacities that fit frame 0 but not the trajectory's largest frame.  The first frame that does not fit (named from the
    CPU lists) runs on the previous arrays: its gradient and loss are NaN, the optimizer (fused: on the device; eager: on the
    host) skips it — every parameter, Adam's moments and its step counter are those before the step — and the NEXT call raises
    ValueError naming the capacities, without falling back to the bf16 planes or capturing anew.  A handled path: nothing faults."""
    Z, N, pbc, frames = C.trajectory(C.BATCH, C.FRAMES)
    e0, t0, _ = C.sizes(frames[0])
    deg = max(C.sizes(f)[2] for f in frames)
    over = next(s for s in range(len(frames)) if C.sizes(frames[s])[0] > e0 or C.sizes(frames[s])[1] > t0)
    assert 1 <= over < len(frames) - 1
    assert max(C.sizes(f)[0] for f in frames) > e0 or max(C.sizes(f)[1] for f in frames) > t0
    model = _model("wide")
    builder = _builder(N, pbc)
    ts = _attach(_padded_step(model, Z, N, pbc, frames, caps=(e0, t0, deg, C.groups_for(frames, e0, deg)), fused=fused),
                 builder, frames[0])
    Et, Ft, St = _targets(len(N), len(Z))
    precision = model.matmul_precision
    params = lambda: [p.detach().clone() for p in model.parameters()]      # noqa: E731
    start = params()
    for s in range(over):
        R, cell = _frame(frames[s])
        loss = ts.step_positions(R, cell, Et, Ft, St)
        torch.cuda.synchronize()
        assert ts.pad.index_error() == 0 and bool(torch.isfinite(loss)), s
    graph = ts._graph
    before = params()
    assert any(not torch.equal(p, q) for p, q in zip(before, start))       # the fitting steps did move them
    moments = [t.clone() for t in (ts.fused.m, ts.fused.v, ts.fused.vmax, ts.fused.ema)] if fused else None
    steps = ts.fused.steps if fused else None
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        R, cell = _frame(frames[over])
        loss = ts.step_positions(R, cell, Et, Ft, St)
        torch.cuda.synchronize()
        E, T = C.sizes(frames[over])[:2]
        want = (1 if E > e0 else 0) | (2 if E <= e0 and T > t0 else 0)
        # (a build whose edges alone do not fit stops before it counts triplets: it reports E and T = 0)
        got = ts.pad.index_sizes()
        assert ts.pad.index_error() == want and got[0] == E and got[1] == (T if E <= e0 else 0)
        assert bool(torch.isnan(loss)) and bool(torch.isnan(ts.buf.flat).all())
        assert all(torch.equal(p, q) for p, q in zip(params(), before))
        if fused:
            assert all(torch.equal(a, b) for a, b in zip(moments, (ts.fused.m, ts.fused.v, ts.fused.vmax, ts.fused.ema)))
        R, cell = _frame(frames[over + 1])
        with pytest.raises(ValueError, match=rf"capacities \(e_cap {e0}, t_cap {t0}") as err:
            ts.step_positions(R, cell, Et, Ft, St)
        assert f"bits {want}" in str(err.value) and f"sizes {got}" in str(err.value)
        torch.cuda.synchronize()
    assert not [w for w in seen if "gemnet_pytorch_amd" in str(w.message)], [str(w.message) for w in seen]     # no fall-back
    assert all(torch.equal(p, q) for p, q in zip(params(), before))
    if fused:
        assert ts.fused.steps == steps                                     # the skipped step does not count
    assert model.matmul_precision == precision and ts._graph is graph and not ts.flag.tripped()
    with pytest.raises(ValueError, match="capacities"):                    # the report is sticky
        ts.step_positions(R, cell, Et, Ft, St)
    assert all(torch.equal(p, q) for p, q in zip(params(), before))


def test_the_capture_is_race_free_and_replays_the_eager_step():
    """The capture of `step_positions` (in-graph list + plan + forward + force graph + one-launch loss + backward + the poison
    launches) under the happens-before checker; its replay equals an eager run of the same padded step bit for bit."""
    Z, N, pbc, frames = C.trajectory(C.BATCH, C.FRAMES)
    base = _model("wide")
    builder = _builder(N, pbc)
    Et, Ft, St = _targets(len(N), len(Z))
    ts = _attach(_padded_step(copy.deepcopy(base), Z, N, pbc, frames), builder, frames[0])
    ts.check = True
    R, cell = _frame(frames[3])
    loss = ts.step_positions(R, cell, Et, Ft, St, step_optimizer=False)
    torch.cuda.synchronize()
    races, summary = ts.hb.races(), ts.hb.summary()
    print(ts.hb.format(races))
    assert not races
    assert summary["unrecorded_nodes"] == 0 and summary["unresolved_pointers"] == 0 and summary["ops"] > 50, summary
    assert ts.pad.index_error() == 0 and ts.pad.index_sizes() == C.sizes(frames[3])[:2]
    eager = _attach(_padded_step(copy.deepcopy(base), Z, N, pbc, frames), builder, frames[0])
    eager.inputs["R"][:eager.pad.A].copy_(R)
    eager._load(cell, Et, Ft, St)
    loss_e = eager._eager(eager.inputs, eager.targets)
    torch.cuda.synchronize()
    assert eager._graph is None and bool(torch.isfinite(loss))
    assert torch.equal(loss, loss_e) and torch.equal(ts.buf.flat, eager.buf.flat)
    assert np.isfinite(float(ts.buf.flat.norm())) and float(ts.buf.flat.norm()) > 0
