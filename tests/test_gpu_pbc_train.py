"""GPU: training GemNet-T on periodic batches (GemNet.periodic_training, training/periodic.py, csrc/pbc_train.hip) — the new
kernels against their fp64 restatements, the parameter gradients of the energy + force + stress loss against the gradient
oracle (tests/pbc_train_common.py), the fused training form against the composite closure, the large-cell limit against the
molecular training step, the captured step, and training-mode against eval-mode outputs.

The oracle costs ~10 s per configuration on the host (7 s of it the central-difference forces and stress of
pbc_common.fd_forces_stress, the yardstick of tests/test_gpu_pbc.py as well); it is computed once per configuration."""
import copy
from collections import Counter

import numpy as np
import pytest
import torch

import pbc_common as P
import pbc_train_common as PT
from conftest import SCALE_FILE
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd import ops, ops_train
from gemnet_pytorch_amd.model.gemnet import GemNet
from gemnet_pytorch_amd.training.ddp import TrainStep
from gemnet_pytorch_amd.training.periodic import PeriodicTrainStep
from oracle import gemnet_oracle as GO
from redzone import put, redzone_on_request  # noqa: F401  (the kernel-level tests below ask for `redzone`: they run under the red-zone harness)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFGS = {"cfg": P.CFG, "wide": PT.CFG_WIDE}


def close(a, b, rtol, atol):
    torch.testing.assert_close(a.detach().cpu().double(), b.detach().cpu().double(), rtol=rtol, atol=atol)


f32 = lambda t: put(t.float())       # noqa: E731


# ---------------------------------------------------------------------------------------------------------------- kernels
def test_edge_vector_geometry_kernels(redzone):
    """csrc/pbc_train.hip: distance and angle value / first adjoint / tangent on edge vectors against fp64 autograd of the
    reference formulas (tests/pbc_train_common.py), E = 67, T = 131 (no full wavefront), one exactly collinear triplet (the
    max(|u x v|, 1e-9) clamp) and a T = 0 call.  Bars: those of test_gpu_kernels.test_twice_differentiable_geometry_kernels."""
    g = torch.Generator().manual_seed(31)
    E, T = 67, 131
    V = ((torch.rand(E, 3, generator=g, dtype=torch.float64) - 0.5) * 5.0).float().double()
    V[1] = 2.0 * V[0]                                       # edges 0 and 1 parallel (exact in fp32)
    tV = torch.randn(E, 3, generator=g, dtype=torch.float64).float().double()
    pairs = torch.stack([torch.randperm(E, generator=g)[:2] for _ in range(T)]).int()
    pairs[0] = torch.tensor([0, 1])                         # the collinear triplet
    red, exp = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
    d = put
    gD = torch.randn(E, generator=g, dtype=torch.float64).float().double()
    close(K.dist_vec_fwd(f32(V)), PT.dist_vec_fwd(V), rtol=1e-6, atol=1e-6)
    close(K.dist_vec_bwd(f32(gD), f32(V)), PT.dist_vec_bwd(gD, V), rtol=1e-5, atol=1e-5)
    close(K.dist_vec_jvp(f32(V), f32(tV)), PT.dist_vec_jvp(V, tV), rtol=1e-5, atol=1e-5)
    gth = torch.randn(T, generator=g, dtype=torch.float64).float().double()
    th = PT.angle_vec_fwd(V, red, exp)
    close(K.angle_vec_fwd(f32(V), d(red), d(exp)), th, rtol=1e-5, atol=2e-6)
    # derivatives divide by sin(theta): elementwise on the well-conditioned triplets, finite everywhere (incl. the collinear one)
    well = torch.sin(th) >= 0.3
    well[0] = False
    assert int(well.sum()) > T // 2
    wd = well.to(DEV)
    Gu, Gv = K.angle_vec_bwd(f32(gth), f32(V), d(red), d(exp))
    rGu, rGv = PT.angle_vec_bwd(gth, V, red, exp)
    sc = float(rGu[well].abs().max())
    close(Gu[wd], rGu[well], rtol=1e-3, atol=2e-4 * sc)
    close(Gv[wd], rGv[well], rtol=1e-3, atol=2e-4 * sc)
    assert torch.isfinite(Gu).all() and torch.isfinite(Gv).all()
    thd = K.angle_vec_jvp(f32(V), f32(tV), d(red), d(exp))
    rthd = PT.angle_vec_jvp(V, tV, red, exp)
    close(thd[wd], rthd[well], rtol=1e-3, atol=2e-4 * float(rthd[well].abs().max()))
    assert torch.isfinite(thd).all()
    # bit-repeatable
    assert torch.equal(thd, K.angle_vec_jvp(f32(V), f32(tV), d(red), d(exp)))
    # T = 0 / E = 0: success without a launch
    none = torch.zeros(0, dtype=torch.int32, device=DEV)
    assert K.angle_vec_fwd(f32(V), none, none).shape == (0,)
    assert K.angle_vec_jvp(f32(V), f32(tV), none, none).shape == (0,)
    assert all(t.shape == (0, 3) for t in K.angle_vec_bwd(f32(gth[:0]), f32(V), none, none))
    empty = torch.zeros(0, 3, device=DEV)
    assert K.dist_vec_fwd(empty).shape == (0,) and K.dist_vec_jvp(empty, empty).shape == (0,)


@pytest.mark.parametrize("with_stress", [True, False])
def test_force_stress_adjoint_kernel(with_stress, redzone):
    """gn_pbc_force_stress_adj_f32 against fp64 autograd of an ATen forces + stress composite, 3 structures; gS given / NULL."""
    g = torch.Generator().manual_seed(5)
    N = [3, 5, 4]
    E = 67
    off = np.concatenate([[0], np.cumsum(N)])
    batch_seg = torch.tensor(np.repeat(np.arange(3), N)).int()
    mol = torch.randint(0, 3, (E,), generator=g)
    id_a = torch.tensor([off[m] + int(torch.randint(0, N[m], (1,), generator=g)) for m in mol.tolist()]).int()
    id_c = torch.tensor([off[m] + int(torch.randint(0, N[m], (1,), generator=g)) for m in mol.tolist()]).int()
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()      # noqa: E731
    V, gF, gS = rnd(E, 3), rnd(12, 3), rnd(3, 3, 3)
    cell = (rnd(3, 3, 3) * 0.4 + torch.eye(3, dtype=torch.float64) * 3.0).float().double()
    G = rnd(E, 3).requires_grad_(True)
    F = torch.zeros(12, 3, dtype=torch.float64).index_add(0, id_a.long(), G).index_add(0, id_c.long(), -G)
    b = batch_seg.long()[id_a.long()]
    S = -torch.zeros(3, 3, 3, dtype=torch.float64).index_add(0, b, V[:, :, None] * G[:, None, :]) \
        / torch.linalg.det(cell).abs()[:, None, None]
    (ref,) = torch.autograd.grad((F * gF).sum() + ((S * gS).sum() if with_stress else 0.0), G)
    d = put
    out = K.pbc_force_stress_adj(f32(gF), f32(gS) if with_stress else None, f32(V), d(id_c), d(id_a), d(batch_seg), f32(cell))
    close(out, ref, rtol=1e-5, atol=1e-5)
    close(out, PT.pbc_force_stress_adj(gF, gS if with_stress else None, V, id_c, id_a, batch_seg, cell), rtol=1e-5, atol=1e-5)
    assert torch.equal(out, K.pbc_force_stress_adj(f32(gF), f32(gS) if with_stress else None, f32(V), d(id_c), d(id_a),
                                                   d(batch_seg), f32(cell)))


# ------------------------------------------------------------------------------------------------------------------ model
_PARAMS, _REF = {}, {}


def _params(tag):
    if tag not in _PARAMS:
        _PARAMS[tag] = PT.make_params(CFGS[tag])
    return _PARAMS[tag]


def _model(tag):
    m = GemNet(**CFGS[tag], scale_file=SCALE_FILE)
    m.load_state_dict(GO.expand_to_reference_state_dict({k: v.float() for k, v in _params(tag).items()}))
    return m.to(DEV)


def _reference(tag):
    """The oracle of the 4-structure batch for configuration `tag` (computed once, shared, never modified)."""
    if tag not in _REF:
        _REF[tag] = PT.oracle(_params(tag), CFGS[tag], PT.structures(), PT.trainable(_model(tag), _params(tag)))
    return _REF[tag]


def _targets(ref=None, stress=True):
    if ref is not None:
        t = dict(E=ref["Et"], F=ref["Ft"], S=ref["St"])
    else:
        oE, oF, oS = PT.offsets(PT.structures())
        t = dict(E=torch.tensor(oE), F=torch.tensor(oF), S=torch.tensor(oS))
    return {k: v.float().to(DEV) for k, v in t.items() if stress or k != "S"}


def _batch():
    return PT.batch(PT.structures(), device=DEV, dtype=torch.float32)


def _gradients(ts):
    return {n: p.grad.detach().double().cpu() for n, p in ts.model.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("tag", ["cfg", "wide"])
def test_parameter_gradients_match_the_oracle(tag, monkeypatch):
    """[small, triclinic, slab, cubic1], rho_force = 0.9, rho_stress = 0.05, fp32 on the device against the fp64 gradient oracle.
    Bars: the molecular training bar of test_gpu_model.test_training_gradients_parity — per-parameter norms rtol 2e-3 with
    atol 1e-6 max|g_ref|, |g - g_ref| <= 2e-3 |g_ref| + the same atol per parameter, loss rtol 2e-5.  `wide`: the widths of
    kernels.bil_train_supported — the fused bilinear training Function, the chain programs and the tangent kernels must have
    run.  `cfg` has 8-wide embeddings, which are no shapes of the split-operand chain kernel: on the device such a model trains
    on the composite closure as a whole (GemNet._train2_widths_ok), for molecules and periodic batches alike.
    Measured on MI355X (worst |g - g_ref| / bar): cfg 0.003, wide 0.007; loss 3.4e-7 / 1.7e-6 relative."""
    ref = _reference(tag)
    cnt = Counter()
    for mod, name in ((ops_train, "bilinear"), (ops_train, "stack"), (K, "angle_vec_jvp"), (K, "dist_vec_jvp"),
                      (K, "pbc_force_stress_adj"), (K, "chain")):
        f = getattr(mod, name)
        monkeypatch.setattr(mod, name, (lambda *a, _f=f, _n=name, **k: (cnt.update([_n]), _f(*a, **k))[1]))
    ts = PeriodicTrainStep(_model(tag), rho_force=PT.RHO_FORCE, rho_stress=PT.RHO_STRESS, fused_optimizer=True)
    loss = float(ts(_batch(), _targets(ref), step_optimizer=False))
    torch.cuda.synchronize()
    g, gref = _gradients(ts), ref["grads"]
    assert set(g) == set(gref)
    gmax = max(float(v.norm()) for v in gref.values())
    atol = 1e-6 * gmax
    ratio = {n: float((g[n] - gref[n]).norm()) / (2e-3 * float(gref[n].norm()) + atol) for n in gref}
    worst = max(ratio, key=ratio.get)
    print(f"{tag}: loss {loss:.8f} (oracle {ref['loss']:.8f}); worst |g - g_ref| / (2e-3 |g_ref| + 1e-6 max|g_ref|) = "
          f"{ratio[worst]:.3f} ({worst}); launches {dict(cnt)}")
    np.testing.assert_allclose(loss, ref["loss"], rtol=2e-5)
    names = sorted(gref)
    np.testing.assert_allclose([float(g[n].norm()) for n in names], [float(gref[n].norm()) for n in names], rtol=2e-3, atol=atol)
    assert ratio[worst] <= 1.0, (worst, ratio[worst])
    assert cnt["pbc_force_stress_adj"] == 1, cnt
    if tag == "wide":
        assert K.bil_train_supported(7, CFGS[tag]["emb_size_trip"], CFGS[tag]["emb_size_cbf"])
        assert cnt["angle_vec_jvp"] == 1 and cnt["dist_vec_jvp"] == 1 and cnt["chain"] > 0 and cnt["stack"] > 0, cnt
        assert cnt["bilinear"] == CFGS[tag]["num_blocks"], cnt
    else:
        assert cnt["chain"] == 0 and cnt["stack"] == 0 and cnt["angle_vec_jvp"] == 0, cnt


@pytest.mark.parametrize("tag", ["cfg", "wide"])
def test_fused_training_form_equals_composite_closure(tag, monkeypatch):
    """ops.USE_TRAIN2 on / off on the same weights; the bars of tests/test_gpu_qtrain.py: loss 2e-5, flat gradient 2e-3 of the
    norm (worst element 5e-3 of the largest)."""
    base = _model(tag)
    flat, loss = {}, {}
    for form in (True, False):
        monkeypatch.setattr(ops, "USE_TRAIN2", form)
        ts = PeriodicTrainStep(copy.deepcopy(base), rho_force=PT.RHO_FORCE, rho_stress=PT.RHO_STRESS, fused_optimizer=True)
        loss[form] = float(ts(_batch(), _targets(), step_optimizer=False))
        torch.cuda.synchronize()
        flat[form] = ts.buf.flat.clone()
        assert bool(torch.isfinite(flat[form]).all())
    rel = float((flat[True] - flat[False]).norm() / flat[False].norm())
    worst = float((flat[True] - flat[False]).abs().max() / flat[False].abs().max())
    print(f"{tag}: loss {loss[True]:.8f} / {loss[False]:.8f}; fused vs composite: {rel:.2e} of the norm, worst element {worst:.2e}")
    assert abs(loss[True] - loss[False]) <= 2e-5 * abs(loss[False])
    assert rel <= 2e-3 and worst <= 5e-3


def test_large_cell_is_the_molecular_training_step():
    """A 30 A cube holds no image within the cutoff: the periodic index arrays are the molecular ones, the training-mode E is
    bit-identical to the molecular training-mode E, and the parameter gradients of the energy + force loss are the molecular
    TrainStep's up to the order of the geometry-adjoint sums (per edge first, then per atom).  Measured on MI355X:
    |g_periodic - g_molecular| = 2.4e-8 |g| (loss identical to the last digit printed)."""
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder
    structs = [(s[0], s[1], np.eye(3) * 30.0, np.array([True] * 3)) for s in PT.structures()[:3]]
    R = torch.tensor(np.concatenate([s[0] for s in structs]), dtype=torch.float32, device=DEV)
    N = [len(s[0]) for s in structs]
    cell = torch.tensor(np.stack([s[2] for s in structs]), dtype=torch.float32, device=DEV)
    idx = PeriodicGraphBuilder(N, P.CUTOFF, device=DEV)(R, cell)
    assert int(idx["cell_offsets"].abs().max()) == 0 and idx["id_a"].shape[0] > 0
    base = dict(R=R, Z=torch.tensor(np.concatenate([s[1] for s in structs]), device=DEV).long(), N=torch.tensor(N, device=DEV))
    mol = dict(base, **{k: v for k, v in idx.items() if k != "cell_offsets"})
    per = dict(base, **idx, cell=cell)
    targets = _targets(stress=False)
    targets = dict(E=targets["E"][:3], F=targets["F"][:R.shape[0]])
    model = _model("wide")
    tm = TrainStep(copy.deepcopy(model), rho_force=PT.RHO_FORCE, fused_optimizer=True)
    tp = PeriodicTrainStep(copy.deepcopy(model), rho_force=PT.RHO_FORCE, fused_optimizer=True)
    E0, _ = tm.model.train()(dict(mol))
    E1, _ = tp.model.train()(dict(per))
    assert torch.equal(E0, E1)
    lm = float(tm(mol, targets, step_optimizer=False))
    lp = float(tp(per, targets, step_optimizer=False))
    torch.cuda.synchronize()
    gm, gp = tm.buf.flat, tp.buf.flat
    rel = float((gp - gm).norm() / gm.norm())
    print(f"large cell: loss {lp:.8f} / molecular {lm:.8f}; |g_periodic - g_molecular| / |g| = {rel:.3e}")
    assert abs(lp - lm) <= 2e-6 * abs(lm)
    assert rel <= LARGE_CELL_BAR


# 10 x the measured difference (2.4e-8, see the test); never to be set above 2e-4, a tenth of the oracle bar
LARGE_CELL_BAR = 2.5e-7


def test_captured_step_is_clean_bit_reproducible_and_equals_eager():
    """PeriodicTrainStep(fused_optimizer=True, rho_stress > 0).capture(check=True): the happens-before checker sees every node,
    resolves every pointer and finds no race; four replays give the eager step's flat gradient bit for bit; three optimizer
    steps replayed equal three eager steps."""
    base = _model("wide")
    inputs, targets = _batch(), _targets()
    kw = dict(rho_force=PT.RHO_FORCE, rho_stress=PT.RHO_STRESS, fused_optimizer=True)
    eager = PeriodicTrainStep(copy.deepcopy(base), **kw)
    eager(inputs, targets, step_optimizer=False)
    torch.cuda.synchronize()
    ref = eager.buf.flat.clone()
    cap = PeriodicTrainStep(copy.deepcopy(base), **kw)
    cap_inputs = _batch()
    cap.capture(cap_inputs, targets, check=True)
    races, summary = cap.hb.races(), cap.hb.summary()
    print(cap.hb.format(races))
    assert not races
    assert summary["unrecorded_nodes"] == 0 and summary["unresolved_pointers"] == 0 and summary["ops"] > 50, summary
    for _ in range(4):
        cap(cap_inputs, targets, step_optimizer=False)
        torch.cuda.synchronize()
        assert torch.equal(cap.buf.flat, ref)
    le, lc = [], []
    for _ in range(3):
        le.append(float(eager(inputs, targets)))
        lc.append(float(cap(cap_inputs, targets)))
    torch.cuda.synchronize()
    assert le == lc, (le, lc)
    for p, q in zip(eager.model.parameters(), cap.model.parameters()):
        assert torch.equal(p, q)
    assert any(not torch.equal(p, q) for p, q in zip(cap.model.parameters(), base.parameters()))     # the optimizer stepped


def test_training_mode_outputs_and_the_switch():
    """Training-mode (E, F, S) — autograd graph to the parameters — against eval-mode (E, F, S) of the same weights, within the
    bars of test_gpu_pbc.test_batch_of_structures_equals_single_runs; eval outputs do not depend on the switch, bit for bit."""
    model = _model("cfg")
    E0, F0, S0 = model.eval()(_batch(), stress=True)
    model.periodic_training = True
    E1, F1, S1 = model(_batch(), stress=True)
    assert torch.equal(E0, E1) and torch.equal(F0, F1) and torch.equal(S0, S1)
    assert not (E1.requires_grad or F1.requires_grad or S1.requires_grad)
    Et, Ft, St = model.train()(_batch(), stress=True)
    assert Et.requires_grad and Ft.requires_grad and St.requires_grad
    E2, F2 = model(_batch())
    assert torch.equal(E2, Et) and torch.equal(F2, Ft)
    torch.cuda.synchronize()
    e, f, s = (t.double().cpu().numpy() for t in (E0, F0, S0))
    Et, Ft, St = (t.detach().double().cpu().numpy() for t in (Et, Ft, St))
    print("train vs eval:", np.abs(Et - e).max(), np.abs(Ft - f).max(), np.abs(St - s).max())
    assert (np.abs(Et - e) <= 1e-5 * np.maximum(1.0, np.abs(e))).all()
    assert np.abs(Ft - f).max() <= 1e-5 * max(1.0, np.abs(f).max())
    assert np.abs(St - s).max() <= 1e-5 * max(1e-2, np.abs(s).max())
    model.periodic_training = False
    with pytest.raises(NotImplementedError, match="periodic_training"):
        model(_batch())
