"""GPU: periodic TRAINING on cells with a height below the cutoff, sheared cells and a left-handed one — batch H =
pbc_train_common.HARD = [bcc_pert, thin, skewed, skewed_lh] (10 atoms, 74 edges, 598 triplets: self-image edges, image ranges up
to |n| = 3, triplets at exactly theta = 0 and pi, det < 0) and bcc alone.  The second-order sweep of the default training path
(csrc/pbc_train.hip, the tangent kernels of the bilinear layer, gn_direct_force_bwd_f32, the captured and the padded step with
its in-graph image list) against float64.

Reference of GemNet-T: the float64 emulated step (pbc_train_common.emulate) of the same float32-representable weights and
inputs, run on the host in this process (~1 s); tests/test_pbc_train_cells_cpu.py ties that step to the cluster oracle on these
cells to 1e-9 of the largest gradient.  The targets are the float64 step's own E, F, S plus pbc_train_common.offsets.
Reference of GemNet-dT: the exact-autograd cluster oracle itself (pbc_direct_train_common.oracle, ~1 s).  References are
computed once per case and never modified."""
import copy
import functools
from collections import Counter

import numpy as np
import pytest
import torch

import pbc_common as P
import pbc_direct_train_common as DT
import pbc_padded_train_common as C
import pbc_train_common as PT
import test_gpu_pbc_padded_train as TP
from conftest import SCALE_FILE
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd import ops, ops_train
from gemnet_pytorch_amd.model.gemnet import GemNet
from gemnet_pytorch_amd.training.periodic import PeriodicTrainStep
from oracle import gemnet_oracle as GO
from redzone import put, redzone_on_request  # noqa: F401  (the kernel-level tests below ask for `redzone`: they run under the red-zone harness)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFGS = {"cfg": P.CFG, "wide": PT.CFG_WIDE}
BATCHES = {"H": PT.HARD, "bcc": ("bcc",)}
WEIGHTS = {"default": (PT.RHO_FORCE, PT.RHO_STRESS), "stress": (0.0, 1.0)}


def close(a, b, rtol, atol):
    torch.testing.assert_close(a.detach().cpu().double(), b.detach().cpu().double(), rtol=rtol, atol=atol)


f32 = lambda t: put(t.float())       # noqa: E731


# ---------------------------------------------------------------------------------------------------------------- kernels
@functools.lru_cache(maxsize=None)
def _kernel_case():
    """V (float32-exact, held in float64), index arrays and cells of [bcc, thin, skewed_lh] from the brute-force list, the rows
    at exactly theta = 0 / pi, and fixed random cotangents and tangents."""
    V, idx, cell, at0, atpi = PT.collinear_rows([P.structure(k) for k in ("bcc", "thin", "skewed_lh")])
    g = torch.Generator().manual_seed(17)
    E, T = len(V), len(idx["id3_reduce_ca"])
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()      # noqa: E731
    return dict(V=torch.tensor(V, dtype=torch.float64), idx=idx, cell=torch.tensor(cell), at0=at0, atpi=atpi,
                tV=rnd(E, 3), gD=rnd(E), gth=rnd(T), gF=rnd(len(idx["batch_seg"]), 3), gS=rnd(len(cell), 3, 3))


def test_geometry_kernels_on_the_edge_vectors_of_real_cells(redzone):
    """gn_dist_vec_* / gn_angle_vec_* on the edge vectors and triplets of [bcc, thin, skewed_lh] (E = 60, T = 546), random
    cotangents and tangent, against the float64 restatements of tests/pbc_train_common.py under the bars of
    test_gpu_pbc_train.test_edge_vector_geometry_kernels: elementwise where sin(theta) >= 0.3 (more than a third of the rows),
    finite everywhere, bit-repeatable.  The 8 rows at exactly theta = 0 and the 44 at exactly pi (counted in
    tests/test_pbc_train_cells_cpu.py) have an exactly zero cross product on both sides: there the kernel must take the clamp
    like the restatement — adjoint rows g dtheta/du = -(1e-9 / (u.v)^2) g v, a product of a few float32 roundings without any
    cancellation: 1e-5 relative, elementwise; the tangent is the sum of six such products against the tangent's components:
    1e-5 of the sum of their magnitudes (measured on MI355X: 1.8e-7; |thdot| <= 5.7e-10 on those rows)."""
    c = _kernel_case()
    V, tV, idx = c["V"], c["tV"], c["idx"]
    red, exp = torch.tensor(idx["id3_reduce_ca"]).int(), torch.tensor(idx["id3_expand_ba"]).int()
    E, T = V.shape[0], red.shape[0]
    assert (E, T) == (60, 546) and len(c["at0"]) == 8 and len(c["atpi"]) == 44
    d = put
    close(K.dist_vec_fwd(f32(V)), PT.dist_vec_fwd(V), rtol=1e-6, atol=1e-6)
    close(K.dist_vec_bwd(f32(c["gD"]), f32(V)), PT.dist_vec_bwd(c["gD"], V), rtol=1e-5, atol=1e-5)
    close(K.dist_vec_jvp(f32(V), f32(tV)), PT.dist_vec_jvp(V, tV), rtol=1e-5, atol=1e-5)
    assert torch.equal(K.dist_vec_fwd(f32(V)), K.dist_vec_fwd(f32(V)))
    assert torch.equal(K.dist_vec_bwd(f32(c["gD"]), f32(V)), K.dist_vec_bwd(f32(c["gD"]), f32(V)))
    assert torch.equal(K.dist_vec_jvp(f32(V), f32(tV)), K.dist_vec_jvp(f32(V), f32(tV)))
    th = PT.angle_vec_fwd(V, red, exp)
    close(K.angle_vec_fwd(f32(V), d(red), d(exp)), th, rtol=1e-5, atol=2e-6)
    well = torch.sin(th) >= 0.3
    col = torch.tensor(np.concatenate([c["at0"], c["atpi"]]))
    assert int(well.sum()) > T // 3 and not bool(well[col].any())
    wd = well.to(DEV)
    gth = c["gth"]
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
    # the exactly collinear rows: the clamp, as in the restatement
    cd = col.to(DEV)
    assert float(rGu[col].abs().max()) < 1e-8 * float(gth.abs().max()) and float(rGu[col].abs().max()) > 0
    close(Gu[cd], rGu[col], rtol=1e-5, atol=0.0)
    close(Gv[cd], rGv[col], rtol=1e-5, atol=0.0)
    one_u, one_v = PT.angle_vec_bwd(torch.ones(T, dtype=torch.float64), V, red, exp)
    m = (one_u.abs() * tV[red.long()].abs()).sum(1) + (one_v.abs() * tV[exp.long()].abs()).sum(1)
    err = (thd.cpu().double() - rthd).abs()
    print(f"collinear rows: worst |thdot - ref| / sum|terms| = {float((err[col] / m[col]).max()):.2e}; max |thdot| there "
          f"{float(thd[cd].abs().max()):.2e}; well-conditioned rows {int(well.sum())} of {T}")
    assert bool((err[col] <= 1e-5 * m[col]).all())
    # bit-repeatable
    assert torch.equal(thd, K.angle_vec_jvp(f32(V), f32(tV), d(red), d(exp)))
    Gu2, Gv2 = K.angle_vec_bwd(f32(gth), f32(V), d(red), d(exp))
    assert torch.equal(Gu, Gu2) and torch.equal(Gv, Gv2)
    assert torch.equal(K.angle_vec_fwd(f32(V), d(red), d(exp)), K.angle_vec_fwd(f32(V), d(red), d(exp)))


@pytest.mark.parametrize("with_stress", [True, False])
def test_force_stress_adjoint_kernel_on_self_image_edges_and_a_left_handed_cell(with_stress, redzone):
    """gn_pbc_force_stress_adj_f32 on the edges of [bcc, thin, skewed_lh]: 20 self-image edges (id_a == id_c: the force part of
    the adjoint vanishes exactly, the stress part does not) and det(cell) < 0 for the third structure (1 / |det|); gS given /
    NULL; against float64 autograd of the forces + stress composite, the bars of test_gpu_pbc_train.test_force_stress_adjoint_kernel."""
    c = _kernel_case()
    V, idx, cell, gF, gS = c["V"], c["idx"], c["cell"], c["gF"], c["gS"]
    id_a, id_c, batch_seg = (torch.tensor(idx[k]).int() for k in ("id_a", "id_c", "batch_seg"))
    own = id_a == id_c
    assert int(own.sum()) == 20 and float(torch.linalg.det(cell)[2]) < 0 < float(torch.linalg.det(cell)[0])
    A, B = len(batch_seg), len(cell)
    G = torch.zeros(V.shape[0], 3, dtype=torch.float64, requires_grad=True)
    F = torch.zeros(A, 3, dtype=torch.float64).index_add(0, id_a.long(), G).index_add(0, id_c.long(), -G)
    b = batch_seg.long()[id_a.long()]
    S = -torch.zeros(B, 3, 3, dtype=torch.float64).index_add(0, b, V[:, :, None] * G[:, None, :]) \
        / torch.linalg.det(cell).abs()[:, None, None]
    (ref,) = torch.autograd.grad((F * gF).sum() + ((S * gS).sum() if with_stress else 0.0), G)
    d = put
    args = (f32(gF), f32(gS) if with_stress else None, f32(V), d(id_c), d(id_a), d(batch_seg), f32(cell))
    out = K.pbc_force_stress_adj(*args)
    close(out, ref, rtol=1e-5, atol=1e-5)
    close(out, PT.pbc_force_stress_adj(gF, gS if with_stress else None, V, id_c, id_a, batch_seg, cell), rtol=1e-5, atol=1e-5)
    od = own.to(DEV)
    if with_stress:
        assert float(ref[own].abs().max()) > 1e-3 and float(out[od].abs().max()) > 1e-3
        # the left-handed structure's rows carry the sign of 1 / |det|: a signed determinant flips them, far outside the bar
        lh = b == 2
        assert float((2 * (ref[lh] - gF[id_a.long()][lh] + gF[id_c.long()][lh])).abs().max()) > 1e-2
    else:
        assert float(out[od].abs().max()) == 0.0
    assert torch.equal(out, K.pbc_force_stress_adj(*args))


# ------------------------------------------------------------------------------------------------------------------ model
@functools.lru_cache(maxsize=None)
def _params(tag):
    """The weights, rounded through float32: what the device model holds, in float64."""
    return {k: v.float().double() for k, v in PT.make_params(CFGS[tag]).items()}


@functools.lru_cache(maxsize=None)
def _structs(batch):
    structs = [P.f32_round(s) for s in PT.hard_structures(BATCHES[batch])]
    R, Z, N, cell, pbc = P.arrays(structs)
    assert P.cutoff_margin_ok(R, N, cell, pbc, margin=1e-5)
    return structs


def _model(tag):
    m = GemNet(**CFGS[tag], scale_file=SCALE_FILE)
    m.load_state_dict(GO.expand_to_reference_state_dict({k: v.float() for k, v in _params(tag).items()}))
    return m.to(DEV)


def _host_model(tag):
    m = GemNet(**CFGS[tag], scale_file=SCALE_FILE).double()
    m.load_state_dict(GO.expand_to_reference_state_dict(_params(tag)), strict=True)
    m._check_inputs = lambda R: None
    return m


@functools.lru_cache(maxsize=None)
def _host_outputs(tag, batch):
    """Training-mode (E, F, S) of the float64 emulated model and the targets built on them."""
    structs = _structs(batch)
    with PT.emulate():
        model = _host_model(tag).train()
        model.periodic_training = True
        E, F, S = (t.detach() for t in model(PT.batch(structs), stress=True))
    oE, oF, oS = PT.offsets(structs)
    return dict(E=E, F=F, S=S, Et=E + torch.tensor(oE), Ft=F + torch.tensor(oF), St=S + torch.tensor(oS))


@functools.lru_cache(maxsize=None)
def _reference(tag, batch, weights):
    """The float64 emulated step -> dict(loss, grads {name: tensor}) + the outputs and targets of `_host_outputs`."""
    out = _host_outputs(tag, batch)
    rho_f, rho_s = WEIGHTS[weights]
    with PT.emulate():
        model = _host_model(tag).train()
        ts = PeriodicTrainStep(model, rho_force=rho_f, rho_stress=rho_s)
        loss = float(ts._forward_backward(PT.batch(_structs(batch)), dict(E=out["Et"], F=out["Ft"], S=out["St"])))
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    return dict(out, loss=loss, grads=grads)


def _targets(ref):
    return {k: ref[k + "t"].float().to(DEV) for k in ("E", "F", "S")}


def _batch(batch):
    return PT.batch(_structs(batch), device=DEV, dtype=torch.float32)


@pytest.mark.parametrize("weights", list(WEIGHTS))
@pytest.mark.parametrize("tag,batch", [("cfg", "H"), ("wide", "H"), ("wide", "bcc")])
def test_parameter_gradients_match_the_float64_step(tag, batch, weights, monkeypatch):
    """fp32 on the device against the float64 emulated step, at (rho_force, rho_stress) = (0.9, 0.05) and at the stress-only
    weights (0, 1) — at the default weights the stress adjoint is 0.05 of the loss, and a det for |det| there moves the
    gradient by only 2.4 x the bar, at (0, 1) by 43 x (tests/test_pbc_train_cells_cpu.py).  Bars of
    test_gpu_pbc_train.test_parameter_gradients_match_the_oracle, unchanged: per-parameter norms rtol 2e-3 with atol 1e-6
    max|g_ref|, |g - g_ref| <= 2e-3 |g_ref,n| + the same atol per parameter, loss rtol 2e-5; `wide`: the launcher counts of that
    test (the fused bilinear training Function, the chain programs and the tangent kernels ran).
    Measured on MI355X (worst |g - g_ref| / bar; loss relative), default / stress-only weights: cfg H 0.0037; 1.1e-7 / 0.0012;
    1.6e-7, wide H 0.0043; 2.3e-7 / 0.0017; 2.6e-7, wide bcc 0.0037; 1.0e-7 / 0.0017; 5.4e-7 — no bar needed raising."""
    ref = _reference(tag, batch, weights)          # (before the counters: the emulated step calls the same Python entry points)
    rho_f, rho_s = WEIGHTS[weights]
    cnt = Counter()
    for mod, name in ((ops_train, "bilinear"), (ops_train, "stack"), (K, "angle_vec_jvp"), (K, "dist_vec_jvp"),
                      (K, "pbc_force_stress_adj"), (K, "chain")):
        f = getattr(mod, name)
        monkeypatch.setattr(mod, name, (lambda *a, _f=f, _n=name, **k: (cnt.update([_n]), _f(*a, **k))[1]))
    ts = PeriodicTrainStep(_model(tag), rho_force=rho_f, rho_stress=rho_s, fused_optimizer=True)
    loss = float(ts(_batch(batch), _targets(ref), step_optimizer=False))
    torch.cuda.synchronize()
    g = {n: p.grad.detach().double().cpu() for n, p in ts.model.named_parameters() if p.requires_grad}
    gref = ref["grads"]
    assert set(g) == set(gref)
    gmax = max(float(v.norm()) for v in gref.values())
    atol = 1e-6 * gmax
    ratio = {n: float((g[n] - gref[n]).norm()) / (2e-3 * float(gref[n].norm()) + atol) for n in gref}
    worst = max(ratio, key=ratio.get)
    print(f"{tag} {batch} {weights}: loss {loss:.8f} (float64 step {ref['loss']:.8f}, rel {abs(loss - ref['loss']) / abs(ref['loss']):.2e}); "
          f"worst |g - g_ref| / (2e-3 |g_ref| + 1e-6 max|g_ref|) = {ratio[worst]:.4f} ({worst}); launches {dict(cnt)}")
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


@pytest.mark.parametrize("tag,batch", [("cfg", "H"), ("wide", "H"), ("cfg", "bcc"), ("wide", "bcc")])
def test_training_mode_outputs(tag, batch):
    """Training-mode (E, F, S) on the device against (a) the float64 step's outputs and (b) the model's own eval-mode outputs,
    both under the bars of test_gpu_pbc_train.test_training_mode_outputs_and_the_switch.  On bcc the forces vanish by symmetry
    (the cluster oracle's are 1e-12): whatever is visible is rounding that fails to cancel over the images, and it must stay
    below 1e-5 max(1, max|S| |det|^(1/3)).  Measured on MI355X, worst over cfg / wide: H against the float64 step E 2.4e-6,
    F 2.9e-6 (max|F| 12.4), S 2.6e-6 (max|S| 2.4), against eval mode 1.2e-6 / 1.4e-6 / 3.3e-6; bcc max|F| 1.2e-7."""
    ref = _host_outputs(tag, batch)
    model = _model(tag)
    E0, F0, S0 = model.eval()(_batch(batch), stress=True)
    model.periodic_training = True
    Et, Ft, St = model.train()(_batch(batch), stress=True)
    assert Et.requires_grad and Ft.requires_grad and St.requires_grad
    torch.cuda.synchronize()
    e, f, s = (t.double().cpu().numpy() for t in (E0, F0, S0))
    Et, Ft, St = (t.detach().double().cpu().numpy() for t in (Et, Ft, St))
    for what, (re, rf, rs) in (("float64 step", (ref["E"].numpy(), ref["F"].numpy(), ref["S"].numpy())), ("eval mode", (e, f, s))):
        print(f"{tag} {batch}: train vs {what}: E {np.abs(Et - re).max():.2e}, F {np.abs(Ft - rf).max():.2e} (max|F| "
              f"{np.abs(rf).max():.2e}), S {np.abs(St - rs).max():.2e} (max|S| {np.abs(rs).max():.2e})")
    for re, rf, rs in ((ref["E"].numpy(), ref["F"].numpy(), ref["S"].numpy()), (e, f, s)):
        assert (np.abs(Et - re) <= 1e-5 * np.maximum(1.0, np.abs(re))).all()
        assert np.abs(Ft - rf).max() <= 1e-5 * max(1.0, np.abs(rf).max())
        assert np.abs(St - rs).max() <= 1e-5 * max(1e-2, np.abs(rs).max())
    if batch == "bcc":
        det = abs(float(np.linalg.det(_structs(batch)[0][2])))
        assert float(ref["F"].abs().max()) <= 1e-9
        assert np.abs(Ft).max() <= 1e-5 * max(1.0, np.abs(ref["S"].numpy()).max() * det ** (1.0 / 3.0))


@pytest.mark.parametrize("tag", ["cfg", "wide"])
def test_fused_training_form_equals_composite_closure(tag, monkeypatch):
    """ops.USE_TRAIN2 on / off on H, the same weights; the bars of test_gpu_pbc_train.test_fused_training_form_equals_composite_closure:
    loss 2e-5, flat gradient 2e-3 of the norm (worst element 5e-3 of the largest).  Measured on MI355X: wide 2.7e-5 of the norm,
    worst element 2.5e-5, loss 7.8e-7; cfg (8-wide embeddings: the composite closure either way) identical."""
    base = _model(tag)
    targets = _targets(_host_outputs(tag, "H"))
    flat, loss = {}, {}
    for form in (True, False):
        monkeypatch.setattr(ops, "USE_TRAIN2", form)
        ts = PeriodicTrainStep(copy.deepcopy(base), rho_force=PT.RHO_FORCE, rho_stress=PT.RHO_STRESS, fused_optimizer=True)
        loss[form] = float(ts(_batch("H"), targets, step_optimizer=False))
        torch.cuda.synchronize()
        flat[form] = ts.buf.flat.clone()
        assert bool(torch.isfinite(flat[form]).all())
    rel = float((flat[True] - flat[False]).norm() / flat[False].norm())
    worst = float((flat[True] - flat[False]).abs().max() / flat[False].abs().max())
    print(f"{tag} H: loss {loss[True]:.8f} / {loss[False]:.8f}; fused vs composite: {rel:.2e} of the norm, worst element {worst:.2e}")
    assert abs(loss[True] - loss[False]) <= 2e-5 * abs(loss[False])
    assert rel <= 2e-3 and worst <= 5e-3


# -------------------------------------------------------------------------------------------------------------- GemNet-dT
def _direct_model(tag, coupled):
    m = GemNet(**DT.direct_cfg(CFGS[tag], coupled), scale_file=SCALE_FILE)
    m.load_state_dict(GO.expand_to_reference_state_dict({k: v.float() for k, v in DT.make_params(tag, coupled).items()}))
    return m.to(DEV)


@pytest.mark.parametrize("tag,coupled", [("cfg", True), ("wide", True), ("wide", False)])
def test_direct_force_gradients_match_the_oracle(tag, coupled, monkeypatch):
    """GemNet-dT on H, rho_force = 0.9, fp32 on the device against the float64 exact-autograd cluster oracle (computed here:
    ~1 s).  Bars of test_gpu_pbc_direct_train.test_parameter_gradients_match_the_oracle: loss rtol 2e-5, per-parameter norms
    rtol 2e-3 with atol 1e-6 max|g_ref|, |g - g_ref| <= 2e-3 |g_ref| + the same atol per parameter; the force head and its
    adjoint (gn_direct_force_bwd_f32) run exactly once.  Measured on MI355X (worst |g - g_ref| / bar; loss relative): cfg coupled
    0.0032; 2.0e-7, wide coupled 0.0020; 1.7e-7, wide uncoupled 0.0032; 6.0e-7."""
    params = DT.make_params(tag, coupled)
    structs = PT.hard_structures()
    ref = DT.oracle(params, DT.direct_cfg(CFGS[tag], coupled), structs, PT.trainable(_direct_model(tag, coupled), params))
    cnt = Counter()
    for name in ("direct_force", "direct_force_bwd", "chain"):
        f = getattr(K, name)
        monkeypatch.setattr(K, name, (lambda *a, _f=f, _n=name, **k: (cnt.update([_n]), _f(*a, **k))[1]))
    ts = PeriodicTrainStep(_direct_model(tag, coupled), rho_force=PT.RHO_FORCE, fused_optimizer=True)
    targets = {k: ref[k + "t"].float().to(DEV) for k in ("E", "F")}
    loss = float(ts(PT.batch(structs, device=DEV, dtype=torch.float32), targets, step_optimizer=False))
    torch.cuda.synchronize()
    g = {n: p.grad.detach().double().cpu() for n, p in ts.model.named_parameters() if p.requires_grad}
    gref = ref["grads"]
    assert set(g) == set(gref)
    gmax = max(float(v.norm()) for v in gref.values())
    atol = 1e-6 * gmax
    ratio = {n: float((g[n] - gref[n]).norm()) / (2e-3 * float(gref[n].norm()) + atol) for n in gref}
    worst = max(ratio, key=ratio.get)
    print(f"dT {tag} coupled={coupled} H: loss {loss:.8f} (oracle {ref['loss']:.8f}, rel {abs(loss - ref['loss']) / abs(ref['loss']):.2e}); "
          f"worst |g - g_ref| / (2e-3 |g_ref| + 1e-6 max|g_ref|) = {ratio[worst]:.4f} ({worst}); launches {dict(cnt)}")
    np.testing.assert_allclose(loss, ref["loss"], rtol=2e-5)
    names = sorted(gref)
    np.testing.assert_allclose([float(g[n].norm()) for n in names], [float(gref[n].norm()) for n in names], rtol=2e-3, atol=atol)
    assert ratio[worst] <= 1.0, (worst, ratio[worst])
    assert cnt["direct_force"] == 1 and cnt["direct_force_bwd"] == 1, cnt
    assert (cnt["chain"] > 0) == (tag == "wide"), cnt


# ---------------------------------------------------------------------------------------------------------- captured steps
def test_captured_step_is_clean_bit_reproducible_and_equals_eager():
    """PeriodicTrainStep(fused_optimizer=True, rho_stress > 0).capture(check=True) on H: the happens-before checker sees every
    node, resolves every pointer and finds no race; four replays give the eager step's flat gradient bit for bit; three
    optimizer steps replayed equal three eager steps."""
    base = _model("wide")
    inputs, targets = _batch("H"), _targets(_host_outputs("wide", "H"))
    kw = dict(rho_force=PT.RHO_FORCE, rho_stress=PT.RHO_STRESS, fused_optimizer=True)
    eager = PeriodicTrainStep(copy.deepcopy(base), **kw)
    eager(inputs, targets, step_optimizer=False)
    torch.cuda.synchronize()
    ref = eager.buf.flat.clone()
    cap = PeriodicTrainStep(copy.deepcopy(base), **kw)
    cap_inputs = _batch("H")
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
    assert bool(torch.isfinite(ref).all()) and float(ref.norm()) > 0


def _hard_trajectory(direct):
    """pbc_padded_train_common.trajectory on the hard cells: (E, T) from (70, 512) to (76, 620) over 6 frames, in-degree <= 14,
    image ranges up to |n| = 4 (its own assertions: no pair on the cutoff, sizes changing)."""
    Z, N, pbc, frames = C.trajectory(PT.HARD, 3 if direct else C.FRAMES)
    assert len(Z) == 10 and max(int(np.abs(f[2]["cell_offsets"]).max()) for f in frames) >= 3
    return Z, N, pbc, frames


@pytest.mark.parametrize("direct", [False, True])
def test_padded_step_on_hard_cells_equals_the_eager_step_on_the_unpadded_batch(direct):
    """test_gpu_pbc_padded_train.test_padded_step_equals_the_eager_step_on_the_unpadded_batch restated on the trajectory of the
    hard cells (`wide`, autograd and direct forces; capacities from pbc_padded_train_common.capacities), its assertions and bars:
    loss 2e-5, flat gradient 1e-5 of its norm per frame through ONE graph; three optimizer steps on both sides stay together.
    Measured on MI355X: worst gradient deviation 2.8e-7 (direct: 1.2e-7), loss 1.2e-7 (9e-8)."""
    Z, N, pbc, frames = _hard_trajectory(direct)
    base = TP._model("wide", direct)
    ts = TP._padded_step(copy.deepcopy(base), Z, N, pbc, frames, direct=direct)
    eager = PeriodicTrainStep(copy.deepcopy(base), rho_force=TP.RHO_F, rho_stress=0.0 if direct else TP.RHO_S, fused_optimizer=True)
    builder = TP._builder(N, pbc)
    Et, Ft, St = TP._targets(len(N), len(Z))
    tgt = dict(E=Et, F=Ft) if direct else dict(E=Et, F=Ft, S=St)
    Zd, Nd = torch.tensor(Z, device=DEV).long(), torch.tensor(N, device=DEV)
    graph, worst_g, worst_l = None, 0.0, 0.0
    for step_opt, use in ((False, frames), (True, frames[:3])):
        for s, frame in enumerate(use):
            R, cell = TP._frame(frame)
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
                print(f"hard cells, direct={direct}, frame {s} sizes {C.sizes(frame)}: loss {la:.8f} / {lb:.8f}, "
                      f"|g - g_eager| / |g| = {rel:.2e}")
                assert float(gb.norm()) > 0 and bool(torch.isfinite(ga).all())
                assert abs(la - lb) <= 2e-5 * abs(lb), (s, la, lb)
                assert rel <= 1e-5, (s, rel)
    assert not ts.flag.tripped() and not eager.flag.tripped()
    pa = torch.cat([p.detach().reshape(-1) for p in ts.model.parameters()])
    pb = torch.cat([p.detach().reshape(-1) for p in eager.model.parameters()])
    drift = float((pa - pb).abs().max())
    print(f"hard cells, direct={direct}: worst gradient deviation {worst_g:.2e}, worst loss deviation {worst_l:.2e}, parameters "
          f"after three optimizer steps differ by at most {drift:.2e}")
    assert any(not torch.equal(p, q) for p, q in zip(ts.model.parameters(), base.parameters()))      # the optimizer stepped
    assert drift <= 6.5e-3          # (2 x 3 steps x lr 1e-3: see the test restated here)


@pytest.mark.parametrize("direct", [False, True])
def test_in_graph_list_on_hard_cells_equals_handed_in_lists_bit_for_bit(direct):
    """test_gpu_pbc_padded_train.test_in_graph_list_equals_handed_in_lists_bit_for_bit restated on the hard cells: the list built
    inside the replay (`step_positions`) against `step` with the builder's own lists — torch.equal on the loss and the flat
    gradient at every frame; the in-graph build reports no error (its sticky state stays 0: no frame is refused by the
    image-box caps) and the sizes of the brute-force list."""
    Z, N, pbc, frames = _hard_trajectory(direct)
    base = TP._model("wide", direct)
    builder = TP._builder(N, pbc)
    handed = TP._padded_step(copy.deepcopy(base), Z, N, pbc, frames, direct=direct)
    inside = TP._attach(TP._padded_step(copy.deepcopy(base), Z, N, pbc, frames, direct=direct), builder, frames[0])
    Et, Ft, St = TP._targets(len(N), len(Z))
    St = None if direct else St
    graph = None
    for s, frame in enumerate(frames):
        R, cell = TP._frame(frame)
        l0 = handed.step(R, builder(R, cell, dtype=torch.int32), cell, Et, Ft, St, step_optimizer=False)
        l1 = inside.step_positions(R, cell, Et, Ft, St, step_optimizer=False)
        torch.cuda.synchronize()
        assert inside.pad.index_error() == 0, (s, inside.pad.index_error(), inside.pad.index_sizes())
        assert inside.pad.index_sizes() == C.sizes(frame)[:2], s
        assert bool(torch.isfinite(l1)) and float(handed.buf.flat.norm()) > 0
        assert torch.equal(l0, l1) and torch.equal(handed.buf.flat, inside.buf.flat), s
        graph = graph or inside._graph
        assert inside._graph is graph
    assert not inside.flag.tripped()
