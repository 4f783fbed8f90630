"""CPU, float64: periodic TRAINING on cells with a height below the cutoff, sheared cells and a left-handed one
(pbc_train_common.HARD = bcc_pert, thin, skewed, skewed_lh, and bcc alone) — the float64 emulated training step, which is the
reference of tests/test_gpu_pbc_train_cells.py, tied to the cluster oracle: GemNet-T with the energy + force + stress loss
against the gradient oracle of tests/pbc_train_common.py at the default and at stress-only loss weights, a knocked-out adjoint
(det in place of |det|) that the same bars must catch, direct-force GemNet-T (GemNet-dT) against exact autograd of the cluster
oracle, the fused training form against the composite closure, and the exactly collinear triplets of these cells counted from
the brute-force lists.

The oracle's forces and stress are Richardson-extrapolated here ((4 fd(h) - fd(2h)) / 3, pbc_common.fd_forces_stress): they
set the targets and thereby the cotangents of the loss, and the plain central difference at h = 1e-4 is ~1e-6 relative off on
cells with image distances below 1 A — above the 1e-6 bar of tests/test_pbc_train_cpu.py, whose cells do not have them
(`test_plain_central_differences_are_the_oracles_own_error`).  E, F, S of a batch are computed once per configuration and
shared by both loss weights; nothing below modifies them."""
import functools
from collections import Counter

import numpy as np
import pytest
import torch

import pbc_common as P
import pbc_direct_train_common as DT
import pbc_train_common as PT
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd import ops
from gemnet_pytorch_amd.training.periodic import PeriodicTrainStep
from test_model_cpu import build

CFGS = {"cfg": P.CFG, "wide": PT.CFG_WIDE}
BATCHES = {"H": PT.HARD, "bcc": ("bcc",), "skewed": ("skewed",)}
WEIGHTS = {"default": (PT.RHO_FORCE, PT.RHO_STRESS), "stress": (0.0, 1.0)}
CASES = [("cfg", "H"), ("cfg", "bcc"), ("wide", "H")]


@functools.lru_cache(maxsize=None)
def _params(tag):
    return PT.make_params(CFGS[tag])


@functools.lru_cache(maxsize=None)
def _structs(batch):
    return PT.hard_structures(BATCHES[batch])


@functools.lru_cache(maxsize=None)
def _names(tag):
    with PT.emulate():
        return tuple(PT.trainable(build(CFGS[tag], _params(tag)), _params(tag)))


@functools.lru_cache(maxsize=None)
def _efs(tag, batch):
    """The cluster oracle's E, F (Richardson), S (Richardson) of a batch: once per configuration."""
    return PT.energies_forces_stress(_params(tag), CFGS[tag], _structs(batch), richardson=True)


@functools.lru_cache(maxsize=None)
def _reference(tag, batch, weights):
    rho_f, rho_s = WEIGHTS[weights]
    return PT.oracle(_params(tag), CFGS[tag], _structs(batch), list(_names(tag)), rho_f, rho_s, efs=_efs(tag, batch))


def _step(tag, batch, ref, weights, train2=True, count=None, adjoint=None):
    """One forward + loss + backward of PeriodicTrainStep on the emulated launchers -> (model, loss).  `adjoint`: a stand-in
    for the emulated pbc_force_stress_adj (the knock-out test)."""
    rho_f, rho_s = WEIGHTS[weights]
    old = ops.USE_TRAIN2
    ops.USE_TRAIN2 = train2
    try:
        with PT.emulate():
            saved = {n: getattr(K, n) for n in PT._K_NAMES + ["chain"]}
            if adjoint is not None:
                K.pbc_force_stress_adj = adjoint
            if count is not None:
                for n in saved:
                    setattr(K, n, (lambda *a, _f=getattr(K, n), _n=n, **k: (count.update([_n]), _f(*a, **k))[1]))
            try:
                model = build(CFGS[tag], _params(tag)).train()
                ts = PeriodicTrainStep(model, rho_force=rho_f, rho_stress=rho_s)
                loss = ts._forward_backward(PT.batch(_structs(batch)), dict(E=ref["Et"], F=ref["Ft"], S=ref["St"]))
            finally:
                for n, f in saved.items():
                    setattr(K, n, f)
    finally:
        ops.USE_TRAIN2 = old
    return model, float(loss)


def _errors(model, ref):
    """-> (worst |g - g_ref| / max|g_ref| with its name, worst |g - g_ref| / (2e-3 |g_ref,n| + 1e-6 max|g_ref|): the float64 bar
    of this file and the float32 bar of the GPU tests)."""
    g = {n: p.grad for n, p in model.named_parameters() if p.requires_grad}
    gref = ref["grads"]
    assert set(g) == set(gref) and all(v is not None for v in g.values())
    gmax = max(float(v.norm()) for v in gref.values())
    err = {n: float((g[n] - gref[n]).norm()) / gmax for n in gref}
    f32 = max(float((g[n] - gref[n]).norm()) / (2e-3 * float(gref[n].norm()) + 1e-6 * gmax) for n in gref)
    worst = max(err, key=err.get)
    return err[worst], worst, f32


# ----------------------------------------------------------------------------------------------------------------- GemNet-T
@pytest.mark.parametrize("weights", list(WEIGHTS))
@pytest.mark.parametrize("tag,batch", CASES)
def test_parameter_gradients_match_the_richardson_oracle(tag, batch, weights):
    """grad_theta of (1 - rho_f) mean|E - Et| + rho_f mean_a |F_a - Ft_a| + rho_s (1/B) sum_b |S_b - St_b|_F at (rho_f, rho_s) =
    (0.9, 0.05) and at the stress-only weights (0, 1), where the stress adjoint — 1/|det|, the self-image edges whose force
    adjoint vanishes — is all there is besides the energy.  Batch H = [bcc_pert, thin, skewed, skewed_lh] (10 atoms, 74 edges,
    598 triplets) and bcc alone (forces zero by symmetry, 28 triplets at exactly pi).  Bars of tests/test_pbc_train_cpu.py:
    |g - g_ref| <= 1e-6 max_n |g_ref,n| per parameter, loss rtol 1e-7, every launcher of the second-order sweep once.
    Measured (worst |g - g_ref| / max|g_ref|; the oracle's |D(h) - Richardson| / max|g_ref|; loss, relative):
        cfg  H    default 2.9e-11; 9.9e-7; 1e-12      stress 5.1e-12; 1.1e-6; 8e-14
        cfg  bcc  default 4.0e-11; 3.9e-8; 3e-13      stress 1.3e-12; 7.3e-8; 2e-13
        wide H    default 9.3e-11; 1.1e-6; 1e-13      stress 1.2e-9;  1.5e-5; 5e-11"""
    ref = _reference(tag, batch, weights)
    cnt = Counter()
    model, loss = _step(tag, batch, ref, weights, count=cnt)
    err, worst, _ = _errors(model, ref)
    print(f"{tag} {batch} {weights}: loss {loss:.12f} (oracle {ref['loss']:.12f}, rel {abs(loss - ref['loss']) / abs(ref['loss']):.1e}); "
          f"worst |g - g_ref| / max|g_ref| = {err:.3e} ({worst}); oracle |D(h) - Richardson| / max|g_ref| = {ref['trunc']:.3e}")
    np.testing.assert_allclose(loss, ref["loss"], rtol=1e-7)
    assert err <= 1e-6, (worst, err, ref["trunc"])
    assert cnt["chain"] > 0
    for n in PT._K_NAMES:
        assert cnt[n] == 1, (n, cnt)
    if batch == "bcc":
        assert float(ref["F"].abs().max()) <= 1e-9              # symmetry: what the force term sees is the offset alone


def test_plain_central_differences_are_the_oracles_own_error():
    """A property of the ORACLE, and the reason for its Richardson form here: on `skewed` (cfg, default weights) the gap
    between the float64 step and the oracle with plain central-difference forces and stress falls as h^2 — the gaps at h = 1e-4
    and h = 5e-5 are in the ratio 4 +- 25 % — while the step does not change.  Measured: 1.18e-6 and 2.9e-7 of max|g_ref| (ratio
    4.0), above / below the 1e-6 bar; with Richardson 4e-11."""
    tag, batch, weights = "cfg", "skewed", "default"
    gap = {}
    for h in (1e-4, 5e-5):
        ref = PT.oracle(_params(tag), CFGS[tag], _structs(batch), list(_names(tag)), fd_h=h)
        model, _ = _step(tag, batch, ref, weights)
        gap[h] = _errors(model, ref)[0]
    ref = _reference(tag, batch, weights)
    rich = _errors(_step(tag, batch, ref, weights)[0], ref)[0]
    print(f"skewed: |g - g_ref| / max|g_ref| with plain differences h = 1e-4: {gap[1e-4]:.3e}, h = 5e-5: {gap[5e-5]:.3e} "
          f"(ratio {gap[1e-4] / gap[5e-5]:.2f}); Richardson: {rich:.3e}")
    assert 3.0 <= gap[1e-4] / gap[5e-5] <= 5.0
    assert rich <= 1e-3 * gap[1e-4]


def _signed_det_adjoint(gF, gS, V, id_c, id_a, batch_seg, cell, scale=-1.0):
    """pbc_train_common.pbc_force_stress_adj with det in place of |det|: the classic left-handed-cell error."""
    gG = gF[id_a.long()] - gF[id_c.long()]
    if gS is not None:
        b = batch_seg.long()[id_a.long()]
        gG = gG + (scale / torch.linalg.det(cell))[b][:, None] * torch.einsum("ei,eij->ej", V, gS[b])
    return gG


@pytest.mark.parametrize("tag", ["cfg", "wide"])
def test_a_signed_determinant_in_the_adjoint_is_caught(tag):
    """Teeth: the same step with the emulated pbc_force_stress_adj using det instead of |det| (a substitution of a Python
    function on the host).  On H — one of four cells is left-handed — it must miss the float32 bar of the GPU tests,
    2e-3 |g_ref,n| + 1e-6 max|g_ref|, by at least 10 x at the stress-only weights and miss it at the default weights, where the
    stress term is 0.05 of the loss; it then misses the float64 bar of this file by orders of magnitude.  Without a left-handed
    cell (bcc) the substitution changes nothing.  Measured (x the float32 bar, default / stress-only): cfg 2.4 / 43.0, wide 2.3 / 43.4."""
    ratio = {}
    for weights in WEIGHTS:
        ref = _reference(tag, "H", weights)
        model, _ = _step(tag, "H", ref, weights, adjoint=_signed_det_adjoint)
        err, worst, ratio[weights] = _errors(model, ref)
        print(f"{tag} H {weights}: det for |det| in the adjoint: {ratio[weights]:.1f} x the float32 bar, {err / 1e-6:.3g} x the "
              f"float64 bar ({worst})")
        assert err > 1e-6
    assert ratio["stress"] >= 10.0 and ratio["default"] > 1.0, ratio
    if tag == "cfg":
        ref = _reference(tag, "bcc", "stress")
        assert _errors(_step(tag, "bcc", ref, "stress", adjoint=_signed_det_adjoint)[0], ref)[0] <= 1e-6


@pytest.mark.parametrize("tag", ["cfg", "wide"])
def test_fused_training_form_equals_composite_closure(tag):
    """ops.USE_TRAIN2 on / off on H, the float64 bars of tests/test_pbc_train_cpu.py: loss rtol 1e-9, gradients 1e-7 relative."""
    ref = _reference(tag, "H", "default")
    cnt = Counter()
    m1, l1 = _step(tag, "H", ref, "default", True)
    m0, l0 = _step(tag, "H", ref, "default", False, cnt)
    assert cnt["chain"] == 0 and cnt["dist_vec_fwd"] == 0 and cnt["angle_vec_jvp"] == 0 and cnt["pbc_force_stress_adj"] == 1, cnt
    np.testing.assert_allclose(l1, l0, rtol=1e-9)
    g0 = dict(m0.named_parameters())
    for n, p in m1.named_parameters():
        if p.requires_grad:
            assert float((p.grad - g0[n].grad).norm()) <= 1e-7 * float(g0[n].grad.norm()) + 1e-12, n


# ---------------------------------------------------------------------------------------------------------------- GemNet-dT
@functools.lru_cache(maxsize=None)
def _direct_reference(tag, coupled):
    params, cfg = DT.make_params(tag, coupled), DT.direct_cfg(CFGS[tag], coupled)
    with DT.emulate():
        names = PT.trainable(build(cfg, params), params)
    return DT.oracle(params, cfg, _structs("H"), names)


@pytest.mark.parametrize("coupled", [True, False])
@pytest.mark.parametrize("tag", ["cfg", "wide"])
def test_direct_force_gradients_match_exact_autograd(tag, coupled):
    """GemNet-dT on H against pbc_direct_train_common.oracle (the cluster oracle with the parameters as leaves: no finite
    differences), the bars of tests/test_pbc_direct_train_cpu.py: every parameter within 1e-7 relative, the loss within 1e-9;
    every parameter is reached; the force head and its adjoint run once.  Measured: worst 3.5e-14 relative, loss 3e-15."""
    ref = _direct_reference(tag, coupled)
    assert all(float(v.abs().max()) > 0 for v in ref["grads"].values())
    cnt = Counter()
    with DT.emulate():
        saved = {n: getattr(K, n) for n in DT._K_NAMES}
        for n, f in saved.items():
            setattr(K, n, (lambda *a, _f=f, _n=n, **k: (cnt.update([_n]), _f(*a, **k))[1]))
        try:
            model = build(DT.direct_cfg(CFGS[tag], coupled), DT.make_params(tag, coupled)).train()
            ts = PeriodicTrainStep(model, rho_force=PT.RHO_FORCE)
            loss = float(ts._forward_backward(PT.batch(_structs("H")), dict(E=ref["Et"], F=ref["Ft"])))
        finally:
            for n, f in saved.items():
                setattr(K, n, f)
    g = {n: p.grad for n, p in model.named_parameters() if p.requires_grad}
    assert set(g) == set(ref["grads"]) and all(v is not None for v in g.values())
    err = {n: float((g[n] - ref["grads"][n]).norm()) / float(ref["grads"][n].norm()) for n in g}
    worst = max(err, key=err.get)
    print(f"dT {tag} coupled={coupled}: loss rel {abs(loss - ref['loss']) / abs(ref['loss']):.1e}; worst |g - g_ref| / |g_ref| = "
          f"{err[worst]:.3e} ({worst})")
    np.testing.assert_allclose(loss, ref["loss"], rtol=1e-9)
    assert err[worst] <= 1e-7, (worst, err[worst])
    assert cnt["direct_force"] == 1 and cnt["direct_force_bwd"] == 1, cnt


# ------------------------------------------------------------------------------------------------------ collinear triplets
COLLINEAR = {"bcc": (0, 28), "thin": (8, 16)}          # exactly collinear triplets (theta = 0, theta = pi) per kind


def test_exactly_collinear_triplets_of_the_hard_cells():
    """The max(|u x v|, 1e-9) clamp is reached through real lists: [bcc, thin], rounded to float32, holds 8 triplets at exactly
    theta = 0 (thin: the self-image edges n = 1 and n = 2 along its 1.2 A axis) and 44 at exactly pi (bcc: 28, opposite images;
    thin: 16) — bcc alone has none at theta = 0, so the GPU kernel test uses both kinds.  Such an edge pair lies along a cell
    axis or has float32-exact products, so the cross product vanishes with and without fused multiply-adds.  More than a third
    of the triplets of [bcc, thin, skewed_lh] have sin(theta) >= 0.3 (the rows compared elementwise on the GPU)."""
    for kind, (n0, npi) in COLLINEAR.items():
        _, _, _, at0, atpi = PT.collinear_rows([P.structure(kind)])
        print(f"{kind}: {len(at0)} triplets at exactly theta = 0, {len(atpi)} at exactly pi")
        assert (len(at0), len(atpi)) == (n0, npi)
    V, idx, _, at0, atpi = PT.collinear_rows([P.structure(k) for k in ("bcc", "thin")])
    assert len(at0) == 8 and len(atpi) == 44
    # every self-image edge has a partner at exactly pi
    own = np.nonzero(idx["id_a"] == idx["id_c"])[0]
    assert len(own) == 20 and set(own) <= set(idx["id3_reduce_ca"][atpi])
    V, idx, _, at0, atpi = PT.collinear_rows([P.structure(k) for k in ("bcc", "thin", "skewed_lh")])
    Vd = torch.tensor(V, dtype=torch.float64)
    th = PT.angle_vec_fwd(Vd, torch.tensor(idx["id3_reduce_ca"]), torch.tensor(idx["id3_expand_ba"]))
    T = len(th)
    assert T == 364 + 112 + 70 and int((torch.sin(th) >= 0.3).sum()) > T // 3
    assert float(th[at0].max()) < 1e-8 and float((th[atpi] - np.pi).abs().max()) < 1e-8
