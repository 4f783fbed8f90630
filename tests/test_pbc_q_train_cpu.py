"""CPU, float64: training GemNet-Q on periodic batches (GemNet.periodic_quadruplets_training, training/periodic.py) on the
emulated launchers — the stored gradient oracle against a recomputation, the training-mode outputs and the parameter gradients of
the energy + force + stress loss against it (fused form and composite closure), the opt-in switch, and the adjoint / tangent
duality of the fp64 restatements of csrc/pbc_quad_train.hip on geometry with exactly planar and collinear quadruplets."""
from collections import Counter

import numpy as np
import pytest
import torch

import pbc_common as P
import pbc_q_common as Q
import pbc_q_train_common as QT
import pbc_train_common as PT
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd import ops
from gemnet_pytorch_amd.training.periodic import PeriodicTrainStep
from test_model_cpu import build

CFG = QT.CFG_QW


@pytest.fixture(scope="module")
def params():
    return QT.make_params(CFG)


@pytest.fixture(scope="module")
def golden():
    return QT.load_golden()


def _names(params):
    with QT.emulate():
        return PT.trainable(build(CFG, params), params)


def _targets(ref):
    return dict(E=ref["Et"], F=ref["Ft"], S=ref["St"])


def _step(params, tag, ref, quad, count=None, train2=True):
    """One forward + loss + backward of PeriodicTrainStep on batch `tag` -> (model, loss)."""
    old = ops.USE_TRAIN2_QUAD, ops.USE_TRAIN2
    ops.USE_TRAIN2_QUAD, ops.USE_TRAIN2 = quad, train2
    try:
        with QT.emulate():
            saved = {}
            if count is not None:
                for n in QT.COUNTED + ["chain"]:
                    f = saved[n] = getattr(K, n)
                    setattr(K, n, (lambda *a, _f=f, _n=n, **k: (count.update([_n]), _f(*a, **k))[1]))
            try:
                model = build(CFG, params).train()
                ts = PeriodicTrainStep(model, rho_force=QT.RHO_FORCE, rho_stress=QT.RHO_STRESS)
                assert model.periodic_quadruplets and model.periodic_training and model.periodic_quadruplets_training
                loss = ts._forward_backward(QT.batch(QT.structures(tag)), _targets(ref))
            finally:
                for n, f in saved.items():
                    setattr(K, n, f)
    finally:
        ops.USE_TRAIN2_QUAD, ops.USE_TRAIN2 = old
    return model, float(loss)


def test_stored_slab_contribution_is_recomputed_from_the_oracle(params, golden):
    """tests/golden/pbc_q_train.npz against pbc_q_train_common: E, F, S of 'slab' and its term of grad_theta L of batch A (with the
    cotangents of the stored batch), 1e-9 relative."""
    ref = golden["A"]
    structs = QT.structures("A")
    b = QT.BATCHES["A"].index("slab")
    off = sum(len(s[0]) for s in structs[:b])
    n = len(structs[b][0])
    E, F, S = QT.efs(params, CFG, structs[b])
    rel = lambda a, r: float(np.abs(np.asarray(a) - np.asarray(r)).max()) / float(np.abs(np.asarray(r)).max())       # noqa: E731
    assert rel(E, ref["E"][b, 0]) <= 1e-9 and rel(F, ref["F"][off:off + n]) <= 1e-9 and rel(S, ref["S"][b]) <= 1e-9
    terms, (gE, u, w) = QT.loss_terms(ref["E"][:, 0].tolist(), [ref["F"].numpy()], list(ref["S"].numpy()), structs)
    np.testing.assert_allclose(terms["loss"], ref["loss"], rtol=1e-12)
    assert torch.equal(terms["Et"], ref["Et"]) and torch.equal(terms["Ft"], ref["Ft"]) and torch.equal(terms["St"], ref["St"])
    names = _names(params)
    g, _ = QT.contribution(params, CFG, names, structs[b], gE[b, 0], u[off:off + n], w[b])
    stored = golden["A.slab"]
    assert set(g) == set(stored)
    got, want = QT.flatten({k: v.numpy() for k, v in g.items()}, names), QT.flatten({k: v.numpy() for k, v in stored.items()}, names)
    assert float(np.linalg.norm(got - want)) <= 1e-9 * float(np.linalg.norm(want))
    assert max(rel(g[k], stored[k]) for k in names) <= 1e-9


def test_training_mode_outputs_are_the_oracles(params, golden):
    """The bars of test_pbc_train_cpu.test_training_mode_outputs_are_the_oracles (central differences with h = 1e-4)."""
    ref = golden["A"]
    with QT.emulate():
        model = build(CFG, params).train()
        model.periodic_quadruplets = model.periodic_training = model.periodic_quadruplets_training = True
        E, F, S = model(QT.batch(QT.structures("A")), stress=True)
        assert E.requires_grad and F.requires_grad and S.requires_grad
        E2, F2 = model(QT.batch(QT.structures("A")))
    assert torch.equal(E, E2) and torch.equal(F, F2)
    assert float((E.detach() - ref["E"]).abs().max()) <= 1e-9 * max(1.0, float(ref["E"].abs().max()))
    assert float((F.detach() - ref["F"]).abs().max()) <= 1e-6 * max(1.0, float(ref["F"].abs().max()))
    assert float((S.detach() - ref["S"]).abs().max()) <= 1e-6 * max(1e-2, float(ref["S"].abs().max()))


@pytest.mark.parametrize("tag", ["A", "B"])
@pytest.mark.parametrize("quad", [True, False], ids=["fused", "composite"])
def test_parameter_gradients_match_the_oracle(params, golden, tag, quad):
    """grad_theta of the loss of training/periodic.py (rho_f = 0.9, rho_s = 0.05) on batch A / B, the fused quadruplet form
    (ops_train._AngleVec2Q / _QuadAnglesVec2) and the composite closure (GemNet.calculate_angles_vec).  Bar: the oracle's,
    |g - g_ref| <= 1e-6 max_n |g_ref,n| per parameter, loss rtol 1e-7 (test_pbc_train_cpu)."""
    ref = golden[tag]
    cnt = Counter()
    model, loss = _step(params, tag, ref, quad, cnt)
    g = {n: p.grad for n, p in model.named_parameters() if p.requires_grad}
    assert set(g) == set(ref["grads"]) and all(v is not None for v in g.values())
    gmax = max(float(v.norm()) for v in ref["grads"].values())
    assert min(float(v.norm()) for v in ref["grads"].values()) >= 1e-6 * gmax
    err = {n: float((g[n] - ref["grads"][n]).norm()) / gmax for n in g}
    worst = max(err, key=err.get)
    print(f"{tag} {'fused' if quad else 'composite'}: loss {loss:.12f} (oracle {ref['loss']:.12f}); worst |g - g_ref| / max|g_ref| = "
          f"{err[worst]:.3e} ({worst}); oracle |D(h) - Richardson| / max|g_ref| = {ref['trunc']:.3e}")
    np.testing.assert_allclose(loss, ref["loss"], rtol=1e-7)
    assert err[worst] <= 1e-6, (worst, err[worst], ref["trunc"])
    assert cnt["chain"] > 0 and cnt["pbc_force_stress_adj"] == 2 and cnt["angle_vec_jvp"] == 1, cnt
    for n in ("dist_vec_fwd", "dist_vec_bwd", "dist_vec_jvp"):
        assert cnt[n] == 2, (n, cnt)                   # V and Vint
    for n in QT._K_NAMES:
        assert cnt[n] == (1 if quad else 0), (n, cnt)


def test_fused_form_equals_composite_closure(params, golden):
    """The three forms on the same weights — fused quadruplet twins, ATen on (V, Vint) under the fused stacks, ATen throughout
    (GEMNET_TRAIN2=0) — at the fp64 bars of tests/test_train2_cpu.py: loss rtol 1e-9, gradients 1e-7 relative."""
    ref = golden["B"]
    m1, l1 = _step(params, "B", ref, True)
    for train2 in (True, False):
        cnt = Counter()
        m0, l0 = _step(params, "B", ref, not train2, cnt, train2=train2)
        assert all(cnt[n] == 0 for n in QT._K_NAMES) and (cnt["chain"] > 0) == train2, cnt
        np.testing.assert_allclose(l1, l0, rtol=1e-9)
        g0 = dict(m0.named_parameters())
        for n, p in m1.named_parameters():
            if p.requires_grad:
                assert float((p.grad - g0[n].grad).norm()) <= 1e-7 * float(g0[n].grad.norm()) + 1e-12, n


def test_without_the_switch_a_training_call_raises_the_unchanged_message(params):
    msg = r"GemNet-Q runs on the first-order \(eval\) path only; training with a cell is GemNet-T only"
    with QT.emulate():
        model = build(CFG, params).train()
        assert getattr(model, "periodic_quadruplets_training", False) is False
        model.periodic_quadruplets = True
        for flag in (False, True):
            model.periodic_training = flag
            with pytest.raises(NotImplementedError, match=msg):
                model(QT.batch(QT.structures("B")))
        model.periodic_quadruplets_training = True
        inputs = QT.batch(QT.structures("B"))
        inputs["R"] = inputs["R"].requires_grad_(True)
        with pytest.raises(NotImplementedError, match=r"GemNet-Q.*autograd graph"):
            model(inputs)
        with pytest.raises(NotImplementedError, match=r"GemNet-Q.*padded"):
            model(dict(QT.batch(QT.structures("B")), _guard_rows=(1, 2)))
        model.periodic_training = False
        with pytest.raises(NotImplementedError, match="periodic_training"):
            model(QT.batch(QT.structures("B")))


def test_stress_term_needs_its_targets(params, golden):
    ref = golden["B"]
    with QT.emulate():
        ts = PeriodicTrainStep(build(CFG, params).train(), rho_force=QT.RHO_FORCE, rho_stress=QT.RHO_STRESS)
        with pytest.raises(ValueError, match=r"targets\['S'\]"):
            ts(QT.batch(QT.structures("B")), dict(E=ref["Et"], F=ref["Ft"]))


def test_adjoint_and_tangent_of_the_restatements_are_dual():
    """sum_q g_ang . tang == <gV, tV> + <gVint, tVint> to 1e-12 on the real geometry of ['bcc_pert', 'thin'] (exactly planar and
    exactly collinear quadruplets: both sides take the decisions of quad_math.h), and the same for the a - b <- d angle."""
    from gemnet_pytorch_amd import pbc
    from gemnet_pytorch_amd.graph import GraphPlan
    inputs = QT.batch([P.structure("bcc_pert"), P.structure("thin")])
    plan = GraphPlan(inputs, False)
    with QT.emulate():
        V, Vint = PT.edge_vectors(inputs["R"], plan, inputs["cell"]), QT.int_edge_vectors(inputs["R"], plan, inputs["cell"])
        flat, vanished, fixed = QT.quad_decisions(*QT.quad_vectors(V, Vint, *pbc.quad_index(plan)))
        assert int(flat.sum()) > 0 and int(vanished.sum()) > 0 and int((fixed & ~vanished).sum()) > 0
        g = torch.Generator().manual_seed(7)
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)       # noqa: E731
        tV, tVint = rnd(*V.shape), rnd(*Vint.shape)
        g_ang = torch.zeros(plan.quad.size, 4, dtype=torch.float64)
        g_ang[:, :2] = rnd(plan.quad.size, 2)
        gV, gVint = QT.quad_angles_vec_adjoint(g_ang, V, Vint, plan)
        tang = QT.quad_angles_vec_jvp(V, Vint, tV, tVint, *pbc.quad_index(plan))
        assert (tang[flat, 0] == 0).all() and (tang[fixed, 1] == 0).all() and (tang[:, 2:] == 0).all()
        lhs, rhs = float((g_ang * tang).sum()), float((gV * tV).sum() + (gVint * tVint).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)
        iu, iw = plan.intm_ab.idx32, plan.intm_db.idx32
        gth = rnd(iu.shape[0])
        GU, GW = QT.angle_vec2_bwd(gth, Vint, iu, V, iw)
        lhs = float((gth * QT.angle_vec2_jvp(Vint, iu, V, iw, tVint, tV)).sum())
        rhs = float((K.segsum(GU, *plan.intm_ab.csr, plan.n_int) * tVint).sum() + (K.segsum(GW, *plan.intm_db.csr, plan.n_edges) * tV).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)
