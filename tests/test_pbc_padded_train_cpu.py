"""Padded periodic training (training.periodic.PeriodicPaddedTrainStep) on the host emulation of the launchers, float64: loss
and every parameter gradient of the padded step equal the plain PeriodicTrainStep on the unpadded batch (the dummy molecule's
energy, forces and stress row are cut off before the loss) — algebra, not rounding; the refusals; and the float64
restatement of the one-launch loss (tests/pbc_padded_train_common.py) against autograd of pbc_train_common.loss_fp64."""
import numpy as np
import pytest
import torch

import pbc_common as P
import pbc_direct_train_common as DT
import pbc_padded_train_common as C
import pbc_train_common as PT
from gemnet_pytorch_amd.training.periodic import PeriodicPaddedTrainStep, PeriodicTrainStep
from test_model_cpu import build

CFGS = {"cfg": P.CFG, "wide": PT.CFG_WIDE}
F64 = torch.float64


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _compare(tag, direct):
    Z, N, pbc, frames = C.trajectory(C.BATCH, 3)
    cfg = DT.direct_cfg(CFGS[tag], True) if direct else CFGS[tag]
    params = PT.make_params(cfg)
    e_cap, t_cap, deg, G = C.capacities(frames)
    rho_s = 0.0 if direct else PT.RHO_STRESS
    Et, Ft, St = (torch.tensor(t) for t in C.targets(len(N), len(Z)))
    Zt, Nt = torch.tensor(Z).long(), torch.tensor(N)
    assert len({C.sizes(f)[:2] for f in frames}) >= 2
    with C.emulate(direct):
        padded = build(cfg, params).train()
        ts = PeriodicPaddedTrainStep(padded, Zt, Nt, e_cap, t_cap, cell=torch.tensor(frames[0][1]), pbc=pbc, max_in_degree=deg,
                                     n_groups=G, rho_force=PT.RHO_FORCE, rho_stress=rho_s)
        assert padded.periodic_training and bool(getattr(padded, "periodic_direct_forces", False)) == direct
        # the runner keeps the cells in float32 (what the device reads); the float64 stand-ins take |det cell| in the cell's own
        # dtype, so the emulation holds them in float64 like the unpadded batch (the frames are float32-representable)
        ts.pad.inputs["cell"] = ts.inputs["cell"] = ts.pad.inputs["cell"].double()
        for s, frame in enumerate(frames):
            R, cell, idx = C.frame_tensors(frame, "cpu", F64)
            lp = ts.step(R, idx, cell, Et, Ft, None if direct else St, step_optimizer=False)
            gp = _grads(padded)
            plain = build(cfg, params).train()
            te = PeriodicTrainStep(plain, rho_force=PT.RHO_FORCE, rho_stress=rho_s)
            tgt = dict(E=Et, F=Ft) if direct else dict(E=Et, F=Ft, S=St)
            le = te(C.unpadded_inputs(Z, N, frame, "cpu", F64), tgt, step_optimizer=False)
            ge = _grads(plain)
            # the bar of tests/test_padded_cpu.py (the molecular twin)
            np.testing.assert_allclose(float(lp), float(le), rtol=1e-12)
            assert gp.keys() == ge.keys() and len(ge) > 10
            for n in ge:
                np.testing.assert_allclose(gp[n].numpy(), ge[n].numpy(), rtol=1e-9,
                                           atol=1e-12 * float(ge[n].abs().max() + 1e-30), err_msg=f"frame {s}: {n}")
            assert any(float(g.abs().max()) > 0 for g in ge.values())


@pytest.mark.parametrize("tag", ["cfg", "wide"])
def test_padded_step_has_the_loss_and_gradients_of_the_unpadded_batch(tag):
    """3 frames of (small, triclinic, slab, cubic1) through one set of buffers, energy + force + stress loss."""
    _compare(tag, direct=False)


@pytest.mark.parametrize("tag", ["cfg", "wide"])
def test_padded_step_of_a_direct_force_model(tag):
    """The same for GemNet-dT (E, F; no stress)."""
    _compare(tag, direct=True)


def test_refusals():
    Z, N, pbc, frames = C.trajectory(C.BATCH, 3)
    e_cap, t_cap, deg, G = C.capacities(frames)
    Zt, Nt, cell0 = torch.tensor(Z).long(), torch.tensor(N), torch.tensor(frames[0][1])
    Et, Ft, St = (torch.tensor(t) for t in C.targets(len(N), len(Z)))
    kw = dict(cell=cell0, pbc=pbc, max_in_degree=deg, n_groups=G, rho_force=PT.RHO_FORCE)
    with C.emulate(direct=True):
        # GemNet-Q
        q = build(dict(P.CFG, triplets_only=False), PT.make_params(dict(P.CFG, triplets_only=False))).train()
        with pytest.raises(NotImplementedError, match="GemNet-Q"):
            PeriodicPaddedTrainStep(q, Zt, Nt, e_cap, t_cap, **kw)
        assert not getattr(q, "periodic_training", False)
        # an atom capacity with a cell: the runner's refusal
        t = build(P.CFG, PT.make_params(P.CFG)).train()
        with pytest.raises(NotImplementedError, match=r"periodic cells: fixed structure layout only \(no a_cap\)"):
            PeriodicPaddedTrainStep(t, Zt, Nt, e_cap, t_cap, a_cap=len(Z) + 4, **kw)
        with pytest.raises(ValueError, match="cell"):
            PeriodicPaddedTrainStep(t, Zt, Nt, e_cap, t_cap, max_in_degree=deg)
        # a direct-force model has no stress
        dcfg = DT.direct_cfg(P.CFG, True)
        d = build(dcfg, PT.make_params(dcfg)).train()
        with pytest.raises(ValueError, match="no stress"):
            PeriodicPaddedTrainStep(d, Zt, Nt, e_cap, t_cap, rho_stress=0.01, **kw)
        # the stress term needs its targets; the in-graph list needs its builder
        ts = PeriodicPaddedTrainStep(t, Zt, Nt, e_cap, t_cap, rho_stress=PT.RHO_STRESS, **kw)
        R, cell, idx = C.frame_tensors(frames[0], "cpu", F64)
        with pytest.raises(ValueError, match="stress targets"):
            ts.step(R, idx, cell, Et, Ft, step_optimizer=False)
        with pytest.raises(RuntimeError, match="attach_builder"):
            ts.step_positions(R, cell, Et, Ft, St, step_optimizer=False)
        ts.step(R, idx, cell, Et, Ft, St, step_optimizer=False)          # and with them it runs
        # what stays refused word for word: the model's own refusal of padded lists for a periodic GemNet-Q in training
        q.periodic_quadruplets = q.periodic_training = q.periodic_quadruplets_training = True
        with pytest.raises(NotImplementedError) as err:
            q._check_periodic({"_guard_rows": (len(N), len(Z))})
        assert str(err.value) == ("periodic cells (GemNet-Q): training runs on fixed index arrays only, not on the "
                                  "padded or in-graph-rebuilt lists of padded.PaddedGraphRunner")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("with_S", [True, False])
def test_loss_restatement_equals_autograd_of_the_composite(with_S, masked):
    """periodic_loss (closed-form cotangents) against torch.autograd of pbc_train_common.loss_fp64 with the weights folded as the
    step folds them; a masked row and a structure with S_b == St_b get exact zeros."""
    g = torch.Generator().manual_seed(2)
    B, A = 4, 37
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)      # noqa: E731
    E, Et, F, Ft, S, St = rnd(B, 1), rnd(B, 1), rnd(A, 3), rnd(A, 3), rnd(B, 3, 3), rnd(B, 3, 3)
    n_real = A - 5 if masked else A
    mask = (torch.arange(A) < n_real).to(F64) if masked else None
    leaves = [t.clone().requires_grad_(True) for t in (E, F, S)]
    ref = PT.loss_fp64(leaves[0], leaves[1][:n_real], leaves[2], Et, Ft[:n_real], St,
                       rho_stress=PT.RHO_STRESS if with_S else 0.0)
    rE, rF, rS = torch.autograd.grad(ref, leaves, allow_unused=True)
    w_f = PT.RHO_FORCE if masked else PT.RHO_FORCE / A
    dev = torch.tensor(1.0 / n_real, dtype=F64) if masked else None
    loss, gE, gF, gS = C.periodic_loss(E, Et, F, Ft, (1 - PT.RHO_FORCE) / B, w_f, S=S if with_S else None,
                                       St=St if with_S else None, w_s=PT.RHO_STRESS / B, mask=mask, w_f_dev=dev)
    np.testing.assert_allclose(float(loss), float(ref.detach()), rtol=1e-13)
    np.testing.assert_allclose(gE.numpy(), rE.numpy(), rtol=1e-13, atol=0)
    np.testing.assert_allclose(gF.numpy(), rF.numpy(), rtol=1e-12, atol=1e-300)
    assert float(gF[n_real:].abs().sum()) == 0.0
    if with_S:
        np.testing.assert_allclose(gS.numpy(), rS.numpy(), rtol=1e-12, atol=0)
        St2 = St.clone()
        St2[2] = S[2]
        assert float(C.periodic_loss(E, Et, F, Ft, 0.1, 0.2, S=S, St=St2, w_s=0.3)[3][2].abs().sum()) == 0.0
    else:
        assert gS is None
