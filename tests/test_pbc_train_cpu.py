"""CPU, float64: training GemNet-T on periodic batches (GemNet.periodic_training, training/periodic.py) on the emulated
launchers — the parameter gradients of the energy + force + stress loss against the gradient oracle of
tests/pbc_train_common.py, the fused training form against the composite closure, the opt-in switch, and two gloo ranks
against one process."""
import os
import sys
from collections import Counter

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pbc_common as P
import pbc_train_common as PT
from conftest import ROOT
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd import ops
from gemnet_pytorch_amd.training.periodic import PeriodicTrainStep
from test_model_cpu import build


@pytest.fixture(scope="module")
def params():
    return PT.make_params(P.CFG)


@pytest.fixture(scope="module")
def structs():
    return PT.structures()


@pytest.fixture(scope="module")
def reference(params, structs):
    """The oracle's E, F, S, targets, loss and parameter gradients of the 4-structure batch (computed once, never modified)."""
    with PT.emulate():
        names = PT.trainable(build(P.CFG, params), params)
    return PT.oracle(params, P.CFG, structs, names)


def _step(params, structs, ref, train2, count=None, rho_stress=PT.RHO_STRESS):
    """One forward + loss + backward of PeriodicTrainStep -> (model, loss)."""
    old = ops.USE_TRAIN2
    ops.USE_TRAIN2 = train2
    try:
        with PT.emulate():
            saved = {}
            if count is not None:
                for n in PT._K_NAMES + ["chain"]:
                    f = saved[n] = getattr(K, n)
                    setattr(K, n, (lambda *a, _f=f, _n=n, **k: (count.update([_n]), _f(*a, **k))[1]))
            try:
                model = build(P.CFG, params).train()
                ts = PeriodicTrainStep(model, rho_force=PT.RHO_FORCE, rho_stress=rho_stress)
                loss = ts._forward_backward(PT.batch(structs), dict(E=ref["Et"], F=ref["Ft"], S=ref["St"]))
            finally:
                for n, f in saved.items():
                    setattr(K, n, f)
    finally:
        ops.USE_TRAIN2 = old
    return model, float(loss)


def test_parameter_gradients_match_the_oracle(params, structs, reference):
    """grad_theta of (1 - rho_f) mean|E - Et| + rho_f mean_a |F_a - Ft_a| + rho_s (1/B) sum_b |S_b - St_b|_F, rho_f = 0.9,
    rho_s = 0.05, on [small, triclinic, slab, cubic1].  Bar: |g - g_ref| <= 1e-6 max_n |g_ref,n| per parameter — set by the
    oracle's truncation (Richardson of central differences), not by the model.  Measured: worst 3.9e-8 of max |g_ref| with
    the oracle's |D(h) - Richardson| at 8e-7 of it; loss 4e-9 relative (the central-difference forces of the oracle)."""
    cnt = Counter()
    model, loss = _step(params, structs, reference, True, cnt)
    ref = reference["grads"]
    g = {n: p.grad for n, p in model.named_parameters() if p.requires_grad}
    assert set(g) == set(ref) and all(v is not None for v in g.values())
    gmax = max(float(v.norm()) for v in ref.values())
    err = {n: float((g[n] - ref[n]).norm()) / gmax for n in ref}
    worst = max(err, key=err.get)
    print(f"loss {loss:.12f} (oracle {reference['loss']:.12f}); worst |g - g_ref| / max|g_ref| = {err[worst]:.3e} ({worst}); "
          f"oracle |D(h) - Richardson| / max|g_ref| = {reference['trunc']:.3e}")
    np.testing.assert_allclose(loss, reference["loss"], rtol=1e-7)      # (F, S of the oracle: central differences, h = 1e-4)
    assert err[worst] <= 1e-6, (worst, err[worst], reference["trunc"])
    # the step ran the training form on the new launchers: value, first adjoint (under create_graph) and tangent, each once
    assert cnt["chain"] > 0
    for n in ("dist_vec_fwd", "dist_vec_bwd", "dist_vec_jvp", "angle_vec_fwd", "angle_vec_bwd", "angle_vec_jvp",
              "pbc_force_stress_adj"):
        assert cnt[n] == 1, (n, cnt)


def test_training_mode_outputs_are_the_oracles(params, structs, reference):
    with PT.emulate():
        model = build(P.CFG, params).train()
        model.periodic_training = True
        E, F, S = model(PT.batch(structs), stress=True)
        assert E.requires_grad and F.requires_grad and S.requires_grad
        E2, F2 = model(PT.batch(structs))
    assert torch.equal(E, E2) and torch.equal(F, F2)
    # central differences with h = 1e-4: ~1e-8 absolute
    assert float((E.detach() - reference["E"]).abs().max()) <= 1e-9 * max(1.0, float(reference["E"].abs().max()))
    assert float((F.detach() - reference["F"]).abs().max()) <= 1e-6 * max(1.0, float(reference["F"].abs().max()))
    assert float((S.detach() - reference["S"]).abs().max()) <= 1e-6 * max(1e-2, float(reference["S"].abs().max()))


def test_fused_training_form_equals_composite_closure(params, structs, reference):
    """ops_train._DistVec2 / _AngleVec2 + the chain programs against ATen on V (GEMNET_TRAIN2=0), the fp64 bars of
    tests/test_train2_cpu.py: loss rtol 1e-9, gradients 1e-7 relative."""
    cnt = Counter()
    m1, l1 = _step(params, structs, reference, True)
    m0, l0 = _step(params, structs, reference, False, cnt)
    assert cnt["chain"] == 0 and cnt["dist_vec_fwd"] == 0 and cnt["angle_vec_jvp"] == 0 and cnt["pbc_force_stress_adj"] == 1, cnt
    np.testing.assert_allclose(l1, l0, rtol=1e-9)
    g0 = dict(m0.named_parameters())
    for n, p in m1.named_parameters():
        if p.requires_grad:
            ref = g0[n].grad
            assert float((p.grad - ref).norm()) <= 1e-7 * float(ref.norm()) + 1e-12, n


def test_energy_and_force_terms_alone(params, structs, reference):
    """rho_stress = 0: no stress is computed or asked for (targets without 'S'), the adjoint kernel runs without gS."""
    seen = []
    with PT.emulate():
        emu = K.pbc_force_stress_adj
        K.pbc_force_stress_adj = lambda gF, gS, *a, **k: (seen.append(gS), emu(gF, gS, *a, **k))[1]
        try:
            model = build(P.CFG, params).train()
            ts = PeriodicTrainStep(model, rho_force=PT.RHO_FORCE)
            loss = ts._forward_backward(PT.batch(structs), dict(E=reference["Et"], F=reference["Ft"]))
        finally:
            K.pbc_force_stress_adj = emu
    assert seen == [None]
    want = PT.loss_fp64(reference["E"], reference["F"], reference["S"], reference["Et"], reference["Ft"], reference["St"],
                        rho_stress=0.0)
    np.testing.assert_allclose(float(loss), float(want), rtol=1e-7)


def test_without_the_switch_a_periodic_training_call_raises(params, structs):
    with PT.emulate():
        model = build(P.CFG, params).train()
        assert model.periodic_training is False
        with pytest.raises(NotImplementedError, match="periodic_training"):
            model(PT.batch(structs))
        with pytest.raises(NotImplementedError, match="periodic_training"):
            model(PT.batch(structs), stress=True)
        model.eval()
        model.force_graph = True
        with pytest.raises(NotImplementedError, match="periodic_training"):
            model(PT.batch(structs))
        # what a cell never supports keeps raising with the switch on
        model.periodic_training = True
        model.train()
        model.force_graph = None
        inputs = PT.batch(structs)
        inputs["R"] = inputs["R"].requires_grad_(True)
        with pytest.raises(NotImplementedError, match="autograd graph"):
            model(inputs)


def test_stress_term_needs_its_targets(params, structs, reference):
    with PT.emulate():
        model = build(P.CFG, params).train()
        ts = PeriodicTrainStep(model, rho_force=PT.RHO_FORCE, rho_stress=PT.RHO_STRESS)
        assert model.periodic_training is True
        with pytest.raises(ValueError, match=r"targets\['S'\]"):
            ts(PT.batch(structs), dict(E=reference["Et"], F=reference["Ft"]))
        inputs = PT.batch(structs)
        del inputs["cell"]
        with pytest.raises(ValueError, match="periodic batch"):
            ts(inputs, dict(E=reference["Et"], F=reference["Ft"], S=reference["St"]))


def test_eager_optimizer_steps(params, structs, reference):
    """Whole steps (forward, loss, backward, rescale, clip, AdamW) on a periodic batch: the parameters move, the loss stays finite."""
    with PT.emulate():
        model = build(P.CFG, params).train()
        ts = PeriodicTrainStep(model, rho_force=PT.RHO_FORCE, rho_stress=PT.RHO_STRESS)
        inputs, targets = PT.batch(structs), dict(E=reference["Et"], F=reference["Ft"], S=reference["St"])
        before = torch.cat([p.detach().reshape(-1).clone() for p in ts.buf.params])
        losses = [float(ts(inputs, targets)) for _ in range(3)]
    after = torch.cat([p.detach().reshape(-1) for p in ts.buf.params])
    assert all(np.isfinite(losses)) and not torch.equal(before, after)
    np.testing.assert_allclose(losses[0], reference["loss"], rtol=1e-7)


# ------------------------------------------------------------------------------------------------------------ world_size > 1
SHARDS = [[0, 3], [1, 2]]


def _targets(structs):
    oE, oF, oS = PT.offsets(structs)
    return dict(E=torch.tensor(oE), F=torch.tensor(oF), S=torch.tensor(oS))


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        structs = [PT.structures()[i] for i in SHARDS[rank]]
        with PT.emulate():
            model = build(P.CFG, PT.make_params(P.CFG)).train()
            ts = PeriodicTrainStep(model, world_size=world, rho_force=PT.RHO_FORCE, rho_stress=PT.RHO_STRESS)
            loss = ts(PT.batch(structs), _targets(structs), step_optimizer=False)
        lt = loss.clone()
        dist.all_reduce(lt)
        np.save(os.path.join(out_dir, f"grad_{rank}.npy"), ts.buf.flat.numpy())
        np.save(os.path.join(out_dir, f"loss_{rank}.npy"), np.array(float(lt)))
    finally:
        dist.destroy_process_group()


def test_two_rank_gradients_equal_single_process(params, tmp_path):
    """Each rank holds two of the four structures; the stress term is weighted by the GLOBAL structure count like the others."""
    from test_ddp_cpu import _free_port
    order = SHARDS[0] + SHARDS[1]
    structs = [PT.structures()[i] for i in order]
    per_rank = [_targets([PT.structures()[i] for i in s]) for s in SHARDS]
    targets = {k: torch.cat([t[k] for t in per_rank]) for k in ("E", "F", "S")}
    with PT.emulate():
        model = build(P.CFG, params).train()
        ts = PeriodicTrainStep(model, rho_force=PT.RHO_FORCE, rho_stress=PT.RHO_STRESS)
        loss_ref = float(ts(PT.batch(structs), targets, step_optimizer=False))
        ref = ts.buf.flat.clone().numpy()
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    g0, g1 = np.load(tmp_path / "grad_0.npy"), np.load(tmp_path / "grad_1.npy")
    assert np.array_equal(g0, g1)
    np.testing.assert_allclose(g0, ref, rtol=1e-9, atol=1e-12 * np.abs(ref).max())
    np.testing.assert_allclose(float(np.load(tmp_path / "loss_0.npy")), loss_ref, rtol=1e-10)
