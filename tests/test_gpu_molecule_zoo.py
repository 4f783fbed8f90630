"""-m gpu: the full-width molecular models (emb 128 / 128 / 64: the widths every fused kernel takes) on the sparse and
degenerate molecules of tests/molecule_zoo.py against the float64 oracle — atoms of degree 0, edges without triplets or
quadruplets, one-atom molecules, batches with E = 0, atoms that only the interaction cutoff reaches.  Forward and forces, every
structure as a batch of its own, the second-order training pass, the captured runners and a pass under the red-zone harness.

Every bar is one the suite already sets on the dense fixtures (molecule_zoo.FORCE_TOL ...); tests/test_molecule_zoo_cpu.py
holds the float32 oracle to the same bars.  Each test prints its figures before it asserts; docs/MOLECULE_ZOO.md records them."""
import numpy as np
import pytest
import torch

import molecule_zoo as MZ
from gemnet_pytorch_amd.index_device import DeviceGraphBuilder
from oracle import gemnet_oracle as GO
from test_gpu_model import build

pytestmark = pytest.mark.gpu
DEV = "cuda"
NO_EMBEDDING_EDGE = ("atom", "far_dimer")


def _dev(inputs):
    return {k: (v.float() if v.is_floating_point() else v).to(DEV) for k, v in inputs.items()}


def _model(kind, num_blocks=2, train=False):
    cfg = MZ.cfg_full(kind, num_blocks)
    model = build(cfg, MZ.params(cfg))
    return model.train() if train else model.eval()


def _frozen(kind, num_blocks=2):
    model = _model(kind, num_blocks)
    model.requires_grad_(False)
    return model


def _np(t):
    return t.detach().double().cpu().numpy()


def _assert_exact_zeros(E, F, kind, use=None):
    """Structures without an embedding edge: E and F exactly zero (and finite); GemNet-T also on the far atom of cluster+far."""
    off = 0
    z = MZ.zoo()
    for b, n in enumerate(MZ.names(kind) if use is None else use):
        k = len(z[n][0])
        if n in NO_EMBEDDING_EDGE:
            assert np.isfinite(E[b]).all() and np.isfinite(F[off:off + k]).all(), n
            assert not E[b].any() and not F[off:off + k].any(), (n, E[b], F[off:off + k])
        if n == "cluster+far" and kind == "T":
            assert np.isfinite(F[off + k - 1]).all() and not F[off + k - 1].any(), (n, F[off + k - 1])
        off += k


# ------------------------------------------------------------------------------------------------ a. the whole batch
@pytest.mark.parametrize("num_blocks", [2, 4])
@pytest.mark.parametrize("kind", ["T", "Q"])
def test_energy_force_parity_of_the_zoo_batch(kind, num_blocks):
    ref = MZ.reference(kind, num_blocks)
    assert 0.3 <= float(np.abs(ref["F"]).mean()) <= 1.6          # the fixture itself is O(1) eV/A: the bars are literal
    E, F = _model(kind, num_blocks)(_dev(MZ.batch(kind)))
    assert F.is_cuda and not F.requires_grad
    E, F = _np(E), _np(F)
    MZ.assert_force_energy(MZ.force_energy_figures(E, F, ref, kind), f"zoo {kind} x{num_blocks}")
    _assert_exact_zeros(E, F, kind)


# ------------------------------------------------------------------------------------------ b. every structure alone
@pytest.mark.parametrize("kind", ["T", "Q"])
def test_every_structure_as_a_batch_of_its_own(kind):
    """Launches with A = 1, with E = 0 and with empty triplet / quadruplet lists; the oracle is exactly additive over molecules,
    so each result is held to the same rows of the batch reference."""
    ref, model = MZ.reference(kind, 2), _model(kind, 2)
    for n in MZ.names(kind):
        E, F = model(_dev(MZ.batch(kind, only=[n])))
        torch.cuda.synchronize()
        E, F = _np(E), _np(F)
        MZ.assert_force_energy(MZ.force_energy_figures(E, F, ref, kind, sel=[n]), f"{kind} {n} alone")
        _assert_exact_zeros(E, F, kind, use=[n])


# -------------------------------------------------------------------------------------- c. second-order training gradients
def _targets(kind):
    Et, Ft = MZ.targets(kind)
    return Et.float().to(DEV), Ft.float().to(DEV)


def _check_gradients(named, ref, tag):
    bad = [k for k in ref["grads"] if named[k].grad is None or not bool(torch.isfinite(named[k].grad).all())]
    assert not bad, (tag, "missing or non-finite gradients", bad)
    worst, name, rel = MZ.grad_figures({k: named[k].grad for k in ref["grads"]}, ref)
    print(f"{tag}: worst ||g - g_ref|| = {worst:.3f} of its bar ({name}); worst ||g - g_ref|| / ||g_ref|| = {rel:.2e}")
    assert worst <= 1.0, name


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_training_gradients_parity_on_the_zoo(kind):
    ref = MZ.reference(kind, 2, True)
    model = _model(kind, 2, train=True)
    E, F = model(_dev(MZ.batch(kind)))
    assert F.requires_grad
    loss = GO.training_loss(E[:, :1], F, *_targets(kind))
    print(f"zoo {kind}: loss {loss.item():.6f} (float64 {ref['loss']:.6f})")
    np.testing.assert_allclose(loss.item(), ref["loss"], rtol=MZ.LOSS_RTOL)
    loss.backward()
    _check_gradients(dict(model.named_parameters()), ref, f"zoo {kind}")


def test_fused_training_step_on_the_zoo():
    """One eager TrainStep call with the fused optimizer (grouped weight gradients, fused AdamW / EMA) on the T zoo: the same
    loss and gradients, finite parameters afterwards, and the optimizer did step."""
    from gemnet_pytorch_amd.training.ddp import TrainStep
    ref = MZ.reference("T", 2, True)
    ts = TrainStep(_model("T", 2, train=True), fused_optimizer=True)
    before = ts.fused.flat_p.clone()
    Et, Ft = _targets("T")
    loss = float(ts(_dev(MZ.batch("T")), {"E": Et, "F": Ft}))
    torch.cuda.synchronize()
    np.testing.assert_allclose(loss, ref["loss"], rtol=MZ.LOSS_RTOL)
    _check_gradients(dict(ts.model.named_parameters()), ref, "zoo T, fused step")
    assert all(bool(torch.isfinite(p).all()) for p in ts.model.parameters())
    assert not torch.equal(before, ts.fused.flat_p)


# ------------------------------------------------------------------------------------------------- d. captured runners
@pytest.mark.parametrize("kind", ["T", "Q"])
def test_force_graphs_replay_equals_eager(kind):
    from gemnet_pytorch_amd.runtime import ForceGraphs
    model, batch = _frozen(kind), _dev(MZ.batch(kind))
    E0, F0 = model(dict(batch))
    runner = ForceGraphs(model, [batch])
    runner()
    torch.cuda.synchronize()
    E, F = runner.energies_forces()
    assert torch.equal(E, E0) and torch.equal(F, F0), (float((E - E0).abs().max()), float((F - F0).abs().max()))
    _assert_exact_zeros(_np(E), _np(F), kind)


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_padded_runner_replays_two_zoo_batches(kind):
    """Two zoo batches of the same molecule sizes (seeds 5 and 6: other edge, triplet and quadruplet counts) through one
    captured graph, the index build on the device: bit-identical to the eager call, twice around; the capture passes the
    happens-before checker."""
    from gemnet_pytorch_amd.padded import PaddedGraphRunner
    model = _frozen(kind)
    batches = []
    for seed in (5, 6):
        R, Z, N = MZ.arrays(kind, seed)
        R, Z = torch.tensor(R, dtype=torch.float32, device=DEV), torch.tensor(Z, device=DEV).long()
        idx = DeviceGraphBuilder(N, MZ.CUTOFF, MZ.INT_CUTOFF, kind == "T", device=DEV)(R)
        Nd = torch.tensor(N, device=DEV).long()
        E0, F0 = model(dict(Z=Z, R=R.clone(), N=Nd, **idx))
        batches.append((Z, R, Nd, idx, E0.detach().clone(), F0.detach().clone()))
    sizes = [PaddedGraphRunner.sizes_of(b[3]) for b in batches]
    assert torch.equal(batches[0][2], batches[1][2]) and sizes[0][0] != sizes[1][0] and sizes[0][1] != sizes[1][1], sizes
    caps = PaddedGraphRunner.suggest_capacities(sizes)
    runner = PaddedGraphRunner(model, batches[0][0], batches[0][2], caps[0], caps[1], **({} if kind == "T" else dict(quad_caps=caps[2])))
    runner.check = True
    builders = [DeviceGraphBuilder(MZ.arrays(kind)[2], MZ.CUTOFF, MZ.INT_CUTOFF, kind == "T", device=DEV) for _ in batches]
    for rnd in range(2):
        for (Z, R, _, _, E0, F0), bld in zip(batches, builders):
            E, F = runner.build_and_run(bld, R, Z=Z, positions_ready=bool(rnd))
            torch.cuda.synchronize()
            assert torch.equal(E, E0) and torch.equal(F, F0), (rnd, float((E - E0).abs().max()), float((F - F0).abs().max()))
    races, summary = runner.hb.races(), runner.hb.summary()
    print(runner.hb.format(races))
    assert not races and summary["unrecorded_nodes"] == 0 and summary["unresolved_pointers"] == 0
    print(f"padded zoo {kind}: sizes {sizes} at capacities {(runner.e_cap, runner.t_cap) + (runner.quad_caps or ())}")


def _moving_system(step, steps=6):
    """dimer + cluster+far + chain12: the dimer stretched from 1.2 to 7.5 A (its edge vanishes, both atoms end isolated), the
    far atom brought from 11 to 4 A (it gains embedding edges)."""
    z = MZ.zoo()
    use = ["dimer", "cluster+far", "chain12"]
    R = [z[n][0].copy() for n in use]
    s = step / (steps - 1)
    R[0] = np.array([[0.0, 0.0, 0.0], [1.2 + (7.5 - 1.2) * s, 0.0, 0.0]])
    R[1][-1] = [11.0 + (4.0 - 11.0) * s, 1.0, 1.0]
    return np.concatenate(R), np.concatenate([z[n][1] for n in use]), np.array([len(r) for r in R], np.int64)


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_dynamic_force_field_follows_a_dissociating_system(kind):
    from gemnet_pytorch_amd.runtime import DynamicForceField
    model = _frozen(kind)
    _, Z, N = _moving_system(0)
    Z, Nd = torch.tensor(Z, device=DEV).long(), torch.tensor(N, device=DEV).long()
    ff = DynamicForceField(model, Z, N, MZ.CUTOFF, MZ.INT_CUTOFF)
    sizes = []
    for step in range(6):
        R = torch.tensor(_moving_system(step)[0], dtype=torch.float32, device=DEV)
        E, F = ff(R)
        idx = DeviceGraphBuilder(N, MZ.CUTOFF, MZ.INT_CUTOFF, kind == "T", device=DEV)(R)
        E0, F0 = model(dict(Z=Z, R=R.clone(), N=Nd, **idx))
        torch.cuda.synchronize()
        sizes.append(int(idx["id_c"].shape[0]))
        assert torch.equal(E, E0.detach()) and torch.equal(F, F0.detach()), (step, float((F - F0).abs().max()))
    print(f"dissociating system {kind}: edges per step {sizes}, graphs re-captured {ff.recaptures} time(s)")
    assert len(set(sizes)) > 2
    assert float(E[0].abs().max()) == 0.0 and float(F[:2].abs().max()) == 0.0          # the dimer ended as two isolated atoms


# --------------------------------------------------------------------------------------------------- e. red-zone pass
@pytest.mark.parametrize("kind", ["T", "Q"])
def test_forward_and_forces_under_the_red_zone_harness(kind):
    """Every tensor of the pass between two bands of 0xFF and every `empty` payload NaN until a kernel writes it: finite and
    bit-equal to the plain pass (the path has no atomics)."""
    from redzone import guard, put
    model, inputs = _model(kind), MZ.batch(kind)
    E0, F0 = model(_dev(inputs))
    with guard(DEV) as rz:
        E, F = model({k: put(v.float() if v.is_floating_point() else v) for k, v in inputs.items()})
        torch.cuda.synchronize()
    print(f"zoo {kind}: {rz.n_launches} launches checked ({rz.n_operands} guarded operands), {rz.n_guarded} allocations guarded")
    assert rz.n_launches > 0 and rz.n_operands > rz.n_launches and rz.tracing
    for a, b in ((E, E0), (F, F0)):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


def test_training_backward_under_the_red_zone_harness():
    from redzone import guard, put
    ref = MZ.reference("T", 2, True)
    inputs, (Et, Ft) = MZ.batch("T"), MZ.targets("T")
    with guard(DEV) as rz:
        model = _model("T", 2, train=True)
        E, F = model({k: put(v.float() if v.is_floating_point() else v) for k, v in inputs.items()})
        loss = GO.training_loss(E[:, :1], F, put(Et.float()), put(Ft.float()))
        loss.backward()
        torch.cuda.synchronize()
    print(f"zoo T training pass: {rz.n_launches} launches checked ({rz.n_operands} guarded operands)")
    assert rz.n_launches > 0 and rz.tracing
    np.testing.assert_allclose(loss.item(), ref["loss"], rtol=MZ.LOSS_RTOL)
    _check_gradients(dict(model.named_parameters()), ref, "zoo T under the harness")
