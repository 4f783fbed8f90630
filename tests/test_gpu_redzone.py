"""-m gpu: whole passes and tile-edge kernel cases under the red-zone harness (tests/redzone.py), and the harness itself on
the device.

Whole passes run eagerly (no capture) on the small golden fixtures with every tensor of the pass — inputs, parameters'
packed forms, every intermediate a launcher allocates — between two 128 KiB bands of 0xFF, and every `empty` payload 0xFF
(NaN) until a kernel writes it.  Each pass asserts that the harness stayed silent (a report raises) and that the result
meets the bar of the fixture's own parity test: with unwritten memory NaN, that bar is what catches a read before a write.
The tile-edge cases take the float64 references and the tolerances of their sibling tests in test_gpu_kernels.py /
test_gpu_bil_up.py / test_gpu_index.py at the smallest sizes that straddle a tile."""
import numpy as np
import pytest
import torch

import cpu_kernels as CK
import pbc_common as P
from conftest import check_grad_probes
from gemnet_pytorch_amd import _lib
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd.graph import RowIndex, SegmentPlan
from oracle import index_oracle as IO
from redzone import RedzoneError, guard, put
from test_oracle_model import load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------------------------- the harness itself
def test_a_gather_one_row_past_its_output_is_reported():
    """gn_gather_rows_f32 with T one larger than y has rows (idx and x are large enough): the extra row lands in y's own after
    band — inside this test's allocation by construction — and the report names entry point, operand, band and offset.
    Without this test a harness that silently resolved no pointer would pass everything."""
    with pytest.raises(RedzoneError, match=r"gn_gather_rows_f32: operand y \(torch.empty, 64 B payload\): after band damaged, "
                                           r"first byte at offset 0$"):
        with guard(DEV) as rz:
            x = put(torch.ones(8, 4))                       # 1.0f = 0x3f800000: no byte of it is 0xFF
            idx = put(torch.tensor([3, 1, 7, 0, 5], dtype=torch.int32))
            y = torch.empty(4, 4, device=DEV)
            assert rz.find(y.data_ptr()) is not None and bool(torch.isnan(y).all())
            _lib.load().gn_gather_rows_f32(_lib.ptr(x), _lib.ptr(idx), _lib.ptr(y), 5, 4, _lib.stream())
    assert rz.n_launches == 1 and rz.n_operands == 3


def test_a_clean_launch_is_silent_and_the_allocators_come_back():
    real = torch.empty
    with guard(DEV) as rz:
        x, idx = put(torch.randn(8, 4)), put(torch.tensor([3, 1, 7, 0], dtype=torch.int32))
        y = K.gather(x, idx)
        assert rz.find(y.data_ptr()) is not None and torch.equal(y, x[idx.long()])
    assert rz.n_launches == 1 and rz.n_operands == 3 and torch.empty is real and _lib.TRACE is None


# ------------------------------------------------------------------------------------------------------------- whole passes
def _build(cfg, params):
    from test_gpu_model import build
    return build(cfg, params)


def _report(tag, rz):
    print(f"{tag}: {rz.n_launches} launches checked ({rz.n_operands} guarded operands), {rz.n_guarded} allocations guarded")
    assert rz.n_launches > 0 and rz.n_operands > rz.n_launches and rz.tracing


@pytest.mark.parametrize("tag", ["t1", "t2", "q1", "dt1"])
def test_molecular_forward_and_forces(golden_model, golden_model2, tag):
    """Bars of test_gpu_model.test_energy_force_parity (t1, q1, dt1: 1e-5 eV/A absolute) and, for t2 with its raw test weights,
    of test_relative_precision_on_unscaled_deep_fixtures (1e-5 of mean |F_ref|); energy 2e-5 of max(1, max |E_ref|).  (dt1, the
    direct-force fixture, is stored in tests/golden/model2.npz.)"""
    g = golden_model2 if f"{tag}.E" in golden_model2 else golden_model
    cfg, params, inputs = load_case(g, tag)
    with guard(DEV) as rz:
        model = _build(cfg, params).eval()
        E, F = model({k: put(v) for k, v in inputs.items()})
        torch.cuda.synchronize()
    _report(tag, rz)
    Eref, Fref = g[f"{tag}.E"], g[f"{tag}.F"]
    f_mae = float(np.abs(F.detach().cpu().numpy() - Fref).mean())
    e_err = float(np.abs(E.detach().cpu().numpy() - Eref).max())
    print(f"{tag}: force MAE {f_mae:.3e}, energy err {e_err:.3e}")
    assert f_mae <= 1e-5 * (float(np.abs(Fref).mean()) if tag == "t2" else 1.0)
    assert e_err <= 2e-5 * max(1.0, float(np.abs(Eref).max()))


@pytest.mark.parametrize("tag", ["t2", "q1"])
def test_molecular_fused_training_step(golden_model, tag):
    """One eager TrainStep(fused_optimizer=True) call, optimizer included.  Bars of test_gpu_model.test_training_gradients_parity:
    loss rtol 2e-5, per-parameter gradient norms rtol 2e-3 (atol 1e-6 of the largest), the +-1 probe projections at 2e-3.  (The
    fused optimizer reads the gradients as `const`: they are still the step's raw gradients afterwards.)"""
    from gemnet_pytorch_amd.training.ddp import TrainStep
    g = golden_model
    cfg, params, inputs = load_case(g, tag)
    with guard(DEV) as rz:
        ts = TrainStep(_build(cfg, params), fused_optimizer=True)
        before = ts.fused.flat_p.clone() if hasattr(ts.fused, "flat_p") else None
        targets = dict(E=put(torch.tensor(g[f"{tag}.Et"]).float())[:, None], F=put(torch.tensor(g[f"{tag}.Ft"]).float()))
        loss = float(ts({k: put(v) for k, v in inputs.items()}, targets))
        torch.cuda.synchronize()
    _report(tag + " training step", rz)
    np.testing.assert_allclose(loss, float(g[f"{tag}.loss"]), rtol=2e-5)
    named = dict(ts.model.named_parameters())
    names = [str(n) for n in g[f"{tag}.grad_names"]]
    norms = np.array([0.0 if named[n].grad is None else float(named[n].grad.norm()) for n in names])
    ref = g[f"{tag}.grad_norms"]
    np.testing.assert_allclose(norms, ref, rtol=2e-3, atol=1e-6 * float(ref.max()))
    worst = check_grad_probes(g, tag, {n: named[n].grad for n in names}, rtol=2e-3)
    print(f"{tag}: loss {loss:.6f}; worst probe error / (2e-3 ||g_ref||) = {worst:.3f}")
    assert all(bool(torch.isfinite(p).all()) for p in ts.model.parameters())
    assert before is None or not torch.equal(before, ts.fused.flat_p)          # the optimizer did step


def test_periodic_t_forward_forces_stress():
    """'bcc_pert' (exactly planar and collinear triplets, |n| up to 3) against tests/golden/pbc_cases.npz with the bars of
    test_gpu_pbc_cases.test_energy_forces_stress_match_golden_cluster_oracle."""
    import test_gpu_pbc_cases as C
    g, kind = C._golden(), "bcc_pert"
    with guard(DEV) as rz:
        model = C._new_model()
        E, F, S = model(C._batch([P.structure(kind)]), stress=True)
        torch.cuda.synchronize()
    _report("periodic T " + kind, rz)
    E, F, S = E.double().cpu().numpy(), F.double().cpu().numpy(), S.double().cpu().numpy()
    E_ref, F_ref, S_ref = float(g[kind + ".E"]), g[kind + ".F"], g[kind + ".S"]
    scale = max(1.0, float(np.abs(F_ref).mean()))
    assert abs(E[0, 0] - E_ref) <= 2e-5 * max(1.0, abs(E_ref))
    assert np.abs(F - F_ref).mean() <= 1e-5 * scale and np.abs(F - F_ref).max() <= 1e-4 * scale
    assert np.abs(S[0] - S_ref).max() <= 1e-4 * max(np.abs(S_ref).max(), 1e-2)


def test_periodic_q_forward_forces_stress():
    """'thin' (self-image interaction edges, exactly collinear c - a - b) against tests/golden/pbc_q_cases.npz with the bars of
    test_gpu_pbc_q.test_energy_forces_stress_match_cluster_oracle."""
    import os
    import pbc_q_common as Q
    import test_gpu_pbc_q as TQ
    from conftest import GOLDEN, SCALE_FILE
    from gemnet_pytorch_amd.model.gemnet import GemNet
    from oracle import gemnet_oracle as GO
    g, tag, kind = np.load(os.path.join(GOLDEN, "pbc_q_cases.npz")), "q", "thin"
    with guard(DEV) as rz:
        model = GemNet(**Q.CFGS[tag], scale_file=SCALE_FILE)
        model.load_state_dict(GO.expand_to_reference_state_dict({k: v.float() for k, v in Q.make_params(Q.CFGS[tag]).items()}))
        model.periodic_quadruplets = True
        E, F, S = model.to(DEV).eval()(TQ._batch([P.structure(kind)]), stress=True)
        torch.cuda.synchronize()
    _report("periodic Q " + kind, rz)
    E, F, S = E.double().cpu().numpy(), F.double().cpu().numpy(), S.double().cpu().numpy()
    E_ref, F_ref, S_ref = (g[f"{tag}.{kind}.{k}"] for k in "EFS")
    scale, sS = max(1.0, float(np.abs(F_ref).mean())), max(np.abs(S_ref).max(), 1e-2)
    assert abs(E[0, 0] - float(E_ref)) <= 2e-5 * max(1.0, abs(float(E_ref)))
    assert np.abs(F - F_ref).mean() <= 1e-5 * scale and np.abs(F - F_ref).max() <= 1e-4 * scale
    assert np.abs(S[0] - S_ref).max() <= 1e-4 * sS


def test_periodic_zoo_batch_forward_forces_stress():
    """The 46-structure 'zoo' (1, 2, 63, 64, 65, ~130 atoms, empty lists).  It has no stored oracle; the path has no atomics and
    two runs are bit-identical (test_gpu_model.test_repeatable_bitwise), so the pass under the harness must equal the plain pass
    bit for bit and be finite: a NaN read from an unwritten payload, or a stray write into a neighbour, breaks either."""
    import test_gpu_pbc_cases as C
    model, structs = C._new_model(), P.zoo()
    E0, F0, S0 = model(C._batch(structs), stress=True)
    with guard(DEV) as rz:
        E, F, S = model(C._batch(structs), stress=True)
        torch.cuda.synchronize()
    _report("periodic T zoo", rz)
    for a, b in ((E, E0), (F, F0), (S, S0)):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


def test_periodic_t_fused_training_step():
    """The 4-structure batch of test_gpu_pbc_train on the wide configuration (fused bilinear training Function, chain programs,
    tangent kernels), energy + force + stress loss, one eager PeriodicTrainStep call with the optimizer.  Bars of
    test_gpu_pbc_train.test_parameter_gradients_match_the_oracle; the float64 oracle is that module's, computed once."""
    import pbc_train_common as PT
    import test_gpu_pbc_train as TT
    from gemnet_pytorch_amd.training.periodic import PeriodicTrainStep
    ref = TT._reference("wide")
    with guard(DEV) as rz:
        ts = PeriodicTrainStep(TT._model("wide"), rho_force=PT.RHO_FORCE, rho_stress=PT.RHO_STRESS, fused_optimizer=True)
        loss = float(ts(TT._batch(), {k: put(v) for k, v in TT._targets(ref).items()}))
        torch.cuda.synchronize()
    _report("periodic T training step", rz)
    np.testing.assert_allclose(loss, ref["loss"], rtol=2e-5)
    g, gref = TT._gradients(ts), ref["grads"]
    assert set(g) == set(gref)
    atol = 1e-6 * max(float(v.norm()) for v in gref.values())
    names = sorted(gref)
    np.testing.assert_allclose([float(g[n].norm()) for n in names], [float(gref[n].norm()) for n in names], rtol=2e-3, atol=atol)
    ratio = {n: float((g[n] - gref[n]).norm()) / (2e-3 * float(gref[n].norm()) + atol) for n in gref}
    assert max(ratio.values()) <= 1.0, max(ratio, key=ratio.get)
    assert all(bool(torch.isfinite(p).all()) for p in ts.model.parameters())


# ------------------------------------------------------------------------------------------------- tile-edge kernel cases
# Sizes are the smallest that straddle a tile; references and tolerances are those of the sibling test named in each docstring.
from redzone import redzone_on_request  # noqa: E402,F401  (the tests below ask for `redzone`)
from test_gpu_kernels import close, f32, rnd  # noqa: E402


@pytest.mark.parametrize("mode", ["f32", "split6", "h3", "h3/row"])
@pytest.mark.parametrize("M,width", [(m, w) for w in (64, 128) for m in (1, 15, 16, 17, 79, 80, 81)]
                         + [(18079, 128), (18080, 128), (18081, 128)])
def test_chain_kernel_at_row_tile_edges(M, width, mode, monkeypatch, redzone):
    """test_gpu_kernels.test_chain_kernel_vs_interpreter (same programs, same CHAIN_TOL) at row-tile edges.  The launchers take
    RT = ceil(M / 4096) (csrc/chain.hip, chain2.hip: one round of <= 256 workgroups), so the tile is 16 rows up to M = 4096 and
    M = 1 .. 81 straddles one to six 16-row tiles; the 80-row tile (RT = 5) exists for 16 384 < M <= 20 480 only, where
    M = 18 080 = 226 x 80 and its two neighbours straddle it."""
    from test_gpu_kernels import _chain_vs_interpreter
    _chain_vs_interpreter(M, width, mode, monkeypatch)


@pytest.mark.parametrize("N", [4096, 4097])          # workgroup-per-row up to 4096 rows, wave-per-row above
@pytest.mark.parametrize("C", [3, 4, 128])
def test_segmented_sums_with_one_segment_holding_every_entry(N, C, redzone):
    """test_gpu_kernels.test_gather_segsum / test_segsum_multi_matches_separate_sums at the switch between the two kernels, with
    float4 (C = 4, 128) and scalar (C = 3) rows; T = 333 entries all in the last row (every other segment empty), and all in
    row 0 for a second, sorted term of the multi-sum."""
    g = torch.Generator().manual_seed(N + C)
    T = 333
    y = rnd(g, T, C)
    idx = torch.full((T,), N - 1)
    ri = RowIndex(put(idx), N)
    perm, seg = ri.csr
    ref = torch.zeros(N, C, dtype=torch.float64).index_add(0, idx, y)
    out = K.segsum(f32(y), perm, seg, N)
    close(out, ref)
    assert float(out[:N - 1].abs().max()) == 0.0
    if C <= 4:
        y2 = rnd(g, T, C)
        seg2 = torch.full((N + 1,), T, dtype=torch.int32)
        seg2[0] = 0                                     # sorted keys, all 0: perm = None
        ref2 = ref - 0.5 * torch.zeros(N, C, dtype=torch.float64).index_add(0, torch.zeros(T, dtype=torch.long), y2)
        out2 = K.segsum_multi([(f32(y), perm, seg, 1.0), (f32(y2), None, put(seg2), -0.5)], N)
        close(out2, ref2, rtol=1e-5, atol=1e-5 * max(1.0, float(ref2.abs().max())))
        assert float(out2[1:N - 1].abs().max()) == 0.0


SEG = (0, 1, 8, 9, 33)               # the segment lengths of test_gpu_bil_up.py: empty, one, half a tile +- , two tiles + 1


def _plans(E, J, lens, g):
    lens = torch.tensor(lens)
    red = torch.repeat_interleave(torch.arange(E), lens)
    exp = torch.randint(0, J, (red.shape[0],), generator=g)
    return SegmentPlan(red, exp, E, J), SegmentPlan(put(red), put(exp), E, J)


@pytest.mark.parametrize("shift", [0, 1, 4], ids=["first=0", "first=1", "first=33"])
@pytest.mark.parametrize("E", [1, 15, 16, 17])
def test_bilinear_project_kernels_at_edge_tile_edges(E, shift, redzone):
    """bil_reduce_project, bil_project_bwd (with dY, without, accumulating into gB and into dY), bil_fused_fwd, bil_fused_bwd and
    bil_dy_multi with E around the 16-edge tile and segments of SEG[(e + shift) % 5] triplets: lengths 0, 1 and 33 come first,
    in the middle and last.  Tolerances: test_gpu_kernels.test_bilinear_fused_project_kernels,
    test_bilinear_adjoint_accumulates_y_gradient, test_bilinear_forward_fused_with_the_final_projection,
    test_bilinear_tail_adjoint_one_launch, test_bilinear_deferred_y_gradient_of_several_blocks."""
    S, C, I, O = 7, 64, 16, 64
    g = torch.Generator().manual_seed(100 * E + shift)
    cpu, dev = _plans(E, E, [SEG[(e + shift) % len(SEG)] for e in range(E)], g)
    T = cpu.size
    Y, x, Bm, dP, dP2 = rnd(g, T, S), rnd(g, E, C), rnd(g, E, S, I), rnd(g, E, I, C), rnd(g, E, I, C)
    amax = lambda t: float(t.abs().max()) if t.numel() else 0.0          # noqa: E731
    Sm, Pm = K.bil_reduce_project(f32(Y), f32(x), f32(Bm), dev)
    rSm, rP = CK.bil_reduce_project(Y, x, Bm, cpu)
    close(Sm, rSm, atol=1e-4); close(Pm, rP, atol=2e-4 * amax(rP))
    gB, dSm, dY = K.bil_project_bwd(f32(dP), f32(rSm), f32(Bm), f32(x), dev)
    rgB, rdSm, rdY = CK.bil_project_bwd(dP, rSm, Bm, x, cpu)
    close(gB, rgB, atol=2e-4 * amax(rgB)); close(dSm, rdSm, atol=1e-4); close(dY, rdY, atol=2e-4 * amax(rdY))
    gB2, dSm2, none = K.bil_project_bwd(f32(dP), f32(rSm), f32(Bm), f32(x), dev, want_dY=False)
    assert none is None and torch.equal(gB2, gB) and torch.equal(dSm2, dSm)
    base = f32(rnd(g, E, S, I))
    run = base.clone()
    gB3, _, _ = K.bil_project_bwd(f32(dP), f32(rSm), f32(Bm), f32(x), dev, want_dY=False, gB_accum=run)
    assert gB3 is run and torch.equal(run, base + gB)
    _, _, dY2 = K.bil_project_bwd(f32(dP2), f32(rSm), f32(Bm), f32(x), dev, dY_accum=dY)
    assert dY2.data_ptr() == dY.data_ptr()
    racc = rdY + CK.bil_project_bwd(dP2, rSm, Bm, x, cpu)[2]
    close(dY2, racc, atol=2e-4 * max(1.0, amax(racc)))
    # forward and tail adjoint in one launch each, f32 MFMA and fp16 planes
    W2T = rnd(g, O, I * C) / 32
    rSm1, rout = CK.bil_fused_fwd(Y, x, Bm, W2T, cpu, alpha=0.6)
    for planes in (None, K.pack_weight_split(f32(W2T), fmt=1)):
        Sm1, out = K.bil_fused_fwd(f32(Y), f32(x), f32(Bm), f32(W2T), dev, alpha=0.6, W2T_planes=planes)
        assert torch.equal(Sm1, Sm)
        close(out, rout, atol=3e-4 * max(1.0, amax(rout)))
    gr, W2 = rnd(g, E, O), rnd(g, I * C, O) / 8
    ref = CK.bil_fused_bwd(gr, W2, rSm, Bm, 0.7)
    gB4, dSm4 = K.bil_fused_bwd(f32(gr), f32(W2), f32(rSm), f32(Bm), 0.7)
    close(gB4, ref[0], atol=2e-4 * amax(ref[0])); close(dSm4, ref[1], atol=2e-4 * amax(ref[1]))
    run = base.clone()
    gB5, _ = K.bil_fused_bwd(f32(gr), f32(W2), f32(rSm), f32(Bm), 0.7, gB_accum=run)
    assert gB5 is run and torch.equal(run, base + gB4)
    # the deferred Y gradient of two blocks
    dS2, x2 = rnd(g, E, S, C), rnd(g, E, C)
    rY = CK.bil_project_bwd(dP, rSm, Bm, x, cpu)[2] + CK.bil_dy_multi([dS2], [x2], cpu)
    got = K.bil_dy_multi([dSm, f32(dS2)], [f32(x), f32(x2)], dev)
    close(got, rY, atol=3e-4 * max(1.0, amax(rY)))


ANG_SEG = (0, 1, 15, 16, 17, 31, 32, 33, 65)          # around the 16- and 32-quadruplet tiles and past the 64-row expand tile


@pytest.mark.parametrize("mask", [7, 0], ids=["f16 (default)", "f32-mfma"])
@pytest.mark.parametrize("E", [1, 17])
def test_angle_form_kernels_at_quadruplet_tile_edges(E, mask, monkeypatch, redzone):
    """test_gpu_kernels.test_tensor_basis_angle_form_kernels and test_tensor_basis_tangent_kernels_of_force_training (their
    references and tolerances) with E = 17 edges whose segments run through ANG_SEG (the empty one first, 65 in the middle, the
    lengths again to the end), and with E = 1 once per length — in both arithmetics of kernels.ANG_F16_MASK."""
    monkeypatch.setattr(K, "ANG_F16_MASK", mask)
    S, C, I, J = 49, 32, 32, 40
    for lens in ([ANG_SEG[e % len(ANG_SEG)] for e in range(E)],) if E > 1 else [(n,) for n in ANG_SEG]:
        g = torch.Generator().manual_seed(E * 1000 + lens[0])
        cpu, dev = _plans(E, J, lens, g)
        Q = cpu.size
        th, ph = torch.rand(Q, generator=g, dtype=torch.float64) * 3.0 + 0.05, torch.rand(Q, generator=g, dtype=torch.float64) * 3.1
        ang = torch.stack([torch.sin(th), torch.cos(th), torch.sin(ph), torch.cos(ph)], 1)
        x, B_, D = rnd(g, J, C), rnd(g, E, S, I), rnd(g, E, S, C)
        Sm, Pm = K.bil_reduce_project(f32(ang), f32(x), f32(B_), dev)
        Sm_ref, P_ref = CK.bil_reduce_project(ang, x, B_, cpu)
        close(Sm, Sm_ref, atol=2e-5 * max(1.0, float(Sm_ref.abs().max())))
        close(Pm, P_ref, atol=2e-5 * max(1.0, float(P_ref.abs().max())))
        dx_ref = CK.bil_reduce_t(ang, D, cpu)
        close(K.bil_reduce_t(f32(ang), f32(D), dev), dx_ref, atol=2e-5 * max(1.0, float(dx_ref.abs().max())))
        Ds, xs = [rnd(g, E, S, C) for _ in range(3)], [rnd(g, J, C) for _ in range(3)]
        for nb in (1, 3):
            g_ref = CK.bil_dy_multi(Ds[:nb], xs[:nb], cpu, ang=ang)
            got = K.bil_dy_multi([f32(d) for d in Ds[:nb]], [f32(v) for v in xs[:nb]], dev, ang=f32(ang))
            close(got, g_ref, atol=3e-5 * max(1.0, float(g_ref.abs().max()) if Q else 0.0))
        # tangent kernels
        tx, tB, D2 = rnd(g, J, C), rnd(g, E, S, I), rnd(g, E, S, C)
        tang = torch.zeros(Q, 4, dtype=torch.float64)
        tang[:, 0:2] = rnd(g, Q, 2)
        Smd_ref, Pd_ref = CK.bil_reduce_project_tan(ang, tang, x, tx, B_, tB, Sm_ref, cpu)
        Smd, Pd = K.bil_reduce_project_tan(f32(ang), f32(tang), f32(x), f32(tx), f32(B_), f32(tB), f32(Sm_ref), dev)
        close(Smd, Smd_ref, atol=3e-5 * max(1e-30, float(Smd_ref.abs().max())), rtol=0)
        close(Pd, Pd_ref, atol=3e-5 * max(1e-30, float(Pd_ref.abs().max())), rtol=0)
        for D1 in (D, None):
            ref = CK.bil_reduce_t_tan(ang, tang, D1, D2, cpu)
            got = K.bil_reduce_t_tan(f32(ang), f32(tang), None if D1 is None else f32(D1), f32(D2), dev)
            close(got, ref, atol=3e-5 * float(ref.abs().max()), rtol=0)


@pytest.mark.parametrize("name,n_atoms,E,target", [("one atom", 1, 37, 0), ("first of two holds every edge", 2, 300, 0),
                                                   ("all empty but the last", 37, 100, 36)])
def test_rbf_aggregate_with_every_edge_on_one_atom(name, n_atoms, E, target, redzone):
    """test_gpu_kernels.test_rbf_aggregate_fused_vs_reference_ops (float64 composition, its tolerances) and the grouped forms
    against the single launches as in test_gpu_out_group (forward bit-identical, g_rbf within G * 2^-23 * sum |term|)."""
    g = torch.Generator().manual_seed(E)
    G = 2
    id_a = torch.full((E,), target)
    ms, Ws, gos = [rnd(g, E, 128) for _ in range(G)], [rnd(g, 128, 16) / 4 for _ in range(G)], [rnd(g, n_atoms, 128) for _ in range(G)]
    rbf = rnd(g, E, 16)
    scales = [0.37, 1.25]
    ia = put(id_a.to(torch.int32))
    perm, seg = K.csr_build(ia, n_atoms)
    outs, bwds = [], []
    for m, W, go, sc in zip(ms, Ws, gos, scales):
        ref = torch.zeros(n_atoms, 128, dtype=torch.float64).index_add(0, id_a, m * (rbf @ W.t())) * sc
        out = K.rbf_aggregate_fwd(f32(m), f32(rbf), f32(W), perm, seg, n_atoms, sc)
        close(out, ref, rtol=1e-5, atol=1e-5 * max(1.0, float(ref.abs().max())))
        assert n_atoms == 1 or float(out[torch.arange(n_atoms) != target].abs().max()) == 0.0
        gm, gr = K.rbf_aggregate_bwd(f32(go), f32(m), f32(rbf), f32(W), ia, sc)
        gsel = go[id_a] * sc
        close(gm, gsel * (rbf @ W.t()), rtol=1e-5, atol=1e-5)
        close(gr, (gsel * m) @ W, rtol=1e-5, atol=2e-5 * max(1.0, float(((gsel * m) @ W).abs().max())))
        base_m, base_r = f32(rnd(g, E, 128)), f32(rnd(g, E, 16))
        run_m, run_r = base_m.clone(), base_r.clone()
        gm3, gr3 = K.rbf_aggregate_bwd(f32(go), f32(m), f32(rbf), f32(W), ia, sc, acc_m=run_m, acc_rbf=run_r)
        assert gm3 is run_m and gr3 is run_r and torch.equal(gm3, base_m + gm) and torch.equal(gr3, base_r + gr)
        outs.append(out), bwds.append((gm, gr))
    sc_dev = put(torch.tensor(scales))
    sc32 = [float(v) for v in sc_dev.cpu()]
    single = [K.rbf_aggregate_fwd(f32(m), f32(rbf), f32(W), perm, seg, n_atoms, s) for m, W, s in zip(ms, Ws, sc32)]
    grouped = K.rbf_aggregate_grouped_fwd([f32(m) for m in ms], f32(rbf), [f32(W) for W in Ws], sc_dev, perm, seg, n_atoms)
    assert all(torch.equal(grouped[i], single[i]) for i in range(G))
    g_out = f32(torch.stack(gos))
    g_m, g_rbf = K.rbf_aggregate_grouped_bwd(g_out, [f32(m) for m in ms], f32(rbf), [f32(W) for W in Ws], sc_dev, ia)
    terms = []
    for i in range(G):
        gm1, gr1 = K.rbf_aggregate_bwd(g_out[i], f32(ms[i]), f32(rbf), f32(Ws[i]), ia, sc32[i])
        assert torch.equal(g_m[i], gm1)
        terms.append(gr1.double())
    terms = torch.stack(terms)
    assert ((g_rbf.double() - terms.sum(0)).abs() <= G * 2.0 ** -23 * terms.abs().sum(0)).all()


@pytest.mark.parametrize("n,triplets_only", [(63, True), (64, True), (65, True), (130, True), (63, False), (64, False), (65, False)])
def test_index_builder_on_molecules_around_and_beyond_64_atoms(n, triplets_only, redzone):
    """test_gpu_index._check (bit-exact integers against oracle.index_oracle) on a molecule of n atoms batched between a 1-atom
    and a 2-atom molecule: nothing larger than 64 atoms per molecule went through the molecular device builder before."""
    from gemnet_pytorch_amd.synthetic import make_molecule
    from test_gpu_index import _check
    mols = [make_molecule(k, 700 + i) for i, k in enumerate((1, n, 2))]
    R = np.concatenate([m["R"] for m in mols]).astype(np.float32)
    _check(R, np.array([len(m["R"]) for m in mols]), triplets_only)


@pytest.mark.parametrize("M", [1, 12, 33])
@pytest.mark.parametrize("N", [8, 24, 100])
def test_f32_chain_kernel_with_an_output_width_that_is_no_multiple_of_16(M, N, redzone):
    """Found by the harness (gn_chain_f32, ops[4].pre_out, M = 12, N = 8: the down projection of a model with emb_size_trip = 8):
    the lanes of the last active wave whose column is >= N stored through row * N + col, into the next row and, after the last
    row, past the end of pre_out / out / out2.  Dense -> Hadamard -> Dense with N columns as ops._DenseHadamardDown builds it,
    plus a second output, against the float64 interpreter with the bar of test_gpu_kernels.test_chain_kernel_vs_interpreter."""
    from test_gpu_kernels import CHAIN_TOL
    g = torch.Generator().manual_seed(M * N)
    x, rbf, Wa, Wr, Wd = rnd(g, M, 16), rnd(g, M, 16), rnd(g, 16, 16) / 4, rnd(g, 16, 16) / 4, rnd(g, N, 16) / 4
    Z2 = rnd(g, M, N)

    def build(conv):
        t = {k: conv(v) for k, v in dict(x=x, rbf=rbf, Wa=Wa, Wr=Wr, Wd=Wd, Z2=Z2).items()}
        outs = {k: conv(torch.zeros(M, w, dtype=torch.float64)) for k, w in (("z1", 16), ("r", 16), ("z3", N), ("y", N), ("y2", N))}
        p = K.ChainProgram(M)
        p.load(0, t["x"])
        p.gemm(t["Wa"], a_slot=0, y_slot=1, act=True, pre_out=outs["z1"])
        p.load(0, t["rbf"])
        p.gemm(t["Wr"], a_slot=0, y_slot=0, pre_out=outs["r"], mul=1, alpha=0.8)
        p.gemm(t["Wd"], a_slot=0, y_slot=-1, act=True, pre_out=outs["z3"], out=outs["y"], alpha2=0.9, Z2=t["Z2"], mode2=1,
               out2=outs["y2"])
        return p, outs
    p_ref, o_ref = build(lambda t: t.clone())
    p_dev, o_dev = build(f32)
    CK.chain(p_ref, mode="f32")
    K.chain(p_dev, mode="f32")
    for k in o_ref:
        err = float((o_dev[k].double().cpu() - o_ref[k]).abs().max()) / max(1.0, float(o_ref[k].abs().max()))
        assert err <= 2 * CHAIN_TOL["f32"], (k, err)
