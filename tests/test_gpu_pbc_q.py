"""GPU: periodic cells for GemNet-Q (model.periodic_quadruplets) — the vector-form geometry kernels of csrc/pbc_quad.hip and
their reduction against fp64 torch autograd on the same vectors, energy / forces / stress against the golden cluster oracle
(tests/golden/pbc_q_cases.npz, both parameter sets), consistency, the captured force graph and the cases that must raise."""
import os

import numpy as np
import pytest
import torch

import cpu_kernels as CK
import pbc_common as P
import pbc_q_common as Q
from conftest import GOLDEN, SCALE_FILE
from oracle import basis_oracle as B
from oracle import gemnet_oracle as GO
from redzone import put, redzone_on_request  # noqa: F401  (the kernel-level tests below ask for `redzone`: they run under the red-zone harness)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _batch(structs, **extra):
    from gemnet_pytorch_amd.pbc import PeriodicQuadGraphBuilder
    R, Z, N, cell, pbc = P.arrays(structs)
    b = PeriodicQuadGraphBuilder(N, Q.CUTOFF, Q.INT_CUTOFF, pbc=pbc, device=DEV)
    inputs = b(torch.tensor(R, device=DEV), torch.tensor(cell, device=DEV))
    inputs.update(R=torch.tensor(R, dtype=torch.float32, device=DEV), Z=torch.tensor(Z, device=DEV).long(),
                  N=torch.tensor(N, device=DEV), cell=torch.tensor(cell, dtype=torch.float32, device=DEV), **extra)
    return inputs


# ----------------------------------------------------------------------------------------------------------------- kernels
@pytest.fixture(scope="module")
def geometry():
    """Index arrays and f32 vectors of the batch ['bcc_pert', 'thin'] (5 848 quadruplets; 'thin': self-image interaction
    edges, repeated (c, a) pairs, exactly collinear c - a - b; the first rows, which the small counts take, are bcc_pert's)."""
    from gemnet_pytorch_amd import pbc
    from gemnet_pytorch_amd.graph import GraphPlan
    inputs = _batch([P.structure("bcc_pert"), P.structure("thin")])
    plan = GraphPlan(inputs, False)
    V = pbc.edge_vectors(inputs["R"], plan, inputs["cell"])
    Vint = pbc.int_edge_vectors(inputs["R"], plan, inputs["cell"])
    thin = Q.brute_force_q(*[P.arrays([P.structure("thin")])[i] for i in (0, 2, 3, 4)])
    assert len(thin["id4_reduce_ca"]) > 65 and (thin["id4_int_a"] == thin["id4_int_b"]).any()
    return inputs, V, Vint


def _sub_plan(inputs, quads=slice(None), intm=None):
    """The batch's plan with only the quadruplets `quads` (a slice or an ascending index tensor: they stay sorted by reduce
    edge); with `intm` (a slice): only those intermediate triplets and no quadruplet."""
    from gemnet_pytorch_amd.graph import GraphPlan
    d = {k: v for k, v in inputs.items() if k != "_plan"}
    if intm is not None:
        quads = slice(0, 0)
        for k in ("id4_reduce_intm_ca", "id4_reduce_intm_ab", "id4_expand_intm_db", "id4_expand_intm_ab"):
            d[k] = d[k][intm].contiguous()
    for k in ("id4_reduce_ca", "id4_expand_db", "id4_reduce_cab", "id4_expand_abd", "Kidx4"):
        d[k] = d[k][quads].contiguous()
    return GraphPlan(d, False).warm()


def _quad_geometry64(inputs, V, Vint, quads=slice(None)):
    """fp64 leaves V, Vint on the host and, for the quadruplets `quads`: uac, uab, ubd, the two angles, sin(a - b - d)."""
    ca, db = inputs["id4_reduce_ca"].cpu()[quads], inputs["id4_expand_db"].cpu()[quads]
    k = inputs["id4_expand_intm_ab"].cpu()[inputs["id4_expand_abd"].cpu()[quads]]
    V64, Vi64 = V.double().cpu().requires_grad_(True), Vint.double().cpu().requires_grad_(True)
    uac, uab, ubd = -V64[ca], -Vi64[k], -V64[db]
    phi, th = CK._quad_angles(uac, torch.zeros_like(uac), uab, uab + ubd)
    return V64, Vi64, phi, th, torch.sin(CK._angle_uv(-uab, ubd))


def _well_conditioned(phi, th, sin_abd):
    """The mask of test_gpu_kernels.test_quad_angles_geometry_fwd_bwd (sin of either angle > 0.05) and of a - b - d."""
    return ((torch.sin(phi) > 0.05) & (sin_abd > 0.05) & (torch.sin(th).abs() > 0.05)).detach()


def _check_rows(name, got, ref):
    """Bars of test_gpu_kernels.test_quad_basis_fused_fwd_bwd on the rows that receive a contribution."""
    got, hit = got.double().cpu(), ref.abs().sum(1) > 0
    assert hit.any() and torch.isfinite(got).all() and (got[~hit] == 0).all()
    # (scale: the median magnitude of the non-zero reference entries — bcc rows have exact zeros along the axes)
    err, scale = (got - ref).abs()[hit], float(ref.abs()[ref != 0].median())
    print(f"{name}: rows {int(hit.sum())}, median err {float(err.median()) / scale:.2e}, max {float(err.max()) / scale:.2e} "
          f"(x median |ref| = {scale:.3e})")
    assert float(err.median()) <= 2e-5 * scale and float(err.max()) <= 2e-3 * scale


@pytest.mark.parametrize("n_quad", [1, 63, 64, 65, None])
@pytest.mark.parametrize("angle_form", [False, True])
def test_quad_basis_on_vectors_fwd_and_reduced_adjoint(geometry, n_quad, angle_form, redzone):
    from gemnet_pytorch_amd import pbc
    inputs, V, Vint = geometry
    # the small counts start at the first well-conditioned quadruplet, so that a launch of ONE row has an adjoint to compare
    _, _, phi_all, th_all, sabd_all = _quad_geometry64(inputs, V, Vint)
    first = int(torch.nonzero(_well_conditioned(phi_all, th_all, sabd_all))[0])
    quads = slice(None) if n_quad is None else slice(first, first + n_quad)
    plan = _sub_plan(inputs, quads)
    nq = plan.quad.size
    assert nq == (n_quad or 5848)
    Vd, Vid = put(V.detach()).requires_grad_(True), put(Vint.detach()).requires_grad_(True)
    Y = pbc.quad_basis(Vd, Vid, plan, 7, angle_form=angle_form)
    V64, Vi64, phi, th, sin_abd = _quad_geometry64(inputs, V, Vint, quads)
    g = torch.Generator().manual_seed(5)
    # cotangents only on well-conditioned quadruplets, as test_gpu_kernels.test_quad_angles_geometry_fwd_bwd compares only those:
    # where c - a - b or a - b - d is nearly collinear the azimuth is the angle of a vanishing projection and its gradient ~ 1 / sin
    # is rounding noise in fp32 (the model's cotangent carries the matching factor sin there; a random one does not).  The EXACT
    # degeneracies have a test of their own below
    ok = _well_conditioned(phi, th, sin_abd).double()[:, None]
    assert float(ok.sum()) >= 1 and (float(ok[0]) == 1.0 if n_quad else 0.3 * nq <= float(ok.sum()) < nq)
    if angle_form:
        assert Y.shape == (nq, 4)
        ref = torch.stack([torch.sin(phi), torch.cos(phi), torch.sin(th), torch.cos(th)], dim=1)
        assert float((Y.double().cpu() - ref.detach()).abs().max()) <= 2e-5
        # cotangent in the bilinear kernels' convention: (dE/dPhi_cab, dE/dTheta_cabd, -, -)
        gY = torch.zeros(nq, 4, dtype=torch.float64)
        gY[:, :2] = torch.randn(nq, 2, generator=g, dtype=torch.float64) * ok
        loss = (gY[:, 0] * phi + gY[:, 1] * th).sum()
    else:
        assert Y.shape == (nq, 49)
        ref = B.real_sph_harm_full(7, phi, th)
        assert torch.allclose(Y.double().cpu(), ref.detach(), rtol=1e-4, atol=2e-5)
        gY = torch.randn(nq, 49, generator=g, dtype=torch.float64) * ok
        loss = (gY * ref).sum()
    rV, rVi = torch.autograd.grad(loss, (V64, Vi64))
    gV, gVi = torch.autograd.grad(Y, (Vd, Vid), put(gY.float()))
    _check_rows("dE/dV", gV, rV)
    _check_rows("dE/dVint", gVi, rVi)
    gV2, gVi2 = torch.autograd.grad(pbc.quad_basis(Vd, Vid, plan, 7, angle_form=angle_form), (Vd, Vid), put(gY.float()))
    assert torch.equal(gV, gV2) and torch.equal(gVi, gVi2)          # fixed order of addition


@pytest.mark.parametrize("angle_form", [False, True])
def test_exact_degeneracies_sit_on_the_clamp(geometry, angle_form, redzone):
    """The relative clamp decision of quad_math.h (kRel) on the rows the test above masks out.  EXACTLY planar quadruplets
    (c -> a and d -> b related by a lattice translation; polar angles fine): fp64 autograd sits on the reference's 1e-9 clamp —
    the azimuth's gradient is ~1e-9 — so the adjoint is the polar part alone, and the kernels must give the same within the usual
    bars (with the absolute clamp fp32 picks a side of the kink: an O(1) difference).  EXACTLY collinear quadruplets (a - b <- d
    or c - a - b through an atom's own images): the azimuth is the reference's atan2(1e-9, 0), (sin, cos) = (1, 0) exactly, and an
    azimuth cotangent alone gives exact zeros (fp64 autograd differentiates atan2(1e-9, x ~ 1e-17) there: no reference)."""
    from gemnet_pytorch_amd import pbc
    inputs, V, Vint = geometry
    _, _, phi, th, sin_abd = _quad_geometry64(inputs, V, Vint)
    sphi, sth = torch.sin(phi).detach(), torch.sin(th).abs().detach()
    # (on the clamp in fp64 as well: |p1 x p2| below 1e-9 there.  A planar pair whose vectors round differently leaves ~1e-7 in
    #  fp64 too, where autograd then picks a side of the kink: no reference)
    ca, db = inputs["id4_reduce_ca"].cpu(), inputs["id4_expand_db"].cpu()
    k = inputs["id4_expand_intm_ab"].cpu()[inputs["id4_expand_abd"].cpu()]
    uac, uab, ubd = -V.double().cpu()[ca], -Vint.double().cpu()[k], -V.double().cpu()[db]
    rej = lambda x, n: x - ((x * n).sum(1) / (n * n).sum(1))[:, None] * n      # noqa: E731
    y = torch.linalg.cross(rej(uac, uab), rej(ubd, -uab), dim=-1).norm(dim=-1)
    planar = torch.nonzero((y < 1e-10) & (sth < 2e-9) & (sphi > 0.05) & (sin_abd.detach() > 0.05))[:, 0]
    collinear = torch.nonzero((sphi < 1e-6) | (sin_abd.detach() < 1e-6))[:, 0]
    print("planar", len(planar), "collinear", len(collinear))
    assert len(planar) > 50 and len(collinear) > 300
    g = torch.Generator().manual_seed(9)
    # planar
    plan = _sub_plan(inputs, planar.to(DEV))
    nq = plan.quad.size
    Vd, Vid = put(V.detach()).requires_grad_(True), put(Vint.detach()).requires_grad_(True)
    Y = pbc.quad_basis(Vd, Vid, plan, 7, angle_form=angle_form)
    V64, Vi64, phi, th, _ = _quad_geometry64(inputs, V, Vint, planar)
    if angle_form:
        gY = torch.zeros(nq, 4, dtype=torch.float64)
        gY[:, :2] = torch.randn(nq, 2, generator=g, dtype=torch.float64)
        loss = (gY[:, 0] * phi + gY[:, 1] * th).sum()
    else:
        gY = torch.randn(nq, 49, generator=g, dtype=torch.float64)
        loss = (gY * B.real_sph_harm_full(7, phi, th)).sum()
    rV, rVi = torch.autograd.grad(loss, (V64, Vi64))
    gV, gVi = torch.autograd.grad(Y, (Vd, Vid), put(gY.float()))
    _check_rows("planar dE/dV", gV, rV)
    _check_rows("planar dE/dVint", gVi, rVi)
    # collinear
    plan = _sub_plan(inputs, collinear.to(DEV))
    nq = plan.quad.size
    Vd, Vid = put(V.detach()).requires_grad_(True), put(Vint.detach()).requires_grad_(True)
    ang = pbc.quad_basis(Vd, Vid, plan, 7, angle_form=True)
    assert (ang[:, 2] == 1.0).all() and (ang[:, 3] == 0.0).all()
    g_th = torch.zeros(nq, 4, device=DEV)
    g_th[:, 1] = torch.randn(nq, generator=g).to(DEV)
    gV, gVi = torch.autograd.grad(ang, (Vd, Vid), g_th)
    assert (gV == 0).all() and (gVi == 0).all()


@pytest.mark.parametrize("n_intm", [1, 63, 64, 65, None])
def test_intermediate_triplet_angles_on_vectors(geometry, n_intm, redzone):
    from gemnet_pytorch_amd import pbc
    inputs, V, Vint = geometry
    iab, idb = inputs["id4_expand_intm_ab"].cpu(), inputs["id4_expand_intm_db"].cpu()
    # the small counts start at the first triplet that is not collinear (the first ones are an atom and its own images: on the
    # clamp, gradients of 1e-10 — test_trip_basis_fused_fwd_bwd_including_collinear leaves that row out of its comparison too)
    sin_abd = torch.sin(CK._angle_uv(Vint.double().cpu()[iab], -V.double().cpu()[idb]))
    first = int(torch.nonzero(sin_abd > 0.05)[0])
    rows = slice(None) if n_intm is None else slice(first, first + n_intm)
    plan = _sub_plan(inputs) if n_intm is None else _sub_plan(inputs, intm=rows)
    T = plan.n_intm
    assert T == (n_intm or len(idb)) and T == plan.intm_ab.size
    iab, idb = iab[rows], idb[rows]
    Vd, Vid = put(V.detach()).requires_grad_(True), put(Vint.detach()).requires_grad_(True)
    Y = pbc.trip_basis2(Vid, Vd, plan, 7)
    V64, Vi64 = V.double().cpu().requires_grad_(True), Vint.double().cpu().requires_grad_(True)
    ref = B.real_sph_harm_l0(7, CK._angle_uv(Vi64[iab], -V64[idb]))
    assert Y.shape == ref.shape == (T, 7) and float((Y.double().cpu() - ref.detach()).abs().max()) <= 2e-5
    gY = torch.randn(ref.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    rV, rVi = torch.autograd.grad((gY * ref).sum(), (V64, Vi64))
    gVi, gV = torch.autograd.grad(Y, (Vid, Vd), put(gY.float()))
    # bars of test_trip_basis_fused_fwd_bwd_including_collinear (2e-3 relative + 2e-3 of the median magnitude of the rows that
    # receive a contribution), per row sum; rows without a triplet are exact zeros
    for name, got, want in (("dE/dV", gV, rV), ("dE/dVint", gVi, rVi)):
        got, hit = got.double().cpu(), want.abs().sum(1) > 0
        assert hit.any() and torch.isfinite(got).all() and (got[~hit] == 0).all()
        err, med = (got - want).abs(), float(want.abs()[want != 0].median())
        print(name, "rows", int(hit.sum()), float(err.max()), med)
        assert (err <= 2e-3 * want.abs() + 2e-3 * med).all()


def test_radial_basis_of_the_interaction_edges(geometry, redzone):
    from gemnet_pytorch_amd import pbc
    inputs, V, Vint = geometry
    z, nrm = torch.tensor(B.jn_zeros(7, 6)), torch.tensor(B.sph_bessel_normalizer(7, 6))
    Vid = put(Vint.detach()).requires_grad_(True)
    rad = pbc.radial_basis(Vid, put(z.float()), put(nrm), Q.INT_CUTOFF, 5)
    Vi64 = Vint.double().cpu().requires_grad_(True)
    ref = B.sph_bessel_radial(Vi64.norm(dim=1), 7, 6, Q.INT_CUTOFF, 5)
    assert torch.allclose(rad.double().cpu(), ref.detach(), rtol=1e-4, atol=2e-5)
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    (rW,) = torch.autograd.grad((g * ref).sum(), Vi64)
    (W,) = torch.autograd.grad(rad, Vid, put(g.float()))
    assert torch.allclose(W.double().cpu(), rW, rtol=2e-4, atol=2e-4 * float(rW.abs().max()))


# ------------------------------------------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "pbc_q_cases.npz")))


@pytest.fixture(scope="module")
def models():
    from gemnet_pytorch_amd.model.gemnet import GemNet
    out = {}
    for tag, cfg in Q.CFGS.items():
        params = Q.make_params(cfg)
        m = GemNet(**cfg, scale_file=SCALE_FILE)
        m.load_state_dict(GO.expand_to_reference_state_dict({k: v.float() for k, v in params.items()}))
        m.periodic_quadruplets = True
        out[tag] = m.to(DEV).eval()
    return out


def _run(model, structs):
    E, F, S = model(_batch(structs), stress=True)
    torch.cuda.synchronize()
    return E.double().cpu().numpy(), F.double().cpu().numpy(), S.double().cpu().numpy()


@pytest.mark.parametrize("tag,kind", [(t, k) for t, kinds in Q.GOLDEN_CASES.items() for k in kinds])
def test_energy_forces_stress_match_cluster_oracle(models, golden, tag, kind):
    """Bars of test_gpu_pbc.test_energy_forces_stress_match_cluster_oracle.
    Measured on an MI355X (|dE|, mean / max |dF|, max |dS|): q-small 9e-8, 2e-7 / 4e-7, 2e-8; q-triclinic 1e-7, 4e-7 / 7e-7, 2e-8;
    q-slab 1e-7, 6e-8 / 2e-7, 2e-9; q-bcc_pert 8e-8, 7e-7 / 3e-6, 4e-7; ang-small 2e-7, 3e-7 / 5e-7, 1e-8; ang-triclinic 6e-8,
    7e-7 / 2e-6, 2e-8; q-thin 1.9e-5 (E = 19.7), 2e-6 / 4e-6, 8e-6 (|S| = 8.7).  'thin' and bcc_pert hold exactly collinear and
    exactly planar quadruplets: the kernels take the reference's clamp decision relative to the vectors;
    with the absolute 1e-9 clamp 'thin' forces were 2.5e-3 off."""
    E_ref, F_ref, S_ref = (golden[f"{tag}.{kind}.{k}"] for k in "EFS")
    E, F, S = _run(models[tag], [P.structure(kind)])
    scale = max(1.0, float(np.abs(F_ref).mean()))
    sS = max(np.abs(S_ref).max(), 1e-2)
    print(tag, kind, "E", E[0, 0], float(E_ref), "dE", abs(E[0, 0] - float(E_ref)), "dF mean / max", np.abs(F - F_ref).mean(),
          np.abs(F - F_ref).max(), "scale", scale, "dS", np.abs(S[0] - S_ref).max(), "asym", np.abs(S[0] - S[0].T).max(), "sS", sS)
    assert abs(E[0, 0] - float(E_ref)) <= 2e-5 * max(1.0, abs(float(E_ref)))
    assert np.abs(F - F_ref).mean() <= 1e-5 * scale and np.abs(F - F_ref).max() <= 1e-4 * scale
    assert np.abs(S[0] - S_ref).max() <= 1e-4 * sS
    assert np.abs(S[0] - S[0].T).max() <= 1e-5 * sS


def test_batch_of_structures_equals_single_runs(models):
    model = models["q"]
    structs = [P.structure(k, seed=i) for i, k in enumerate(["small", "thin", "slab"])]
    E, F, S = _run(model, structs)
    off = 0
    for b, s in enumerate(structs):
        e, f, st = _run(model, [s])
        n = len(s[0])
        assert abs(E[b, 0] - e[0, 0]) <= 1e-5 * max(1.0, abs(e[0, 0]))
        assert np.abs(F[off:off + n] - f).max() <= 1e-5 * max(1.0, np.abs(f).max())
        assert np.abs(S[b] - st[0]).max() <= 1e-5 * max(1e-2, np.abs(st).max())
        off += n


def test_invariances(models):
    """Tolerances of test_gpu_pbc.test_invariances.  The supercell is the case that needs the relative clamp of quad_math.h: 36
    of the 260 quadruplets of 'triclinic' are exactly planar, exact zeros in the primitive cell and rounding residues in the
    supercell, where the absolute clamp picked one side of the azimuth's kink per copy (forces 5e-3 off, E and S intact)."""
    model = models["q"]
    R, Z, cell, pbc = P.structure("triclinic")
    E, F, S = _run(model, [(R, Z, cell, pbc)])
    tolE, tolF, tolS = 2e-5 * max(1.0, abs(E[0, 0])), 5e-5 * max(1.0, np.abs(F).max()), 5e-5 * max(1e-2, np.abs(S).max())
    R2 = R.copy()
    R2[2] += cell[1] - cell[0]
    for Rx in (R2, R + np.array([0.41, -0.73, 1.3])):
        e, f, s = _run(model, [(Rx, Z, cell, pbc)])
        assert abs(e[0, 0] - E[0, 0]) <= tolE and np.abs(f - F).max() <= tolF and np.abs(s - S).max() <= tolS
    shifts = [np.array(n) @ cell for n in np.ndindex(2, 2, 2)]
    Rs = np.concatenate([R + t for t in shifts])
    e, f, s = _run(model, [(Rs, np.tile(Z, 8), 2 * cell, pbc)])
    assert abs(e[0, 0] - 8 * E[0, 0]) <= 8 * tolE
    assert np.abs(f - np.tile(F, (8, 1))).max() <= tolF
    assert np.abs(s - S).max() <= tolS
    assert np.abs(S[0] - S[0].T).max() <= tolS


def test_without_images_equals_the_molecular_model(models):
    from gemnet_pytorch_amd.index_device import build_indices_device
    model = models["q"]
    rs = np.random.RandomState(2)
    fff = (False, False, False)
    R, Z, cell, _ = P.f32_round(P._gas_structure(12, rs, fff, density=0.12))
    batch = _batch([(R, Z, cell, np.array(fff))])
    assert len(batch["id4_reduce_ca"]) > 100
    E1, F1, _ = model(batch, stress=True)
    mol = build_indices_device(batch["R"], np.array([12]), Q.CUTOFF, Q.INT_CUTOFF, False)
    E0, F0 = model(dict(R=batch["R"], Z=batch["Z"], N=batch["N"], **mol))
    torch.cuda.synchronize()
    assert (E0 - E1).abs().max().item() <= 1e-5 * max(1.0, E0.abs().max().item())
    assert (F0 - F1).abs().max().item() <= 1e-5 * max(1.0, F0.abs().max().item())


@pytest.mark.parametrize("structs", [P.isolated(1), [P.structure("triclinic_FFF")] + P.isolated(1)])
def test_empty_lists_run(models, structs):
    E, F, S = _run(models["q"], structs)
    assert np.isfinite(E).all() and np.isfinite(F).all() and np.isfinite(S).all()
    assert np.abs(F[-1]).max() == 0.0 and np.abs(S[-1]).max() == 0.0          # the isolated atom


# ----------------------------------------------------------------------------------------------------------------- capture
@pytest.mark.parametrize("tag", ["q", "ang"])
def test_force_graphs_replay_is_the_eager_call(models, tag):
    from gemnet_pytorch_amd.runtime import ForceGraphs
    model = models[tag]
    batch = _batch([P.structure(k, seed=i) for i, k in enumerate(["small", "triclinic"])])
    fg = ForceGraphs(model, [batch])
    g = torch.Generator(device=DEV).manual_seed(1)
    R2 = batch["R"] + 0.01 * torch.randn(batch["R"].shape, device=DEV, generator=g)
    cell2 = batch["cell"] @ (torch.eye(3, device=DEV) + 0.002 * torch.randn(3, 3, device=DEV, generator=g))
    fg.set_positions(0, R2)
    fg.set_cell(0, cell2)
    fg.replay()
    torch.cuda.synchronize()
    E, F = fg.energies_forces()
    S = fg.stress()
    ref = dict(batch, R=R2.clone(), cell=cell2.clone())
    ref.pop("_plan", None)
    E0, F0, S0 = model(ref, stress=True)
    torch.cuda.synchronize()
    assert torch.equal(E, E0) and torch.equal(F, F0) and torch.equal(S, S0)


def test_captured_step_has_no_unordered_conflict(models):
    """The captured periodic GemNet-Q step under the happens-before checker, as tests/test_gpu_hbcheck.py does for the
    molecular steps: no unordered conflicting accesses, every node and pointer accounted for; one replay equals the eager run."""
    from gemnet_pytorch_amd import hbcheck
    model = models["q"]
    batch = _batch([P.structure("small"), P.structure("thin")])
    E0, F0, S0 = (t.detach().clone() for t in model(batch, stress=True))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            model(batch, stress=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with hbcheck.record() as rec:
            Eg, Fg, Sg = model(batch, stress=True)
    races, summary = rec.races(), rec.summary()
    print(rec.format(races))
    assert not races
    assert summary["unrecorded_nodes"] == 0 and summary["unresolved_pointers"] == 0
    assert summary["nodes"] >= summary["ops"] > 50
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(Eg, E0) and torch.equal(Fg, F0) and torch.equal(Sg, S0)


# --------------------------------------------------------------------------------------------------------------- refusals
def test_out_of_scope_cases_raise(models):
    from gemnet_pytorch_amd.md import DeviceMolecule, predict_periodic
    from gemnet_pytorch_amd.model.gemnet import GemNet
    from gemnet_pytorch_amd.padded import PaddedGraphRunner
    from gemnet_pytorch_amd.runtime import DynamicForceField
    s = P.structure("small")
    batch = _batch([s])
    q = GemNet(**Q.CFG_Q, scale_file=SCALE_FILE).to(DEV).eval()
    with pytest.raises(NotImplementedError, match="GemNet-Q"):          # the default model still refuses
        q(dict(batch))
    model = models["q"]
    model(dict(batch))
    # training (with and without periodic_training), direct forces, several targets, positions in a graph
    model.train()
    try:
        for flag in (False, True):
            model.periodic_training = flag
            with pytest.raises(NotImplementedError, match="GemNet-Q"):
                model(dict(batch))
    finally:
        model.periodic_training = False
        model.eval()
    # every refusal of a quadruplet model names it, the ones it shares with GemNet-T included
    for kw, switches in ((dict(direct_forces=True), ("periodic_direct_forces",)), (dict(num_targets=2), ())):
        m = GemNet(**dict(Q.CFG_Q, **kw), scale_file=SCALE_FILE).to(DEV).eval()
        m.periodic_quadruplets = True
        for sw in switches:
            setattr(m, sw, True)
        with pytest.raises(NotImplementedError, match="GemNet-Q"):
            m(dict(batch))
    with pytest.raises(NotImplementedError, match=r"GemNet-Q.*autograd graph"):
        model(dict(batch, R=batch["R"].clone().requires_grad_(True)))
    from gemnet_pytorch_amd.model.scaling import AutomaticFit
    assert not AutomaticFit.fitting_mode
    AutomaticFit.fitting_mode = True
    try:
        with pytest.raises(NotImplementedError, match=r"GemNet-Q.*scale-factor fitting"):
            model(dict(batch))
    finally:
        AutomaticFit.fitting_mode = False
    with pytest.raises(ValueError, match="int_cell_offsets"):
        model({k: v for k, v in batch.items() if k not in ("int_cell_offsets", "_plan")})
    # the padded and in-graph runners
    R, Z, cell, pbc = s
    with pytest.raises(NotImplementedError, match="GemNet-Q"):
        DeviceMolecule(R, Z, Q.CUTOFF, Q.INT_CUTOFF, triplets_only=False, cell=cell, pbc=pbc)
    with pytest.raises(NotImplementedError, match="GemNet-Q"):
        DynamicForceField(model, batch["Z"], [3], Q.CUTOFF, Q.INT_CUTOFF, cell=cell[None], pbc=pbc)
    mol = DeviceMolecule(R, Z, Q.CUTOFF, Q.INT_CUTOFF, triplets_only=True, cell=cell, pbc=pbc)
    mol.to(DEV)
    with pytest.raises(NotImplementedError, match="GemNet-Q"):
        predict_periodic(model, mol.get())
    with pytest.raises(NotImplementedError, match="GemNet-Q"):
        PaddedGraphRunner(model, batch["Z"], batch["N"], 64, 64, max_in_degree=16, quad_caps=(64, 256, 1024), cell=batch["cell"],
                          pbc=pbc[None])


# ------------------------------------------------------------------------------------------------------------ narrow layers
@pytest.mark.parametrize("C,E,J,mk", [(8, 60, 300, 80), (16, 61, 130, 40), (8, 1, 5, 3)])
def test_tensor_basis_x_adjoint_at_narrow_widths(C, E, J, mk, redzone):
    """gn_bil_expand_f32 at S = 49 and C < 32 (the quadruplet x-adjoint of a narrow model, Y_lm rows): the launch takes at most 8
    edge groups per block — 32 groups of C = 8 asked for more LDS than a launch gets.  Bars of test_gpu_kernels.test_bilinear_kernels."""
    from gemnet_pytorch_amd import kernels as K
    from gemnet_pytorch_amd.graph import SegmentPlan
    g = torch.Generator().manual_seed(C * E)
    counts = torch.randint(1, 2 * mk, (E,), generator=g)
    red = torch.repeat_interleave(torch.arange(E), counts)
    exp = torch.randint(0, J, (red.shape[0],), generator=g)
    cpu, dev = SegmentPlan(red, exp, E, J), SegmentPlan(red.to(DEV), exp.to(DEV), E, J)
    Y = torch.randn(cpu.size, 49, generator=g, dtype=torch.float64)
    D = torch.randn(E, 49, C, generator=g, dtype=torch.float64)
    got = K.bil_reduce_t(put(Y.float()), put(D.float()), dev)
    ref = CK.bil_reduce_t(Y, D, cpu)
    assert got.shape == ref.shape and float((got.double().cpu() - ref).abs().max()) <= 1e-4 + 2e-5 * float(ref.abs().max())
