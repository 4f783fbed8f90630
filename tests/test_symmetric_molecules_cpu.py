"""The recipes of tests/symmetric_molecules.py, pinned, with the conditions that make them fixtures (no pair on a cutoff, the
same index lists in every orientation, a well-conditioned plane, an exactly covariant float64 reference); the record of WHY a
decision is needed (the float32 oracle, which keeps the reference's absolute clamp, misses the force bar by orders of magnitude
on GemNet-Q once a planar or linear molecule is rotated off the axes); and the float64 restatements of the molecular quadruplet
kernels (tests/cpu_kernels.py) with the relative decisions of csrc/quad_math.h held to duality, to float64 autograd of the
reference formulas, to the (1, 0) convention, and — through the GemNet module — to the reference."""
import numpy as np
import pytest
import torch

import cpu_kernels as CK
import molecule_zoo as MZ
import symmetric_molecules as SM

COUNTS = {
    "planar9": dict(atoms=9, edges=70, triplets=476, int_edges=72, intm_triplets=560, quadruplets=2856, collinear=0, abd_only=0),
    "linear5": dict(atoms=5, edges=20, triplets=60, int_edges=20, intm_triplets=80, quadruplets=120, collinear=120, abd_only=0),
    "benzene": dict(atoms=12, edges=132, triplets=1320, int_edges=132, intm_triplets=1452, quadruplets=11880, collinear=1224,
                    abd_only=576),
}
ROTATED = ("rot3", "rot11")


def _sin(u, v):
    return np.linalg.norm(np.cross(u, v), axis=1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1))


def _quad_sines(name):
    """sin(c - a - b), sin(a - b - d) of every quadruplet on the exact coordinates."""
    R = SM.coordinates(name)[0]
    qc, qa, qb, qd = (t.long().numpy() for t in SM.quad_atoms(SM.index_lists(name, "axis")))
    return _sin(R[qc] - R[qa], R[qb] - R[qa]), _sin(R[qa] - R[qb], R[qd] - R[qb])


# -------------------------------------------------------------------------------------------------- recipes and conditions
@pytest.mark.parametrize("name", SM.MOLECULES)
def test_recipe_counts_and_index_lists_in_every_orientation(name):
    R, Z = SM.coordinates(name)
    d = np.linalg.norm(R[:, None] - R[None], axis=-1)
    assert np.abs(d - MZ.CUTOFF).min() > 1e-4 and np.abs(d - MZ.INT_CUTOFF).min() > 1e-4       # no pair on a cutoff
    base = SM.index_lists(name, "axis")
    for o in ROTATED:
        idx = SM.index_lists(name, o)
        assert set(idx) == set(base) and all(np.array_equal(base[k], idx[k]) for k in base), o
        Q, _ = SM.rotation(o)
        assert abs(np.linalg.det(Q) - 1.0) < 1e-12 and np.abs(Q @ Q.T - np.eye(3)).max() < 1e-12 and np.abs(Q).min() > 0.01       # generic: no axis stays an axis
        Rp = SM.placed(name, o)
        assert np.array_equal(Rp, Rp.astype(np.float32).astype(np.float64))
        assert np.abs(Rp - (R @ Q.T + SM.SHIFT)).max() <= 2.0 ** -24 * np.abs(Rp).max()
    s_cab, s_abd = _quad_sines(name)
    facts = dict(atoms=len(Z), edges=len(base["id_a"]), triplets=len(base["id3_reduce_ca"]), int_edges=len(base["id4_int_a"]),
                 intm_triplets=len(base["id4_expand_intm_db"]), quadruplets=len(base["id4_reduce_ca"]),
                 collinear=int(((s_cab < 1e-6) | (s_abd < 1e-6)).sum()), abd_only=int(((s_abd < 1e-6) & (s_cab > 1e-6)).sum()))
    assert facts == COUNTS[name]


def test_recipe_details():
    R, Z = SM.coordinates("planar9")
    assert SM.PLANAR_SEED == 550 and Z.tolist() == [6, 1, 8, 6, 1, 1, 8, 6, 1] and not R[:, 2].any()
    assert 0 <= R[:, :2].min() and R[:, :2].max() <= 4.5
    d = np.linalg.norm(R[:, None] - R[None], axis=-1) + 10 * np.eye(9)
    assert d.min() >= 0.95
    R, Z = SM.coordinates("linear5")
    assert R[:, 0].tolist() == [0, 1.16, 2.32, 3.4, 4.6] and not R[:, 1:].any() and Z.tolist() == [8, 6, 8, 6, 1]
    R, Z = SM.coordinates("benzene")
    assert not R[:, 2].any() and np.array_equal(R[:3], -R[3:6]) and np.array_equal(R[6:9], -R[9:])       # para atoms
    assert np.allclose(np.linalg.norm(R[:6], axis=1), 1.39, atol=1e-15) and np.allclose(np.linalg.norm(R[6:], axis=1), 2.48, atol=1e-15)
    assert np.allclose(np.linalg.norm(R[:6] - np.roll(R[:6], 1, axis=0), axis=1), 1.39, atol=1e-15)
    Q3, s = SM.rotation("rot3")
    assert s.tolist() == [0.3, -1.2, 2.1] and not np.allclose(Q3, SM.rotation("rot11")[0])
    assert np.array_equal(SM.rotation("axis")[0], np.eye(3)) and not SM.rotation("axis")[1].any()


def test_the_plane_is_well_conditioned():
    """No triplet c - a - b or a - b - d of a planar9 quadruplet (nor any of its model triplets) below sin = 0.05: the planar
    rows are then well conditioned and the elementwise bars of the kernel tests apply to all of them without a mask."""
    s_cab, s_abd = _quad_sines("planar9")
    R = SM.coordinates("planar9")[0]
    tc, ta, tb = (t.long().numpy() for t in SM.trip_atoms(SM.index_lists("planar9", "axis")))
    print("planar9: min sin", float(s_cab.min()), float(s_abd.min()), float(_sin(R[tc] - R[ta], R[tb] - R[ta]).min()))
    assert s_cab.min() >= 0.05 and s_abd.min() >= 0.05 and _sin(R[tc] - R[ta], R[tb] - R[ta]).min() >= 0.05


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_the_reference_is_covariant_and_of_order_one(kind):
    for name in SM.MOLECULES:
        E, F = SM.axis_reference(name, kind)
        for o in ROTATED:        # float64 on the unrounded rotated coordinates: the same energy
            E2, _ = SM.run_oracle(name, o, kind, rounded=False)
            assert np.abs(E2 - E).max() < 1e-9, (name, o)
        if name == "benzene" and kind == "Q":
            assert SM.reference(name, "rot3", kind)[1] is None
            continue
        assert np.abs(F[:, 2]).max() < 1e-12                          # planar: no out-of-plane force ...
        if name == "linear5":
            assert np.abs(F[:, 1:]).max() < 1e-12                     # ... linear: none off the line
        assert np.abs(F.sum(0)).max() < 1e-9
        assert 0.3 <= float(np.abs(F).mean()) <= 2.5, (name, float(np.abs(F).mean()))
    fm = float(np.abs(SM.axis_reference("planar9", kind)[1]).mean())
    assert 0.3 <= fm <= 1.6, fm                                        # the bars on planar9 are literal, as on the zoo batch


# ------------------------------------------------------------------------------------- the record: why a decision is needed
@pytest.mark.parametrize("name", ["planar9", "linear5"])
def test_float32_oracle_with_the_absolute_clamp_misses_the_force_bar_on_gemnet_q(name):
    """The float32 oracle states the reference's arithmetic: max(|u x v|, 1e-9) against residues of 1e-7.  Axis-aligned it holds
    the bars; rotated it misses FORCE_TOL by at least 1e3 (docs/SYMMETRIC_MOLECULES.md records the figures)."""
    _, Fr = SM.reference(name, "axis", "Q")
    _, F = SM.run_oracle(name, "axis", "Q", dtype=torch.float32)
    mae = float(np.abs(F - Fr).mean())
    print(f"float32 oracle Q {name}/axis: force MAE {mae:.3e} at mean|F| {np.abs(Fr).mean():.3f}")
    assert mae <= MZ.FORCE_TOL * max(1.0, float(np.abs(Fr).mean()))
    E, Fr = SM.reference(name, "rot3", "Q")
    E32, F = SM.run_oracle(name, "rot3", "Q", dtype=torch.float32)
    mae = float(np.abs(F - Fr).mean())
    print(f"float32 oracle Q {name}/rot3: force MAE {mae:.3e} at mean|F| {np.abs(Fr).mean():.3f}; energy err {np.abs(E32 - E).max():.2e}")
    assert mae >= 1e3 * MZ.FORCE_TOL


def test_float32_oracle_energy_of_benzene_is_off_in_every_orientation_on_gemnet_q():
    E = SM.reference("benzene", "axis", "Q")[0]
    for o in SM.ORIENTATIONS:
        E32, _ = SM.run_oracle("benzene", o, "Q", dtype=torch.float32)
        print(f"float32 oracle Q benzene/{o}: E {float(E32[0, 0]):.4f} against {float(E[0, 0]):.6f}")
        assert np.abs(E32 - E).max() > 1e3 * MZ.ENERGY_TOL * max(1.0, float(np.abs(E).max()))


def test_float32_oracle_holds_every_bar_on_gemnet_t():
    for name in SM.MOLECULES:
        for o in ROTATED:
            E, F = SM.run_oracle(name, o, "T", dtype=torch.float32)
            SM.assert_force_energy(SM.force_energy_figures(E, F, name, o, "T"), f"float32 oracle T {name}/{o}")
    ref = SM.training_reference("T")
    got = SM.run_training_oracle("T", "rot3", dtype=torch.float32, rounded=True)
    worst, pname, rel = MZ.grad_figures(got["grads"], ref)
    print(f"float32 oracle T planar9 + linear5 / rot3: loss {got['loss']:.6f} (float64 {ref['loss']:.6f}); worst gradient error "
          f"{worst:.3f} of its bar ({pname}), {rel:.2e} relative")
    assert abs(got["loss"] - ref["loss"]) <= MZ.LOSS_RTOL * abs(ref["loss"]) and worst <= 1.0


def test_float32_oracle_training_on_gemnet_q_is_off_when_rotated():
    ref = SM.training_reference("Q")
    got = SM.run_training_oracle("Q", "rot3", dtype=torch.float32, rounded=True)
    worst, pname, rel = MZ.grad_figures(got["grads"], ref)
    print(f"float32 oracle Q planar9 + linear5 / rot3: loss {got['loss']:.6f} (float64 {ref['loss']:.6f}); worst gradient error "
          f"{worst:.1f} of its bar ({pname}), {rel:.2e} relative")
    assert worst > 10.0


# ------------------------------------------------------------- the float64 restatements of the molecular quadruplet kernels
def _geometry(name, orient):
    """R (float64, what the model receives), the quadruplet atoms and the decision masks on the exact coordinates."""
    R = torch.tensor(SM.placed(name, orient))
    q = SM.quad_atoms(SM.index_lists(name, orient))
    s_cab, s_abd = _quad_sines(name)
    return R, q, torch.tensor(s_cab < 1e-6), torch.tensor((s_cab < 1e-6) | (s_abd < 1e-6))


def _atoms(Gc, Gb, Gd, q, n):
    """Per-quadruplet terms (c, b, d; a: minus their sum) -> atoms."""
    qc, qa, qb, qd = (t.long() for t in q)
    return (torch.zeros(n, 3, dtype=Gc.dtype).index_add(0, qc, Gc).index_add(0, qb, Gb).index_add(0, qd, Gd)
            .index_add(0, qa, -(Gc + Gb + Gd)))


@pytest.mark.parametrize("orient", SM.ORIENTATIONS)
@pytest.mark.parametrize("name", SM.MOLECULES)
def test_adjoint_and_tangent_are_dual(name, orient):
    """sum_q g_ang . tang == <G, tR> to 1e-12: both take the same decisions, so the second-order pass differentiates exactly
    the function whose first adjoint gives the forces."""
    R, q, _, _ = _geometry(name, orient)
    g = torch.Generator().manual_seed(17)
    g_ang = torch.zeros(len(q[0]), 4, dtype=torch.float64)
    g_ang[:, :2] = torch.randn(len(q[0]), 2, generator=g, dtype=torch.float64)
    tR = torch.randn(R.shape, generator=g, dtype=torch.float64)
    G = _atoms(*CK.quad_angles_bwd(g_ang, R, *q), q, len(R))
    tang = CK.quad_angles_jvp(R, tR, *q)
    lhs, rhs = float((g_ang * tang).sum()), float((G * tR).sum())
    print(f"{name}/{orient}: sum g.tang {lhs:.12e}, <G, tR> {rhs:.12e}")
    assert torch.isfinite(G).all() and torch.isfinite(tang).all() and not tang[:, 2:].any()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, float((g_ang[:, :2] * tang[:, :2]).abs().sum()))
    Gc, Gbd = CK.quad_angles_bwd(g_ang, R, *q, packed=True)
    assert not Gbd[:, 3].any() and not Gbd[:, 7].any()


def _elementwise(name, got, ref):
    """The bars of test_gpu_kernels.test_quad_angles_geometry_fwd_bwd, on ALL rows."""
    err = (got - ref).abs() / ref.abs().clamp(min=1.0)
    print(f"{name}: median {float(err.median()):.2e}, max {float(err.max()):.2e} of max(1, |ref|)")
    assert torch.isfinite(got).all() and float(err.median()) <= 1e-5 and float(err.max()) <= 5e-3


@pytest.mark.parametrize("orient", SM.ORIENTATIONS)
def test_planar_adjoint_is_float64_autograd_of_the_reference_formulas(orient):
    """planar9, every row: the restated kernels on the coordinates the model receives (rotated, rounded through float32: the
    planar residue is 1e-7 there, far above 1e-9) against autograd of the REFERENCE's formulas on the exact axis-aligned
    coordinates (where the azimuth sits on the reference's own clamp), carried over by the rotation."""
    R, q, _, _ = _geometry("planar9", orient)
    Q = torch.tensor(SM.rotation(orient)[0])
    Rx = torch.tensor(SM.coordinates("planar9")[0])
    nq = len(q[0])
    g = torch.Generator().manual_seed(23)
    g_ang = torch.zeros(nq, 4, dtype=torch.float64)
    g_ang[:, :2] = torch.randn(nq, 2, generator=g, dtype=torch.float64)
    gY = torch.randn(nq, 49, generator=g, dtype=torch.float64)
    tR = torch.randn(R.shape, generator=g, dtype=torch.float64)
    idx = [t.long() for t in q]
    with torch.enable_grad():
        leaves = [Rx[i].clone().requires_grad_(True) for i in (idx[0], idx[2], idx[3])]
        phi, th = CK._quad_angles(leaves[0], Rx[idx[1]], leaves[1], leaves[2])
        ref_ang = torch.autograd.grad((g_ang[:, 0] * phi + g_ang[:, 1] * th).sum(), leaves, retain_graph=True)
        ref_Y = torch.autograd.grad((gY * CK.B.real_sph_harm_full(7, phi, th)).sum(), leaves)
    # the plane: the azimuth is 0 or pi on every row
    ang = CK.quad_angles_fwd(R, *q)
    assert float(ang[:, 2].abs().max()) <= 1e-5 and float((ang[:, 3].abs() - 1).abs().max()) <= 1e-10
    ref4 = torch.stack([torch.sin(phi), torch.cos(phi), torch.sin(th), torch.cos(th)], 1).detach()
    assert float((ang - ref4).abs().max()) <= 2e-5
    for n_, got, ref in zip("cbd", CK.quad_angles_bwd(g_ang, R, *q), ref_ang):
        _elementwise(f"planar9/{orient} quad_angles_bwd G{n_}", got, ref @ Q.T)
    for n_, got, ref in zip("cbd", CK.quad_basis_bwd(gY, R, *q, 7), ref_Y):
        _elementwise(f"planar9/{orient} quad_basis_bwd G{n_}", got, ref @ Q.T)
    Gc, Gbd = CK.quad_basis_bwd_packed(gY, R, *q, 7)
    assert torch.equal(Gbd[:, 0:3], CK.quad_basis_bwd(gY, R, *q, 7)[1])
    Y = CK.quad_basis_fwd(R, *q, 7)
    assert float((Y - CK.B.real_sph_harm_full(7, phi, th).detach()).abs().max()) <= 2e-5
    # tangent: along the rotated tangent the angles move as they do in the axis frame
    ref_t = CK._jvp(lambda X: torch.stack(CK._quad_angles(X[idx[0]], X[idx[1]], X[idx[2]], X[idx[3]]), 1), Rx, tR @ Q)
    _elementwise(f"planar9/{orient} quad_angles_jvp", CK.quad_angles_jvp(R, tR, *q)[:, :2], ref_t)


@pytest.mark.parametrize("orient", SM.ORIENTATIONS)
@pytest.mark.parametrize("name", ["linear5", "benzene"])
def test_collinear_rows_carry_the_convention(name, orient):
    """Where a rejection has vanished the azimuth is the reference's atan2(1e-9, 0): (sin, cos) = (1, 0) EXACTLY, an
    azimuth-only cotangent gives exact zeros and a position tangent a zero azimuth tangent; where c - a - b itself is collinear
    the polar angle is a constant as well."""
    R, q, flat, vanished = _geometry(name, orient)
    assert int(vanished.sum()) == COUNTS[name]["collinear"] and int((vanished & ~flat).sum()) == COUNTS[name]["abd_only"]
    ang = CK.quad_angles_fwd(R, *q)
    assert (ang[vanished, 2] == 1.0).all() and (ang[vanished, 3] == 0.0).all()
    assert float(ang[flat, 0].abs().max()) <= 1e-6
    g = torch.Generator().manual_seed(29)
    g_th = torch.zeros(len(vanished), 4, dtype=torch.float64)
    g_th[:, 1] = torch.randn(len(vanished), generator=g, dtype=torch.float64) * vanished
    for G in CK.quad_angles_bwd(g_th, R, *q):
        assert not G.any()
    g_phi = torch.zeros_like(g_th)
    g_phi[:, 0] = torch.randn(len(vanished), generator=g, dtype=torch.float64) * flat
    for G in CK.quad_angles_bwd(g_phi, R, *q):
        assert not G.any()
    tang = CK.quad_angles_jvp(R, torch.randn(R.shape, generator=g, dtype=torch.float64), *q)
    assert not tang[vanished, 1].any() and not tang[flat, 0].any()
    Y = CK.quad_basis_fwd(R, *q, 7)
    half_pi = torch.full((int(vanished.sum()),), np.pi / 2, dtype=torch.float64)
    want = CK.B.real_sph_harm_full(7, torch.atan2(ang[vanished, 0], ang[vanished, 1]), half_pi)
    assert float((Y[vanished] - want).abs().max()) <= 1e-12


# --------------------------------------------------------------------------------------------------- the module's wiring
@pytest.mark.parametrize("kind", ["T", "Q"])
def test_module_wiring_on_the_symmetric_molecules(kind):
    """The GemNet module above the C ABI (launchers emulated in float64) in eval mode.  On the unrounded rot3 coordinates: the
    reference at 1e-7, as the other wiring tests.  On the coordinates the model receives (rounded through float32) float64
    with the reference's absolute clamp has a force MAE of 0.7; with the decisions it holds the GPU's bars."""
    from test_model_cpu import build
    cfg, P = SM.params(kind)
    with CK.emulate():
        model = build(cfg, P).eval()
        for name in SM.MOLECULES:
            E, F = model(SM.inputs_of([name], "rot3", kind, rounded=False))
            E, F = E.detach().numpy(), F.detach().numpy()
            Er, Fr = SM.reference(name, "rot3", kind)
            assert np.abs(E - Er).max() <= 1e-7 * max(1.0, float(np.abs(Er).max())), name
            if Fr is not None:
                assert np.abs(F - Fr).max() <= 1e-7 * max(1.0, float(np.abs(Fr).max())), (name, float(np.abs(F - Fr).max()))
            for o in ROTATED:
                E, F = model(SM.inputs_of([name], o, kind))
                E, F = E.detach().numpy(), F.detach().numpy()
                SM.assert_force_energy(SM.force_energy_figures(E, F, name, o, kind), f"emulated {kind} {name}/{o}")
                if name == "benzene":
                    out = np.abs((F @ SM.rotation(o)[0])[:, 2]).max()
                    print(f"emulated {kind} benzene/{o}: out-of-plane force {out:.2e}, mean|F| {np.abs(F).mean():.3f}")
                    assert out <= MZ.FORCE_MAX_TOL * max(1.0, float(np.abs(F).mean()))


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_module_wiring_training_gradients(kind):
    """Training mode (twice-differentiable kernels: value, adjoint, tangent) on planar9 + linear5 / rot3 as the model receives
    them: loss and every parameter gradient at the GPU's bars."""
    from oracle import gemnet_oracle as GO
    from test_model_cpu import build
    cfg, P = SM.params(kind)
    ref = SM.training_reference(kind)
    with CK.emulate():
        model = build(cfg, P).train()
        E, F = model(SM.inputs_of(SM.TRAIN, "rot3", kind))
        loss = GO.training_loss(E[:, :1], F, *SM.train_targets("rot3"))
        loss.backward()
    worst, pname, rel = MZ.grad_figures({k: v.grad for k, v in model.named_parameters()}, ref)
    print(f"emulated {kind} training: loss {loss.item():.9f} (reference {ref['loss']:.9f}); worst gradient error {worst:.3f} of its "
          f"bar ({pname}), {rel:.2e} relative")
    assert abs(loss.item() - ref["loss"]) <= MZ.LOSS_RTOL * abs(ref["loss"]) and worst <= 1.0


@pytest.mark.parametrize("orient", SM.ORIENTATIONS)
def test_collinear_triplets_pass_no_gradient_through_the_cross_product(orient):
    """The restated triplet kernels on linear5 as the model receives it: float64 with the reference's absolute clamp
    differentiates the 1e-7 residue (a unit gradient in a direction that is rounding noise); with the relative decision only the
    d/dx term is left, as on the exact axis-aligned coordinates."""
    R = torch.tensor(SM.placed("linear5", orient))
    t = SM.trip_atoms(SM.index_lists("linear5", orient))
    g = torch.randn(len(t[0]), generator=torch.Generator().manual_seed(31), dtype=torch.float64)
    Ra = R[t[1].long()]
    u, v = (R[t[0].long()] - Ra).requires_grad_(True), (R[t[2].long()] - Ra).requires_grad_(True)
    plain = torch.autograd.grad(CK._angle_uv(u, v), (u, v), g)
    got = CK.angle_bwd(g, R, *t)
    tR = torch.randn(R.shape, generator=torch.Generator().manual_seed(32), dtype=torch.float64)
    thd, Hc, Hb = CK.angle_jvp(R, tR, g, *t)
    print(f"linear5/{orient}: max |G| {max(float(x.abs().max()) for x in got):.2e} (absolute clamp: "
          f"{max(float(x.abs().max()) for x in plain):.2e}), theta tangent {float(thd.abs().max()):.2e}")
    assert max(float(x.abs().max()) for x in got) <= 1e-6 and float(thd.abs().max()) <= 1e-6
    assert torch.isfinite(Hc).all() and torch.isfinite(Hb).all()
    if orient != "axis":
        assert max(float(x.abs().max()) for x in plain) > 0.1
    Gc, Gb = CK.trip_basis_bwd(torch.randn(len(t[0]), 7, generator=torch.Generator().manual_seed(33), dtype=torch.float64), R, *t)
    assert max(float(Gc.abs().max()), float(Gb.abs().max())) <= 1e-6
