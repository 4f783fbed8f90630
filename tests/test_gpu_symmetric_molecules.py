"""-m gpu: exactly planar and exactly linear molecules in general orientation (tests/symmetric_molecules.py) on the HIP path
against the float64 oracle of the exact axis-aligned coordinates, carried over by the rotation.

Kernel level: the quadruplet and triplet geometry kernels on the molecules' own index lists, ALL rows (no mask: the plane is
well conditioned by construction, and the degenerate rows are what the file is about).  Model level: the published widths with
2 blocks, GemNet-T and GemNet-Q, at the bars of molecule_zoo.  Every test runs under the red-zone harness and prints its figures
before it asserts; docs/SYMMETRIC_MOLECULES.md records them."""
import numpy as np
import pytest
import torch

import cpu_kernels as CK
import molecule_zoo as MZ
import symmetric_molecules as SM
from gemnet_pytorch_amd import kernels as K
from oracle import gemnet_oracle as GO
from redzone import put, redzone  # noqa: F401  (autouse: every test of this module runs under the red-zone harness)
from test_gpu_model import build

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROTATED = ("rot3", "rot11")


def f32(t):
    return put(t.float().contiguous())


def _rot(orient):
    return torch.tensor(SM.rotation(orient)[0])


def _quads(name):
    return SM.quad_atoms(SM.index_lists(name, "axis"))          # (the same lists in every orientation: pinned on the CPU)


def _trips(name):
    return SM.trip_atoms(SM.index_lists(name, "axis"))


def _R(name, orient):
    """What the kernel receives (float32 values, held in float64)."""
    return torch.tensor(SM.placed(name, orient))


def _exact(name):
    return torch.tensor(SM.coordinates(name)[0])


def _masks(name, q):
    """On the exact coordinates: flat (c - a - b collinear), vanished (a rejection has vanished)."""
    R = _exact(name)
    c, a, b, d = (R[i.long()] for i in q)
    flat, vanished, _ = CK.quad_decisions(c - a, b - a, d - b)
    return flat, vanished


def _elementwise(tag, got, ref):
    """The bars of test_gpu_kernels.test_quad_angles_geometry_fwd_bwd, on ALL rows."""
    got = got.double().cpu()
    err = (got - ref).abs() / ref.abs().clamp(min=1.0)
    print(f"{tag}: median {float(err.median()):.2e}, max {float(err.max()):.2e} of max(1, |ref|) over {tuple(ref.shape)}")
    assert torch.isfinite(got).all(), tag
    assert float(err.median()) <= 1e-5 and float(err.max()) <= 5e-3, tag


def _dev(idx):
    return [put(i) for i in idx]


# ================================================================================================= quadruplet kernels
@pytest.mark.parametrize("orient", SM.ORIENTATIONS)
@pytest.mark.parametrize("name", SM.MOLECULES)
def test_quad_angles_fwd_on_all_rows(name, orient):
    q = _quads(name)
    R = _R(name, orient)
    ref = CK.quad_angles_fwd(R, *q)
    ang = K.quad_angles_fwd(f32(R), *_dev(q)).double().cpu()
    _, vanished = _masks(name, q)
    err = (ang - ref).abs()
    print(f"{name}/{orient}: quad_angles_fwd max err {float(err.max()):.2e} over {len(ref)} rows, {int(vanished.sum())} convention rows")
    assert torch.isfinite(ang).all() and float(err.max()) <= 2e-5
    assert (ang[vanished, 2] == 1.0).all() and (ang[vanished, 3] == 0.0).all()
    if orient != "axis":       # ... and equal to the axis output: the angles are scalars
        ax = K.quad_angles_fwd(f32(_R(name, "axis")), *_dev(q)).double().cpu()
        print(f"{name}/{orient}: against the axis output {float((ang - ax).abs().max()):.2e}")
        assert float((ang - ax).abs().max()) <= 2e-5


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65])
def test_quad_angles_fwd_and_bwd_on_cut_lists(n_rows):
    """benzene/rot3 cut to its first rows (row 0 is a planar row, row 11 the first collinear one)."""
    q = [i[:n_rows].contiguous() for i in _quads("benzene")]
    R = _R("benzene", "rot3")
    ang = K.quad_angles_fwd(f32(R), *_dev(q)).double().cpu()
    assert ang.shape == (n_rows, 4) and float((ang - CK.quad_angles_fwd(R, *q)).abs().max()) <= 2e-5
    g_ang = torch.zeros(n_rows, 4, dtype=torch.float64)
    g_ang[:, :2] = torch.randn(n_rows, 2, generator=torch.Generator().manual_seed(n_rows), dtype=torch.float64)
    ref = CK.quad_angles_bwd(g_ang, R, *q)
    got = K.quad_angles_bwd(f32(g_ang), f32(R), *_dev(q))
    for n_, a, b in zip("cbd", got, ref):
        _elementwise(f"benzene/rot3 first {n_rows}: G{n_}", a, b)
    Gc, Gbd = K.quad_angles_bwd(f32(g_ang), f32(R), *_dev(q), packed=True)
    assert torch.equal(Gc, got[0]) and torch.equal(Gbd[:, 0:3], got[1]) and torch.equal(Gbd[:, 4:7], got[2])
    assert not Gbd[:, 3].any() and not Gbd[:, 7].any()


@pytest.fixture(scope="module")
def planar_reference():
    """float64 autograd of the REFERENCE's formulas on the exact axis-aligned planar9 (the azimuth sits on the reference's own
    clamp there): adjoints onto (c, b, d) for an angle cotangent and a harmonics cotangent, and the tangent, once."""
    q = _quads("planar9")
    idx = [i.long() for i in q]
    Rx = _exact("planar9")
    nq = len(q[0])
    g = torch.Generator().manual_seed(41)
    g_ang = torch.zeros(nq, 4, dtype=torch.float64)
    g_ang[:, :2] = torch.randn(nq, 2, generator=g, dtype=torch.float64)
    gY = torch.randn(nq, 49, generator=g, dtype=torch.float64)
    tR = torch.randn(Rx.shape, generator=g, dtype=torch.float64)          # a tangent in the axis frame
    with torch.enable_grad():
        leaves = [Rx[i].clone().requires_grad_(True) for i in (idx[0], idx[2], idx[3])]
        phi, th = CK._quad_angles(leaves[0], Rx[idx[1]], leaves[1], leaves[2])
        Y = CK.B.real_sph_harm_full(7, phi, th)
        G_ang = torch.autograd.grad((g_ang[:, 0] * phi + g_ang[:, 1] * th).sum(), leaves, retain_graph=True)
        G_Y = torch.autograd.grad((gY * Y).sum(), leaves)
    tang = CK._jvp(lambda X: torch.stack(CK._quad_angles(X[idx[0]], X[idx[1]], X[idx[2]], X[idx[3]]), 1), Rx, tR)
    return dict(q=q, g_ang=g_ang, gY=gY, tR=tR, G_ang=G_ang, G_Y=G_Y, Y=Y.detach(), tang=tang)


@pytest.mark.parametrize("orient", SM.ORIENTATIONS)
def test_planar_quadruplet_adjoints_and_tangent_on_all_rows(planar_reference, orient):
    p = planar_reference
    q, Q = p["q"], _rot(orient)
    R = _R("planar9", orient)
    dq = _dev(q)
    got = K.quad_angles_bwd(f32(p["g_ang"]), f32(R), *dq)
    for n_, a, b in zip("cbd", got, p["G_ang"]):
        _elementwise(f"planar9/{orient} quad_angles_bwd G{n_}", a, b @ Q.T)
    Gc, Gbd = K.quad_angles_bwd(f32(p["g_ang"]), f32(R), *dq, packed=True)
    assert torch.equal(Gc, got[0]) and torch.equal(Gbd[:, 0:3], got[1]) and torch.equal(Gbd[:, 4:7], got[2])
    Y = K.quad_basis_fwd(f32(R), *dq, 7).double().cpu()
    print(f"planar9/{orient} quad_basis_fwd max err {float((Y - p['Y']).abs().max()):.2e}")
    assert torch.allclose(Y, p["Y"], rtol=1e-4, atol=2e-5)
    gotY = K.quad_basis_bwd(f32(p["gY"]), f32(R), *dq, 7)
    for n_, a, b in zip("cbd", gotY, p["G_Y"]):
        _elementwise(f"planar9/{orient} quad_basis_bwd G{n_}", a, b @ Q.T)
    Gc, Gbd = K.quad_basis_bwd_packed(f32(p["gY"]), f32(R), *dq, 7)
    assert torch.equal(Gc, gotY[0]) and torch.equal(Gbd[:, 0:3], gotY[1]) and torch.equal(Gbd[:, 4:7], gotY[2])
    tang = K.quad_angles_jvp(f32(R), f32(p["tR"] @ Q.T), *dq)
    assert not tang[:, 2:].any()
    _elementwise(f"planar9/{orient} quad_angles_jvp", tang[:, :2], p["tang"])
    if orient != "axis":
        # every output equals the axis output carried over by the rotation: scalars unchanged, vectors times Q.T
        Ra = f32(_R("planar9", "axis"))
        for n_, a, b in zip("cbd", got, K.quad_angles_bwd(f32(p["g_ang"]), Ra, *dq)):
            _elementwise(f"planar9/{orient} against axis: quad_angles_bwd G{n_}", a, b.double().cpu() @ Q.T)
        for n_, a, b in zip("cbd", gotY, K.quad_basis_bwd(f32(p["gY"]), Ra, *dq, 7)):
            _elementwise(f"planar9/{orient} against axis: quad_basis_bwd G{n_}", a, b.double().cpu() @ Q.T)
        assert torch.allclose(Y, K.quad_basis_fwd(Ra, *dq, 7).double().cpu(), rtol=1e-4, atol=2e-5)
        _elementwise(f"planar9/{orient} against axis: quad_angles_jvp", tang[:, :2],
                     K.quad_angles_jvp(Ra, f32(p["tR"]), *dq)[:, :2].double().cpu())


@pytest.mark.parametrize("orient", SM.ORIENTATIONS)
@pytest.mark.parametrize("name", ["linear5", "benzene"])
def test_collinear_rows_carry_the_convention(name, orient):
    """Where a rejection has vanished: an azimuth-only cotangent gives exact zeros and a position tangent a zero azimuth tangent;
    where c - a - b is collinear the polar angle is a constant as well (so every harmonics cotangent on linear5 gives zeros)."""
    q = _quads(name)
    flat, vanished = _masks(name, q)
    nq = len(flat)
    assert int(vanished.sum()) > 100 and (name != "benzene" or int((vanished & ~flat).sum()) == 576)
    R, dq = _R(name, orient), _dev(q)
    g = torch.Generator().manual_seed(43)
    g_th = torch.zeros(nq, 4, dtype=torch.float64)
    g_th[:, 1] = torch.randn(nq, generator=g, dtype=torch.float64) * vanished
    got = K.quad_angles_bwd(f32(g_th), f32(R), *dq)
    Gc, Gbd = K.quad_angles_bwd(f32(g_th), f32(R), *dq, packed=True)
    print(f"{name}/{orient}: azimuth-only cotangent on {int(vanished.sum())} collinear rows -> max |G| "
          f"{max(float(x.abs().max()) for x in got):.3e}")
    for G in got + (Gc, Gbd):
        assert torch.isfinite(G).all() and not G.any()
    g_phi = torch.zeros(nq, 4, dtype=torch.float64)
    g_phi[:, 0] = torch.randn(nq, generator=g, dtype=torch.float64) * flat
    for G in K.quad_angles_bwd(f32(g_phi), f32(R), *dq):
        assert torch.isfinite(G).all() and not G.any()
    tang = K.quad_angles_jvp(f32(R), f32(torch.randn(R.shape, generator=g, dtype=torch.float64)), *dq).cpu()
    print(f"{name}/{orient}: azimuth tangent on the collinear rows: max {float(tang[vanished, 1].abs().max()):.3e}")
    assert torch.isfinite(tang).all() and not tang[vanished, 1].any() and not tang[flat, 0].any()
    # the other rows of benzene are planar and well conditioned: the adjoint is the restatement's, within the bars
    g_ang = torch.zeros(nq, 4, dtype=torch.float64)
    g_ang[:, :2] = torch.randn(nq, 2, generator=g, dtype=torch.float64)
    for n_, a, b in zip("cbd", K.quad_angles_bwd(f32(g_ang), f32(R), *dq), CK.quad_angles_bwd(g_ang, R, *q)):
        _elementwise(f"{name}/{orient} quad_angles_bwd G{n_}", a, b)
    gY = torch.randn(nq, 49, generator=g, dtype=torch.float64)
    Y = K.quad_basis_fwd(f32(R), *dq, 7).double().cpu()
    assert torch.allclose(Y, CK.quad_basis_fwd(R, *q, 7), rtol=1e-4, atol=2e-5)
    GY = K.quad_basis_bwd(f32(gY), f32(R), *dq, 7)
    for n_, a, b in zip("cbd", GY, CK.quad_basis_bwd(gY, R, *q, 7)):
        _elementwise(f"{name}/{orient} quad_basis_bwd G{n_}", a, b)
    if name == "linear5":
        for G in GY:
            assert not G.any()


# ==================================================================================================== triplet kernels
TRIP_BATCH = ("linear5", "planar9")


def _trip_R(orient, exact=False):
    return torch.cat([_exact(n) @ _rot(orient).T if exact else _R(n, orient) for n in TRIP_BATCH])


@pytest.fixture(scope="module")
def triplet_reference():
    """The triplets and edges of linear5 and planar9 as ONE list (60 exactly collinear rows next to 476 well-conditioned ones:
    max|ref| is set by the latter) and float64 on the exact axis-aligned coordinates: values and first adjoints of the distance,
    the angle and Y_l0 for fixed cotangents, and the tangents.  On a collinear row the float64 adjoint keeps only the d/dx term
    (~1e-9)."""
    t, e, off = [], [], 0
    for name in TRIP_BATCH:
        idx = SM.index_lists(name, "axis")
        t.append([x + off for x in _trips(name)])
        e.append([torch.tensor(idx[k].astype(np.int32)) + off for k in ("id_c", "id_a")])
        off += len(SM.coordinates(name)[1])
    t, e = [torch.cat(x) for x in zip(*t)], [torch.cat(x) for x in zip(*e)]
    Rx = _trip_R("axis", exact=True)
    g = torch.Generator().manual_seed(47)
    gth = torch.randn(len(t[0]), generator=g, dtype=torch.float64)
    gY = torch.randn(len(t[0]), 7, generator=g, dtype=torch.float64)
    gD = torch.randn(len(e[0]), generator=g, dtype=torch.float64)
    tR = torch.randn(Rx.shape, generator=g, dtype=torch.float64)
    Y, th = CK.trip_basis_fwd(Rx, *t, 7, want_theta=True)
    collinear = torch.sin(th) < 1e-6
    assert int(collinear.sum()) == 60 and len(th) == 60 + 476
    return dict(t=t, e=e, gth=gth, gY=gY, gD=gD, tR=tR, th=th, Y=Y, D=CK.dist_fwd(Rx, *e), collinear=collinear,
                G_th=CK.angle_bwd(gth, Rx, *t), G_Y=CK.trip_basis_bwd(gY, Rx, *t), W=CK.dist_bwd(gD, Rx, *e),
                jvp_th=CK.angle_jvp(Rx, tR, gth, *t)[0], jvp_D=CK.dist_jvp(Rx, tR, gD, *e))


@pytest.mark.parametrize("orient", SM.ORIENTATIONS)
def test_triplet_and_distance_kernels_on_all_rows(triplet_reference, orient):
    p = triplet_reference
    Q, R = _rot(orient), _trip_R(orient)
    dt, de = _dev(p["t"]), _dev(p["e"])
    col = p["collinear"]
    cpu = lambda x: x.double().cpu()                                  # noqa: E731
    # values: scalars, unchanged by the rotation
    Y, th = K.trip_basis_fwd(f32(R), *dt, 7, want_theta=True)
    th2 = K.angle_fwd(f32(R), *dt)
    D = K.dist_fwd(f32(R), *de)
    print(f"{orient}: theta err {float((cpu(th) - p['th']).abs().max()):.2e}, Y err {float((cpu(Y) - p['Y']).abs().max()):.2e}, "
          f"D err {float((cpu(D) - p['D']).abs().max()):.2e}")
    assert float((cpu(th) - p["th"]).abs().max()) <= 5e-6 and float((cpu(Y) - p["Y"]).abs().max()) <= 2e-5
    assert torch.allclose(cpu(th2), p["th"], rtol=1e-5, atol=2e-6) and torch.allclose(cpu(D), p["D"], rtol=1e-6, atol=1e-6)

    def adjoint(tag, got, ref):
        """within 2e-4 x max|ref| on all rows, the collinear ones included"""
        sc = float(max(r.abs().max() for r in ref))
        for n_, a, r in zip("cb", got, ref):
            err = (cpu(a) - r @ Q.T).abs()
            print(f"{orient} {tag} G{n_}: max err {float(err.max()):.3e} (collinear rows {float(err[col].max()):.3e}) against "
                  f"2e-4 x {sc:.3f}")
            assert torch.isfinite(a).all() and float(err.max()) <= 2e-4 * sc, (tag, n_)

    # first adjoints: vectors, carried over by the rotation
    G_th, G_Y = K.angle_bwd(f32(p["gth"]), f32(R), *dt), K.trip_basis_bwd(f32(p["gY"]), f32(R), *dt)
    adjoint("angle_bwd", G_th, p["G_th"])
    adjoint("trip_basis_bwd", G_Y, p["G_Y"])
    W = K.dist_bwd(f32(p["gD"]), f32(R), *de)
    assert torch.allclose(cpu(W), p["W"] @ Q.T, rtol=1e-5, atol=1e-5)
    # tangents along the rotated tangent
    tR = f32(p["tR"] @ Q.T)
    thd, Hc, Hb = K.angle_jvp(f32(R), tR, f32(p["gth"]), *dt)
    sc = float(p["jvp_th"].abs().max())
    err = (cpu(thd) - p["jvp_th"]).abs()
    print(f"{orient} angle_jvp theta tangent: max err {float(err.max()):.3e} (collinear rows {float(err[col].max()):.3e}) against "
          f"2e-4 x {sc:.3f}")
    assert torch.isfinite(thd).all() and torch.isfinite(Hc).all() and torch.isfinite(Hb).all() and float(err.max()) <= 2e-4 * sc
    Dd, H = K.dist_jvp(f32(R), tR, f32(p["gD"]), *de)
    assert torch.allclose(cpu(Dd), p["jvp_D"][0], rtol=1e-5, atol=1e-5)
    assert torch.allclose(cpu(H), p["jvp_D"][1] @ Q.T, rtol=1e-4, atol=1e-4 * float(p["jvp_D"][1].abs().max()))
    if orient != "axis":
        # against the axis output carried over by the rotation
        Ra = f32(_trip_R("axis"))
        adjoint("against axis: angle_bwd", G_th, [cpu(x) for x in K.angle_bwd(f32(p["gth"]), Ra, *dt)])
        adjoint("against axis: trip_basis_bwd", G_Y, [cpu(x) for x in K.trip_basis_bwd(f32(p["gY"]), Ra, *dt)])
        assert float((cpu(th) - cpu(K.angle_fwd(Ra, *dt))).abs().max()) <= 5e-6


# ================================================================================================================ models
def _to(inputs):
    return {k: put(v.float() if v.is_floating_point() else v) for k, v in inputs.items()}


def _model(kind, train=False, frozen=False):
    cfg, P = SM.params(kind)
    model = build(cfg, P)
    model = model.train() if train else model.eval()
    if frozen:
        model.requires_grad_(False)
    return model


def _np(t):
    return t.detach().double().cpu().numpy()


def _benzene_checks(F, orient, tag):
    """No force reference under GemNet-Q: finite, and no out-of-plane component."""
    Fa = F @ SM.rotation(orient)[0]
    out, scale = float(np.abs(Fa[:, 2]).max()), max(1.0, float(np.abs(F).mean()))
    print(f"{tag}: out-of-plane force {out:.3e} (bar {MZ.FORCE_MAX_TOL * scale:.1e}); mean|F| {np.abs(F).mean():.3f}, max|F| {np.abs(F).max():.3f}")
    assert np.isfinite(F).all() and out <= MZ.FORCE_MAX_TOL * scale, tag
    return Fa


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_energy_and_forces_of_every_molecule_in_every_orientation(kind):
    model = _model(kind)
    axis = {}
    for name in SM.MOLECULES:
        for o in SM.ORIENTATIONS:
            E, F = model(_to(SM.inputs_of([name], o, kind)))
            torch.cuda.synchronize()
            E, F = _np(E), _np(F)
            SM.assert_force_energy(SM.force_energy_figures(E, F, name, o, kind), f"{kind} {name}/{o}")
            if name == "benzene":
                Fa = _benzene_checks(F, o, f"{kind} benzene/{o}")
                if o == "axis":
                    axis[name] = Fa
                else:
                    d, scale = float(np.abs(Fa - axis[name]).max()), max(1.0, float(np.abs(Fa).mean()))
                    print(f"{kind} benzene/{o}: F @ Q against F(axis) {d:.3e} (bar {MZ.FORCE_MAX_TOL * scale:.1e})")
                    assert d <= MZ.FORCE_MAX_TOL * scale


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_energy_and_forces_of_all_nine_as_one_batch(kind):
    inputs, order = SM.all_nine(kind)
    E, F = _model(kind)(_to(inputs))
    torch.cuda.synchronize()
    E, F = _np(E), _np(F)
    off = 0
    for b, (name, o) in enumerate(order):
        n = len(SM.coordinates(name)[1])
        Fm = F[off:off + n]
        SM.assert_force_energy(SM.force_energy_figures(E[b:b + 1], Fm, name, o, kind), f"{kind} batch of nine, {name}/{o}")
        if name == "benzene":
            _benzene_checks(Fm, o, f"{kind} batch of nine, benzene/{o}")
        off += n


def test_benzene_forces_equal_the_periodic_path_without_images():
    """GemNet-Q: the same molecule through pbc = (F, F, F) in a large cell (the vector-form kernels, which take the relative
    decisions since they exist) — as test_gpu_pbc_q.test_without_images_equals_the_molecular_model, within 1e-5."""
    from gemnet_pytorch_amd.pbc import PeriodicQuadGraphBuilder
    model = _model("Q")
    inputs = _to(SM.inputs_of(["benzene"], "rot3", "Q"))
    E0, F0 = model(dict(inputs))
    R, N = inputs["R"], np.array([12], np.int64)
    cell = put(torch.eye(3)[None] * 40.0)
    b = PeriodicQuadGraphBuilder(N, MZ.CUTOFF, MZ.INT_CUTOFF, pbc=np.zeros((1, 3), bool), device=DEV)
    per = b(torch.tensor(SM.placed("benzene", "rot3"), device=DEV), cell.double())
    per.update(R=R, Z=inputs["Z"], N=inputs["N"], cell=cell)
    model.periodic_quadruplets = True
    E1, F1, _ = model(per, stress=True)
    torch.cuda.synchronize()
    assert len(per["id4_reduce_ca"]) == 11880
    E0, F0, E1, F1 = (x.detach() for x in (E0, F0, E1, F1))
    dE, dF = float((E0 - E1).abs().max()), float((F0 - F1).abs().max())
    print(f"benzene/rot3 molecular against periodic without images: dE {dE:.3e}, dF {dF:.3e} at max|F| {float(F0.abs().max()):.3f}")
    assert bool(torch.isfinite(F0).all()) and bool(torch.isfinite(F1).all())
    assert dE <= 1e-5 * max(1.0, float(E0.abs().max())) and dF <= 1e-5 * max(1.0, float(F0.abs().max()))


def _targets():
    Et, Ft = SM.train_targets("rot3")
    return put(Et.float()), put(Ft.float())


def _check_gradients(named, ref, tag):
    bad = [k for k in ref["grads"] if named[k].grad is None or not bool(torch.isfinite(named[k].grad).all())]
    assert not bad, (tag, "missing or non-finite gradients", bad)
    worst, name, rel = MZ.grad_figures({k: named[k].grad for k in ref["grads"]}, ref)
    print(f"{tag}: worst ||g - g_ref|| = {worst:.3f} of its bar ({name}); worst ||g - g_ref|| / ||g_ref|| = {rel:.2e}")
    assert worst <= 1.0, name


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_training_gradients_on_planar9_and_linear5_rotated(kind):
    ref = SM.training_reference(kind)
    model = _model(kind, train=True)
    E, F = model(_to(SM.inputs_of(SM.TRAIN, "rot3", kind)))
    assert F.requires_grad
    loss = GO.training_loss(E[:, :1], F, *_targets())
    print(f"{kind} planar9 + linear5 / rot3: loss {loss.item():.6f} (float64 {ref['loss']:.6f})")
    assert abs(loss.item() - ref["loss"]) <= MZ.LOSS_RTOL * abs(ref["loss"])
    loss.backward()
    _check_gradients(dict(model.named_parameters()), ref, f"{kind} planar9 + linear5 / rot3")


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_fused_training_step_on_planar9_and_linear5_rotated(kind):
    from gemnet_pytorch_amd.training.ddp import TrainStep
    ref = SM.training_reference(kind)
    ts = TrainStep(_model(kind, train=True), fused_optimizer=True)
    before = ts.fused.flat_p.clone()
    Et, Ft = _targets()
    loss = float(ts(_to(SM.inputs_of(SM.TRAIN, "rot3", kind)), {"E": Et, "F": Ft}))
    torch.cuda.synchronize()
    print(f"{kind} fused step: loss {loss:.6f} (float64 {ref['loss']:.6f})")
    assert abs(loss - ref["loss"]) <= MZ.LOSS_RTOL * abs(ref["loss"])
    _check_gradients(dict(ts.model.named_parameters()), ref, f"{kind} fused step")
    assert all(bool(torch.isfinite(p).all()) for p in ts.model.parameters()) and not torch.equal(before, ts.fused.flat_p)


@pytest.mark.parametrize("train", [False, True])
def test_narrow_gemnet_q_on_planar9_rotated(train):
    """Widths no fused quadruplet path takes: the explicit (Q, 49) harmonics kernels in eval mode, the ATen composite closure
    (GemNet.calculate_angles) in training mode."""
    P, Er, Fr = SM.narrow_reference()
    model = build(SM.cfg_narrow(), P)
    model = model.train() if train else model.eval()
    E, F = model(_to(SM.inputs_of(["planar9"], "rot3", "Q")))
    torch.cuda.synchronize()
    Fr = Fr @ SM.rotation("rot3")[0].T
    mae, mx, de = float(np.abs(_np(F) - Fr).mean()), float(np.abs(_np(F) - Fr).max()), float(np.abs(_np(E) - Er).max())
    print(f"narrow Q planar9/rot3 ({'training' if train else 'eval'} mode): force MAE {mae:.3e} (max {mx:.3e}) at mean|F_ref| "
          f"{np.abs(Fr).mean():.3f}; energy err {de:.3e}")
    assert np.isfinite(_np(F)).all() and mae <= MZ.FORCE_TOL and mx <= MZ.FORCE_MAX_TOL
    assert de <= MZ.ENERGY_TOL * max(1.0, float(np.abs(Er).max()))


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_captured_replays_equal_the_eager_call(kind):
    """planar9/rot3 through ForceGraphs and through the padded runner (index build on the device): bit-identical to eager."""
    from gemnet_pytorch_amd.index_device import DeviceGraphBuilder
    from gemnet_pytorch_amd.padded import PaddedGraphRunner
    from gemnet_pytorch_amd.runtime import ForceGraphs
    model = _model(kind, frozen=True)
    batch = _to(SM.inputs_of(["planar9"], "rot3", kind))
    E0, F0 = model(dict(batch))
    runner = ForceGraphs(model, [batch])
    runner()
    torch.cuda.synchronize()
    E, F = runner.energies_forces()
    assert torch.equal(E, E0) and torch.equal(F, F0), (float((E - E0).abs().max()), float((F - F0).abs().max()))
    N = np.array([9], np.int64)
    R, Z, Nd = batch["R"], batch["Z"], batch["N"]
    idx = DeviceGraphBuilder(N, MZ.CUTOFF, MZ.INT_CUTOFF, kind == "T", device=DEV)(R)
    E1, F1 = model(dict(Z=Z, R=R.clone(), N=Nd, **idx))
    caps = PaddedGraphRunner.suggest_capacities([PaddedGraphRunner.sizes_of(idx)])
    # (four dummy groups: the pad edges of so small a batch would overfill one group's in-degree bound of N - 1 = 8)
    padded = PaddedGraphRunner(model, Z, Nd, caps[0], caps[1], n_groups=4, **({} if kind == "T" else dict(quad_caps=caps[2])))
    bld = DeviceGraphBuilder(N, MZ.CUTOFF, MZ.INT_CUTOFF, kind == "T", device=DEV)
    for rnd in range(2):
        E, F = padded.build_and_run(bld, R, Z=Z, positions_ready=bool(rnd))
        torch.cuda.synchronize()
        assert torch.equal(E, E1) and torch.equal(F, F1), (rnd, float((F - F1).abs().max()))
    SM.assert_force_energy(SM.force_energy_figures(_np(E), _np(F), "planar9", "rot3", kind), f"{kind} padded replay planar9/rot3")


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_device_molecule_on_benzene_rotated(kind):
    from gemnet_pytorch_amd.md import DeviceMolecule
    model = _model(kind, frozen=True)
    R = SM.placed("benzene", "rot3").astype(np.float32)
    Z = SM.coordinates("benzene")[1]
    E0 = float(model(_to(SM.inputs_of(["benzene"], "rot3", kind)))[0].detach())
    dm = DeviceMolecule(R, Z, MZ.CUTOFF, MZ.INT_CUTOFF, triplets_only=kind == "T")
    dm.to(DEV)
    Er = SM.reference("benzene", "rot3", kind)[0]
    for call in range(2):
        dm.update(R=R)
        E, F = model.predict(dm.get())
        E, F = float(E), F.double().numpy()
        d0, dr = abs(E - E0), abs(E - float(Er[0, 0]))
        print(f"{kind} DeviceMolecule benzene/rot3 call {call}: |E - E_eager| {d0:.3e}, |E - E_ref| {dr:.3e}")
        bar = MZ.ENERGY_TOL * max(1.0, abs(float(Er[0, 0])))
        assert d0 <= bar and dr <= bar and np.isfinite(F).all()
        _benzene_checks(F.reshape(-1, 3), "rot3", f"{kind} DeviceMolecule call {call}")
