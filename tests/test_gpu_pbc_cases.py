"""GPU: the periodic path of GemNet-T where the four toy structures of tests/test_gpu_pbc.py do not reach — cells with a height
below cutoff / 2, strongly sheared and left-handed cells, mixed periodic axes, self-image edges with their exactly collinear
triplets, batches beyond one wavefront / 1024 rows (tests/pbc_common.py: NEW_KINDS, gas, zoo, isolated), and the six first-order
kernels of csrc/pbc.hip one by one against fp64 restatements (tests/cpu_kernels.py).

a. device builder (csrc/pbc.hip) against brute force, integer equality;  b. in-graph builder (csrc/pbc_index.hip), both fill
branches;  c. kernels;  d. model against the golden cluster oracle (tests/golden/pbc_cases.npz).  CPU references are computed
once (lru_cache) and never modified."""
import functools

import numpy as np
import pytest
import torch

import cpu_kernels as CK
import pbc_common as P
from conftest import GOLDEN, SCALE_FILE
from oracle import basis_oracle as B
from oracle import gemnet_oracle as GO

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN_CASES = ("cubic1", "bcc", "bcc_pert", "thin", "skewed", "skewed_lh")
IDX_KEYS = ("id_c", "id_a", "id_swap", "id_undir", "cell_offsets", "id3_reduce_ca", "id3_expand_ba")


def _check_invariants(idx):
    E = len(idx["id_a"])
    H = E // 2
    swap, undir = idx["id_swap"], idx["id_undir"]
    assert np.array_equal(swap[swap], np.arange(E))
    assert np.array_equal(idx["id_a"][swap], idx["id_c"]) and np.array_equal(idx["id_c"][swap], idx["id_a"])
    assert np.array_equal(idx["cell_offsets"][swap], -idx["cell_offsets"])
    assert np.array_equal(undir, np.concatenate([np.arange(H), np.arange(H)]))
    f = np.column_stack([idx["id_a"][:H], idx["id_c"][:H], idx["cell_offsets"][:H].reshape(H, 3)])
    assert np.array_equal(np.lexsort(f.T[::-1]), np.arange(H))                  # sorted by (i, j, n0, n1, n2)
    assert all(a < c or (a == c and (n0, n1, n2) > (0, 0, 0)) for a, c, n0, n1, n2 in f.tolist())
    red, exp = idx["id3_reduce_ca"], idx["id3_expand_ba"]
    assert (red != exp).all() and (idx["id_a"][red] == idx["id_a"][exp]).all()
    assert np.array_equal(np.lexsort((exp, red)), np.arange(len(red)))


def _unwrapped():
    out = []
    for kind, moves in (("thin", ((3, -2, 0), (-5, 0, 4))), ("skewed", ((-4, 2, 0), (0, 5, -3), (2, 0, 0)))):
        R, Z, cell, pbc = P.structure(kind)
        R = R + np.array(moves, np.float64) @ cell                  # whole lattice vectors: the same crystal
        out.append((R, Z, cell, pbc))
    return out


@functools.lru_cache(maxsize=None)
def _case(name, rounded):
    """-> (structs, brute-force dict).  rounded: positions and cells rounded through float32 first (what a float32 build sees);
    no pair of the rounded inputs lies within 1e-5 A of the cutoff, so the float32 list is the fp64 list of the same inputs."""
    if name.startswith("kind:"):
        structs = [P.structure(name[5:])]
    elif name == "kinds":
        structs = [P.structure(k, seed=i) for i, k in enumerate(P.NEW_KINDS + ["cubic1"])]
    elif name == "unwrapped":
        structs = _unwrapped()
    else:
        structs = {"gas": lambda: [P.gas()], "zoo": P.zoo, "isolated": lambda: P.isolated(7)}[name]()
    if rounded:
        structs = [P.f32_round(s) for s in structs]
    R, Z, N, cell, pbc = P.arrays(structs)
    ref = P.brute_force_fast(R, N, cell, pbc, P.CUTOFF)
    if rounded:
        assert P.cutoff_margin_ok(R, N, cell, pbc, margin=1e-5), "a pair sits on the cutoff: change the recipe"
    return structs, ref


def _device_indices(structs, dtype, index_dtype=torch.int64):
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder
    R, Z, N, cell, pbc = P.arrays(structs)
    b = PeriodicGraphBuilder(N, P.CUTOFF, pbc=pbc, device=DEV)
    idx = b(torch.tensor(R, dtype=dtype, device=DEV), torch.tensor(cell, dtype=dtype, device=DEV), dtype=index_dtype)
    return idx, b


# ------------------------------------------------------------------------------------------------- a. device builder
BUILDER_CASES = ["kind:" + k for k in P.NEW_KINDS] + ["kinds", "unwrapped", "gas", "zoo", "isolated"]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", BUILDER_CASES)
def test_device_builder_equals_brute_force(name, dtype):
    """Every key integer-equal to brute force (fp64 on the same inputs), canonical order and the swap / triplet invariants.
    'gas' (1100 atoms, 3324 edges, 10 044 triplets) and 'zoo' (1188 atoms in 46 structures) take every single-block scan of
    pbc.hip through more than one round of 1024; 'skewed_lh' has det < 0; 'thin' / 'skewed' need images up to |n| = 3."""
    structs, ref = _case(name, dtype == torch.float32)
    idx, _ = _device_indices(structs, dtype)
    idx = {k: v.cpu().numpy() for k, v in idx.items()}
    assert set(ref) <= set(idx)
    for k in ref:
        assert idx[k].shape == ref[k].shape and np.array_equal(idx[k], ref[k]), k
    _check_invariants(idx)
    if name == "isolated":
        assert len(idx["id_a"]) == 0 and len(idx["id3_reduce_ca"]) == 0 and len(idx["batch_seg"]) == 7
    if name == "unwrapped":            # the same crystal as the wrapped structures: same counts
        wrapped = P.brute_force_fast(*[P.arrays([P.structure("thin"), P.structure("skewed")])[i] for i in (0, 2, 3, 4)], P.CUTOFF)
        assert len(wrapped["id_a"]) == len(idx["id_a"]) and len(wrapped["id3_reduce_ca"]) == len(idx["id3_reduce_ca"])
        assert np.abs(idx["cell_offsets"]).max() >= 5


# ------------------------------------------------------------------------------------------------------------ model
@functools.lru_cache(maxsize=None)
def _params():
    return P.make_params()


def _new_model():
    from gemnet_pytorch_amd.model.gemnet import GemNet
    m = GemNet(**P.CFG, scale_file=SCALE_FILE)
    m.load_state_dict(GO.expand_to_reference_state_dict({k: v.float() for k, v in _params().items()}))
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _model():
    """The model of the eager comparisons (tests that capture graphs take a model of their own)."""
    return _new_model()


def _batch(structs):
    idx, _ = _device_indices(structs, torch.float64)
    R, Z, N, cell, pbc = P.arrays(structs)
    inputs = dict(idx)
    inputs.update(R=torch.tensor(R, dtype=torch.float32, device=DEV), Z=torch.tensor(Z, device=DEV).long(),
                  N=torch.tensor(N, device=DEV), cell=torch.tensor(cell, dtype=torch.float32, device=DEV))
    return inputs


def _run(structs):
    E, F, S = _model()(_batch(structs), stress=True)
    torch.cuda.synchronize()
    return E.double().cpu().numpy(), F.double().cpu().numpy(), S.double().cpu().numpy()


# ------------------------------------------------------------------------------------------------- b. in-graph builder
def _image_box_sizes(R, cell, pbc):
    return [int(np.prod(np.subtract(*P.image_box(R[i], R[j], cell, pbc)[::-1]) + 1))
            for i in range(len(R)) for j in range(i, len(R))]


@pytest.mark.parametrize("name", ["kinds", "kind:thin", "zoo"])
def test_in_graph_builder_equals_brute_force_and_eager(name):
    """PaddedGraphRunner.attach_builder: the capture runs on a displaced copy of the case (another list), then ONE replay on the
    case itself: rows [:E] / [:T] of the runner's buffers equal brute force, no error bit, and E, F, S are torch.equal to the
    eager call.  'thin' has one pair with an image box above 64 cells (the re-testing fill branch of pbx_pairs_kernel) and
    pairs at or below 64 (the hit-mask branch); 'zoo' has structures of 1, 2, 63, 64, 65 and ~130 atoms around its 64-lane
    partner loop and more than 1024 atoms / edges / triplets for pbx_scan_kernel."""
    from gemnet_pytorch_amd.padded import PaddedGraphRunner
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder
    structs, ref = _case(name, True)
    R, Z, N, cell, pbc = P.arrays(structs)
    if "thin" in name or name == "kinds":
        thin = P.f32_round(P.structure("thin"))
        sizes = _image_box_sizes(thin[0], thin[2], thin[3])
        assert min(sizes) <= 64 < max(sizes), sizes
    # the geometry the graph is captured on: every atom displaced (float32), so that its list is another one
    R1 = (R + np.random.RandomState(3).normal(0, 0.15, R.shape)).astype(np.float32).astype(np.float64)
    first = P.brute_force_fast(R1, N, cell, pbc, P.CUTOFF)
    assert len(first["id_a"]) != len(ref["id_a"]) or not np.array_equal(first["id_c"], ref["id_c"]) \
        or not np.array_equal(first["cell_offsets"], ref["cell_offsets"])
    nE, nT = len(ref["id_a"]), len(ref["id3_reduce_ca"])
    e_cap = max(nE, len(first["id_a"])) // 4 * 4 + 16
    t_cap = max(nT, len(first["id3_reduce_ca"])) // 2 * 2 + 8
    deg = int(max(np.bincount(ref["id_a"]).max(), np.bincount(first["id_a"]).max())) + 2
    model = _new_model()
    Zd, Nd = torch.tensor(Z, device=DEV).long(), torch.tensor(N, device=DEV)
    Rd, R1d, cd = (torch.tensor(x, dtype=torch.float32, device=DEV) for x in (R, R1, cell))
    builder = PeriodicGraphBuilder(N, P.CUTOFF, pbc=pbc, device=DEV)
    idx = builder(Rd, cd, dtype=torch.int32)
    E0, F0, S0 = (t.clone() for t in model(dict(Z=Zd, N=Nd, R=Rd.clone(), cell=cd.clone(), **idx), stress=True))
    torch.cuda.synchronize()
    n_groups = max(1, -(-(e_cap // 4) // max(deg // 2, 1)))
    run = PaddedGraphRunner(model, Zd, Nd, e_cap, t_cap, max_in_degree=deg, n_groups=n_groups, cell=cd, pbc=pbc)
    run._fill(R1d, builder(R1d, cd, dtype=torch.int32), cell=cd)
    run.attach_builder(builder)
    run.run_positions(R1d, cell=cd)                      # capture (+ its replay) on the displaced geometry
    torch.cuda.synchronize()
    assert run.index_error() == 0
    graph = run.graph
    E, F = run.run_positions(Rd, cell=cd)                # the replay under test
    torch.cuda.synchronize()
    assert run.graph is graph and run.index_error() == 0, run.index_error()
    assert run.index_sizes() == (nE, nT)
    assert run.index_in_degree() == int(np.bincount(ref["id_a"]).max())
    buf = run.padded_inputs()
    for k in IDX_KEYS:
        n = nT if k.startswith("id3") else nE
        assert np.array_equal(buf[k][:n].cpu().numpy(), np.asarray(ref[k]).reshape(buf[k][:n].shape)), k
        assert torch.equal(buf[k][:n], idx[k].reshape(buf[k][:n].shape)), k
    assert torch.equal(E, E0) and torch.equal(F, F0) and torch.equal(run.stress(), S0)
    assert torch.isfinite(E0).all() and torch.isfinite(F0).all() and torch.isfinite(S0).all()


# ------------------------------------------------------------------------------------------------------- c. kernels
def close(a, b, rtol=0.0, atol=0.0):
    torch.testing.assert_close(a.detach().cpu().double(), b.detach().cpu().double(), rtol=rtol, atol=atol)


f32 = lambda t: t.float().to(DEV).contiguous()       # noqa: E731
dev = lambda t: t.to(DEV).contiguous()               # noqa: E731
CUT, PEXP, S_, NR = 6.0, 5, 7, 6


def _lib():
    from gemnet_pytorch_amd import _lib as L
    return L


def k_edge_vec(R, id_c, id_a, batch_seg, cell, offs):
    L = _lib()
    E = id_c.shape[0]
    V = torch.full((E, 3), float("nan"), device=DEV)
    L.check(L.load().gn_pbc_edge_vec_f32(L.ptr(R), L.ptr(id_c), L.ptr(id_a), L.ptr(batch_seg), L.ptr(cell), L.ptr(offs), L.ptr(V),
                                         E, L.stream()), "gn_pbc_edge_vec_f32")
    return V


def k_edge_fwd(V, freq, z, nrm):
    L = _lib()
    E = V.shape[0]
    D = torch.full((E,), float("nan"), device=DEV)
    rbf = torch.full((E, NR), float("nan"), device=DEV)
    rad = torch.full((E, S_, NR), float("nan"), device=DEV)
    L.check(L.load().gn_edge_basis_vec_fwd_f32(L.ptr(V), L.ptr(freq), L.ptr(z), L.ptr(nrm), L.ptr(D), L.ptr(rbf), L.ptr(rad), E, NR,
                                               S_, CUT, PEXP, L.stream()), "gn_edge_basis_vec_fwd_f32")
    return D, rbf, rad


def k_edge_bwd(gD, g_rbf, g_rad, V, freq, z, nrm):
    L = _lib()
    E = V.shape[0]
    W = torch.full((E, 3), float("nan"), device=DEV)
    L.check(L.load().gn_edge_basis_vec_bwd_f32(L.ptr(gD), L.ptr(g_rbf), L.ptr(g_rad), L.ptr(V), L.ptr(freq), L.ptr(z), L.ptr(nrm),
                                               L.ptr(W), E, NR, S_, CUT, PEXP, L.stream()), "gn_edge_basis_vec_bwd_f32")
    return W


def k_trip_fwd(V, red, exp):
    L = _lib()
    T = red.shape[0]
    Y = torch.full((T, S_), float("nan"), device=DEV)
    th = torch.full((T,), float("nan"), device=DEV)
    L.check(L.load().gn_trip_basis_vec_fwd_f32(L.ptr(V), L.ptr(red), L.ptr(exp), L.ptr(Y), L.ptr(th), T, S_, L.stream()),
            "gn_trip_basis_vec_fwd_f32")
    return Y, th


def k_trip_bwd(gY, V, red, exp):
    L = _lib()
    T = red.shape[0]
    Gu = torch.full((T, 3), float("nan"), device=DEV)
    Gv = torch.full((T, 3), float("nan"), device=DEV)
    L.check(L.load().gn_trip_basis_vec_bwd_f32(L.ptr(gY), L.ptr(V), L.ptr(red), L.ptr(exp), L.ptr(Gu), L.ptr(Gv), T, S_, L.stream()),
            "gn_trip_basis_vec_bwd_f32")
    return Gu, Gv


def k_stress(V, G, perm, seg, cell):
    L = _lib()
    Bn = cell.shape[0]
    S = torch.full((Bn, 3, 3), float("nan"), device=DEV)
    L.check(L.load().gn_pbc_stress_f32(L.ptr(V), L.ptr(G), L.ptr(perm), L.ptr(seg), L.ptr(cell), Bn, -1.0, L.ptr(S), L.stream()),
            "gn_pbc_stress_f32")
    return S


def _basis_consts():
    return (torch.arange(1, NR + 1, dtype=torch.float64) * np.pi, torch.tensor(B.jn_zeros(S_, NR)),
            torch.tensor(B.sph_bessel_normalizer(S_, NR)))


def _vectors(g, E):
    """E vectors of length 0.8 .. 5 A (float32-exact); 1 = 2 x vector 0 and 2 = -vector 0 (exact in float32)."""
    d = torch.randn(E, 3, generator=g, dtype=torch.float64)
    V = d / d.norm(dim=1, keepdim=True) * (0.8 + 4.2 * torch.rand(E, 1, generator=g, dtype=torch.float64))
    V[0] = V[0] / V[0].norm() * 2.0
    V = V.float().double()
    V[1], V[2] = 2.0 * V[0], -V[0]
    return V


def _pairs(g, E, T):
    red = torch.randint(0, E, (T,), generator=g)
    exp = (red + 1 + torch.randint(0, E - 1, (T,), generator=g)) % E
    # planted exactly collinear triplets, also in the last rows: theta = 0 between V and 2V, theta = pi between V and -V
    for t, (r, x) in ((0, (0, 1)), (1, (0, 2)), (2, (1, 0)), (T - 2, (2, 0)), (T - 1, (1, 2))):
        red[t], exp[t] = r, x
    return red.int(), exp.int(), torch.tensor([0, 1, 2, T - 2, T - 1])


def _sample(n, boundary, g, k=20000):
    """About k rows of range(n): the first rows, the rows on either side of the stride boundary, the last rows, random ones."""
    rows = torch.cat([torch.arange(0, 4000), torch.arange(boundary - 4000, min(boundary + 4000, n)), torch.arange(n - 2000, n),
                      torch.randint(0, n, (k - 14000,), generator=g)])
    return torch.unique(rows)


@functools.lru_cache(maxsize=None)
def _edge_case(E, sampled):
    g = torch.Generator().manual_seed(41 + E)
    V = _vectors(g, E)
    freq, z, nrm = _basis_consts()
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()      # noqa: E731
    gD, grbf, grad = rnd(E), rnd(E, NR), rnd(E, S_, NR)
    rows = _sample(E, 131072, g) if sampled else torch.arange(E)
    ref_fwd = CK.edge_basis_vec_fwd(V[rows], freq, z, nrm, CUT, PEXP)
    ref_bwd = CK.edge_basis_vec_bwd(gD[rows], grbf[rows], grad[rows], V[rows], freq, z, nrm, CUT, PEXP)
    return V, (gD, grbf, grad), rows, ref_fwd, ref_bwd


@pytest.mark.parametrize("E", [1000, 131072 + 37])
def test_edge_basis_vec_kernels(E):
    """gn_edge_basis_vec_fwd/bwd_f32 against the fp64 restatement: E = 1000 (no multiple of 16, 64, 256), and E = 131 072 + 37,
    where the forward kernel's grid is capped (8192 blocks x 256 threads / 16 lanes per edge) and the last 37 edges are
    reached by its stride loop (reference on ~20 000 sampled rows around the boundary and at the end).  Bars of the molecular
    twin, test_gpu_kernels.test_edge_basis_fused_fwd_bwd."""
    V, (gD, grbf, grad), rows, (rD, rrbf, rrad), rW = _edge_case(E, E > 1000)
    freq, z, nrm = _basis_consts()
    args = (f32(V), f32(freq), f32(z), dev(nrm))
    D, rbf, rad = k_edge_fwd(*args)
    r = rows.to(DEV)
    assert torch.isfinite(D).all() and torch.isfinite(rbf).all() and torch.isfinite(rad).all()      # every row was written
    close(D[r], rD, atol=2e-6)
    close(rbf[r], rrbf, atol=1e-5)
    close(rad[r], rrad, rtol=1e-4, atol=2e-5)
    W = k_edge_bwd(f32(gD), f32(grbf), f32(grad), *args)
    assert torch.isfinite(W).all()
    close(W[r], rW, rtol=2e-4, atol=2e-4 * float(rW.abs().max()))
    # outside the sample: D against |V| directly
    close(D, V.norm(dim=1), atol=2e-6)
    D2, rbf2, rad2 = k_edge_fwd(*args)
    assert torch.equal(D, D2) and torch.equal(rbf, rbf2) and torch.equal(rad, rad2)
    assert torch.equal(W, k_edge_bwd(f32(gD), f32(grbf), f32(grad), *args))


@functools.lru_cache(maxsize=None)
def _trip_case(E, T, sampled):
    g = torch.Generator().manual_seed(43 + T % 1000)
    V = _vectors(g, E)
    red, exp, planted = _pairs(g, E, T)
    gY = torch.randn(T, S_, generator=g, dtype=torch.float32).double()
    rows = torch.unique(torch.cat([_sample(T, 2097152, g), planted])) if sampled else torch.arange(T)
    rY, rth = CK.trip_basis_vec_fwd(V, red[rows], exp[rows], S_)
    rGu, rGv = CK.trip_basis_vec_bwd(gY[rows], V, red[rows], exp[rows])
    where = torch.searchsorted(rows, planted)
    return V, red, exp, gY, rows, where, (rY, rth, rGu, rGv)


@pytest.mark.parametrize("T", [5003, 2097152 + 5])
def test_trip_basis_vec_kernels(T):
    """gn_trip_basis_vec_fwd/bwd_f32 against the fp64 restatement on 1000 edge vectors: T = 5003, and T = 2 097 152 + 5 where the
    grid is capped (8192 x 256) and the last 5 triplets come from the stride loop (reference on ~20 000 sampled rows).  Planted
    rows are exactly collinear (theta = 0: V and 2V; theta = pi: V and -V) and hit the max(|u x v|, 1e-9) clamp.  Bars of
    test_gpu_kernels.test_trip_basis_fused_fwd_bwd_including_collinear; adjoint on the triplets with sin(theta) >= 0.3."""
    V, red, exp, gY, rows, where, (rY, rth, rGu, rGv) = _trip_case(1000, T, T > 5003)
    Vd, rd, xd, gYd = f32(V), dev(red), dev(exp), f32(gY)
    Y, th = k_trip_fwd(Vd, rd, xd)
    r = rows.to(DEV)
    assert torch.isfinite(Y).all() and torch.isfinite(th).all()
    print("theta err", float((th[r].cpu().double() - rth).abs().max()), "Y err", float((Y[r].cpu().double() - rY).abs().max()))
    close(th[r], rth, atol=5e-6)
    close(Y[r], rY, atol=2e-5)
    assert float(rth[where].min()) < 1e-8 and abs(float(rth[where].max()) - np.pi) < 1e-8
    Gu, Gv = k_trip_bwd(gYd, Vd, rd, xd)
    assert torch.isfinite(Gu).all() and torch.isfinite(Gv).all()
    well = torch.sin(rth) >= 0.3
    assert int(well.sum()) > len(rows) // 2
    wd = r[well.to(DEV)]
    close(Gu[wd], rGu[well], rtol=2e-3, atol=2e-3 * float(rGu[well].abs().median()))
    close(Gv[wd], rGv[well], rtol=2e-3, atol=2e-3 * float(rGv[well].abs().median()))
    # the clamped rows: the reference's value (only the d/dx term survives the clamp) within 1e-6 |gY|
    p = r[where.to(DEV)]
    bar = 1e-6 * gY[rows[where]].norm(dim=1, keepdim=True)
    eu, ev = (Gu[p].cpu().double() - rGu[where]).abs(), (Gv[p].cpu().double() - rGv[where]).abs()
    print("collinear rows: |Gu - ref|", eu.max(1).values.tolist(), "|Gv - ref|", ev.max(1).values.tolist(), "bar", bar.flatten().tolist())
    assert (eu <= bar).all() and (ev <= bar).all()
    Y2, th2 = k_trip_fwd(Vd, rd, xd)
    Gu2, Gv2 = k_trip_bwd(gYd, Vd, rd, xd)
    assert torch.equal(Y, Y2) and torch.equal(th, th2) and torch.equal(Gu, Gu2) and torch.equal(Gv, Gv2)


def test_edge_vec_kernel():
    """gn_pbc_edge_vec_f32: V = R[a] - (R[c] + n cell_b) on three structures (a thin, a triclinic and a left-handed cell), image
    offsets up to |n| = 3, E = 1000.  2e-6: four float32 roundings of numbers below 16 (half an ulp: 4.8e-7 each)."""
    g = torch.Generator().manual_seed(47)
    tri = P.structure("triclinic")[2]
    cells = np.stack([P.structure("thin")[2], tri, tri[[1, 0, 2]]]).astype(np.float32).astype(np.float64)
    N = [5, 9, 7]
    off = np.concatenate([[0], np.cumsum(N)])
    frac = torch.rand(sum(N), 3, generator=g, dtype=torch.float64).numpy() * 0.5
    batch_seg = np.repeat(np.arange(3), N)
    R = np.einsum("ak,akj->aj", frac, cells[batch_seg]).astype(np.float32).astype(np.float64)
    E = 1000
    mol = torch.randint(0, 3, (4 * E,), generator=g).numpy()
    n = torch.randint(-3, 4, (4 * E, 3), generator=g).numpy()
    ok = (np.abs(np.einsum("ek,ekj->ej", n.astype(np.float64), cells[mol])).max(1) <= 7.5) & (np.abs(n[:, 1:]).max(1) <= 2)
    mol, n = mol[ok][:E], n[ok][:E]
    assert len(mol) == E and np.abs(n).max() == 3 and set(mol) == {0, 1, 2}
    pick = lambda: np.array([off[m] + int(torch.randint(0, N[m], (1,), generator=g)) for m in mol])      # noqa: E731
    id_a, id_c = pick(), pick()
    t = lambda x, dt: torch.tensor(x, dtype=dt)                                                          # noqa: E731
    ref = CK.pbc_edge_vec(t(R, torch.float64), t(id_c, torch.int64), t(id_a, torch.int64), t(batch_seg, torch.int64),
                          t(cells, torch.float64), t(n, torch.int64))
    a = (f32(t(R, torch.float64)), dev(t(id_c, torch.int32)), dev(t(id_a, torch.int32)), dev(t(batch_seg, torch.int32)),
         f32(t(cells, torch.float64)), dev(t(n, torch.int32)))
    V = k_edge_vec(*a)
    close(V, ref, atol=2e-6)
    assert torch.equal(V, k_edge_vec(*a))
    assert (id_a == id_c).any()                        # self-image edges: V = -n cell
    own = torch.tensor(id_a == id_c)
    close(V[own.to(DEV)], -torch.einsum("ek,ekj->ej", t(n, torch.float64), t(cells, torch.float64)[t(mol, torch.int64)])[own],
          atol=2e-6)


@pytest.mark.parametrize("with_perm", [True, False])
def test_stress_kernel(with_perm):
    """gn_pbc_stress_f32: four structures with 0, 1, 300 and 700 edges (one workgroup each, 256 threads striding over the
    segment), an unsorted permutation, one left-handed cell (|det|).  The kernel accumulates in f64: 1e-5 of max |ref|."""
    g = torch.Generator().manual_seed(53)
    counts = [0, 1, 300, 700]
    E = sum(counts)
    V = _vectors(g, E)
    G = torch.randn(E, 3, generator=g, dtype=torch.float64).float().double()
    cell = (torch.randn(4, 3, 3, generator=g, dtype=torch.float64) * 0.4 + torch.eye(3, dtype=torch.float64) * 3.0)
    cell[2] = cell[2][[1, 0, 2]]
    cell = cell.float().double()
    assert float(torch.linalg.det(cell[2])) < 0 < float(torch.linalg.det(cell[3]))
    seg = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    if with_perm:
        key = torch.repeat_interleave(torch.arange(4), torch.tensor(counts))[torch.randperm(E, generator=g)]      # structure of edge e
        shuffled = torch.randperm(E, generator=g)
        perm = torch.cat([shuffled[key[shuffled] == b] for b in range(4)]).int()        # grouped by structure, unsorted inside
        assert not bool((perm[1:301].diff() > 0).all())
    else:
        perm = None
    ref = CK.pbc_stress(V, G, perm, seg, cell)
    a = (f32(V), f32(G), None if perm is None else dev(perm), dev(seg), f32(cell))
    S = k_stress(*a)
    err = float((S.cpu().double() - ref).abs().max())
    print("stress err", err, "max |ref|", float(ref.abs().max()))
    assert err <= 1e-5 * float(ref.abs().max())
    assert not S[0].any() and float(S[1].abs().max()) > 0
    assert torch.equal(S, k_stress(*a))
    # one structure's tensor does not depend on the others: the 700-edge structure alone
    if not with_perm:
        alone = k_stress(f32(V[301:]), f32(G[301:]), None, dev(torch.tensor([0, 700], dtype=torch.int32)), f32(cell[3:]))
        assert torch.equal(alone[0], S[3])


def test_empty_calls():
    """E = 0 / T = 0 / B = 0: success without a launch."""
    freq, z, nrm = _basis_consts()
    e3, e1 = torch.zeros(0, 3, device=DEV), torch.zeros(0, device=DEV)
    none = torch.zeros(0, dtype=torch.int32, device=DEV)
    V = f32(_vectors(torch.Generator().manual_seed(1), 8))
    assert k_edge_vec(V, none, none, none, torch.eye(3, device=DEV)[None].contiguous(), none.reshape(0, 3)).shape == (0, 3)
    D, rbf, rad = k_edge_fwd(e3, f32(freq), f32(z), dev(nrm))
    assert D.shape == (0,) and rbf.shape == (0, NR) and rad.shape == (0, S_, NR)
    assert k_edge_bwd(e1, torch.zeros(0, NR, device=DEV), torch.zeros(0, S_, NR, device=DEV), e3, f32(freq), f32(z), dev(nrm)).shape == (0, 3)
    Y, th = k_trip_fwd(V, none, none)
    assert Y.shape == (0, S_) and th.shape == (0,)
    assert all(t.shape == (0, 3) for t in k_trip_bwd(torch.zeros(0, S_, device=DEV), V, none, none))
    assert k_stress(e3, e3, none, torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(0, 3, 3, device=DEV)).shape == (0, 3, 3)
    # a structure without edges inside a batch: zeros
    S = k_stress(e3, e3, none, torch.zeros(3, dtype=torch.int32, device=DEV), torch.eye(3, device=DEV).repeat(2, 1, 1).contiguous())
    assert S.shape == (2, 3, 3) and not S.any()


# ---------------------------------------------------------------------------- d. model against the golden cluster oracle
@functools.lru_cache(maxsize=None)
def _golden():
    import os
    return dict(np.load(os.path.join(GOLDEN, "pbc_cases.npz")))


@pytest.mark.parametrize("kind", GOLDEN_CASES)
def test_energy_forces_stress_match_golden_cluster_oracle(kind):
    """E, F, S of the cells with self-image edges, collinear triplets, |n| up to 3 and det < 0 against the fp64 cluster oracle
    stored in tests/golden/pbc_cases.npz, with the bars (and floors) of test_gpu_pbc.test_energy_forces_stress_match_cluster_oracle.
    'cubic1' has nothing but self-image edges: they cancel in F and carry all of S."""
    g = _golden()
    R, Z, cell, pbc = P.structure(kind)
    assert np.array_equal(g[kind + ".R"], R) and np.array_equal(g[kind + ".cell"], cell)
    E, F, S = _run([(R, Z, cell, pbc)])
    E_ref, F_ref, S_ref = float(g[kind + ".E"]), g[kind + ".F"], g[kind + ".S"]
    scale = max(1.0, float(np.abs(F_ref).mean()))
    print(kind, E[0, 0], E_ref, "F err mean/max", np.abs(F - F_ref).mean(), np.abs(F - F_ref).max(), "S err",
          np.abs(S[0] - S_ref).max(), "max|S_ref|", np.abs(S_ref).max(), "asym", np.abs(S[0] - S[0].T).max())
    assert abs(E[0, 0] - E_ref) <= 2e-5 * max(1.0, abs(E_ref))
    assert np.abs(F - F_ref).mean() <= 1e-5 * scale and np.abs(F - F_ref).max() <= 1e-4 * scale
    assert np.abs(S[0] - S_ref).max() <= 1e-4 * max(np.abs(S_ref).max(), 1e-2)
    assert np.abs(S[0] - S[0].T).max() <= 1e-5 * max(np.abs(S_ref).max(), 1e-2)


def test_batch_of_golden_cases_equals_single_runs():
    structs = [P.structure(k) for k in GOLDEN_CASES]
    E, F, S = _run(structs)
    off = 0
    for b, s in enumerate(structs):
        e, f, st = _run([s])
        n = len(s[0])
        assert abs(E[b, 0] - e[0, 0]) <= 1e-5 * max(1.0, abs(e[0, 0]))
        assert np.abs(F[off:off + n] - f).max() <= 1e-5 * max(1.0, np.abs(f).max())
        assert np.abs(S[b] - st[0]).max() <= 1e-5 * max(1e-2, np.abs(st).max())
        off += n


def _supercell():
    R, Z, cell, pbc = P.structure("bcc_pert")
    shifts = [np.array(n) @ cell for n in np.ndindex(3, 3, 3)]
    return (R, Z, cell, pbc), (np.concatenate([R + t for t in shifts]), np.tile(Z, 27), 3 * cell, pbc)


def test_supercell_of_bcc_pert():
    """3 x 3 x 3 supercell: 54 atoms, 756 edges in ONE structure (three strides of the 256-thread stress kernel), 9828 triplets:
    27 E, tiled F, the same S, within the tolerances of test_gpu_pbc.test_invariances."""
    unit, big = _supercell()
    E, F, S = _run([unit])
    idx, _ = _device_indices([big], torch.float64)
    assert (len(big[0]), idx["id_a"].shape[0], idx["id3_reduce_ca"].shape[0]) == (54, 756, 9828)
    assert int(torch.unique(idx["batch_seg"]).numel()) == 1
    tolE, tolF, tolS = 2e-5 * max(1.0, abs(E[0, 0])), 5e-5 * max(1.0, np.abs(F).max()), 5e-5 * max(1e-2, np.abs(S).max())
    e, f, s = _run([big])
    print("supercell", e[0, 0], 27 * E[0, 0], np.abs(f - np.tile(F, (27, 1))).max(), np.abs(s - S).max())
    assert abs(e[0, 0] - 27 * E[0, 0]) <= 27 * tolE
    assert np.abs(f - np.tile(F, (27, 1))).max() <= tolF
    assert np.abs(s - S).max() <= tolS
    assert np.abs(s[0] - s[0].T).max() <= tolS


def test_force_graphs_replay_supercell():
    from gemnet_pytorch_amd.runtime import ForceGraphs
    model = _new_model()
    _, big = _supercell()
    batch = _batch([big])
    fg = ForceGraphs(model, [batch])
    g = torch.Generator(device=DEV).manual_seed(7)
    R2 = batch["R"] + 0.01 * torch.randn(batch["R"].shape, generator=g, device=DEV)
    cell2 = batch["cell"] @ (torch.eye(3, device=DEV) + 0.002 * torch.randn(3, 3, generator=g, device=DEV))
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
