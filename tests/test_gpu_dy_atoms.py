"""-m gpu: the triplet Y gradient per atom on the matrix cores (gn_bil_dy_atoms_f32 behind
kernels.bil_dy_multi, GEMNET_DY_ATOMS).

Kernel level, the batch of tests/test_gpu_xadj_mfma.py built again: thirteen atoms with 17, 1, 33, 0, 16, 2, 31, 5, 15, 32, 9, 29
and 30 in-edges (one N tile and its edge, two N tiles, up to eight M tiles with one output tile per wave and more with two, the
largest matrix group, the first group of the per-edge body, an atom without edges and one without triplets), the edges of an atom
scattered over the edge order, 85 % of the pairs c -> a <- b present, one expand row without triplets; four dSm and four x arrays.
  * against float64 (cpu_kernels.bil_dy_multi on the same fp32 operands), nb = 1, 2, 3, 4: an element is a sum of K = 64 nb
    products and is held to  |dY - dY64| <= 2 * 2^-24 * K * sum |dSm| |x| + K * 2^-149  (the bound derived in the docstring of
    tests/test_gpu_xadj_mfma.py, applied to this sum); gn_bil_dy_multi_f32 is held to the same bound, so the two launches differ
    by at most twice it.  The fraction of the bound reached and whether the launches are bit-equal (same K order: they may be)
    are printed;
  * coverage: dY comes from `empty`, which the harness fills with NaN — a row nobody wrote fails the bound;
  * rows of the dSm blocks scaled by 1e-20 and 1e+20: the bound is linear in dSm, nothing non-finite appears (the padding of
    the dense product reaches LDS nobody wrote, and outputs nobody stores);
  * bitwise: two runs; a captured replay; every atom run alone (edges renumbered from 0, same relative order); the static bounds
    max_rows = 48 and 91 against the exact 33; the 33-group against the per-edge launch; the whole result with the switch off.
Model level (2 molecules x 8 atoms, one block, the case of tests/test_gpu_bil_up.py): the switch on and off against the
float64 oracle at that file's bars; the padded captured replay == eager bit for bit with the switch on."""
import pytest
import torch

import cpu_kernels as CK
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd.graph import SegmentPlan
from gemnet_pytorch_amd.padded import PaddedGraphRunner
from redzone import put, redzone  # noqa: F401  (autouse: every test of this module runs under the red-zone harness)
from test_gpu_bil_up import t_case  # noqa: F401  (the module-scoped model fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, C, NB = 7, 64, 4
SIZES = (17, 1, 33, 0, 16, 2, 31, 5, 15, 32, 9, 29, 30)        # in-edges of atom 0, 1, ...
BARE_ROW_OF = 0                                         # the atom (17 edges) one of whose expand rows loses every triplet


def f32(ts):
    return [put(t.to(torch.float32)) for t in ts]


class Batch:
    def __init__(self):
        g = torch.Generator().manual_seed(1405)
        A = len(SIZES)
        tgt = torch.repeat_interleave(torch.arange(A), torch.tensor(SIZES))
        tgt = tgt[torch.randperm(tgt.shape[0], generator=g)]
        E = int(tgt.shape[0])
        self.edges = [torch.nonzero(tgt == a).flatten().tolist() for a in range(A)]
        self.bare = self.edges[BARE_ROW_OF][3]
        red, exp = [], []
        for es in self.edges:
            for r in es:
                for x in es:
                    if r != x and x != self.bare and float(torch.rand((), generator=g)) < 0.85:
                        red.append(r), exp.append(x)
        red, exp = torch.tensor(red, dtype=torch.int64), torch.tensor(exp, dtype=torch.int64)
        order = torch.argsort(red, stable=True)
        self.red, self.exp, self.tgt, self.A, self.E = red[order], exp[order], tgt, A, E
        self.T = int(red.shape[0])
        self.D = [torch.randn(E, S, C, generator=g, dtype=torch.float64).float() for _ in range(NB)]
        self.X = [torch.randn(E, C, generator=g, dtype=torch.float64).float() for _ in range(NB)]
        self.cpu = SegmentPlan(self.red, self.exp, E, E)
        self.plain = SegmentPlan(self.red.to(DEV), self.exp.to(DEV), E, E)      # no row groups: the per-edge launch
        self.n_trip = torch.bincount(self.exp, minlength=E)

    def plan(self, max_rows=None):
        sp = SegmentPlan(self.red.to(DEV), self.exp.to(DEV), self.E, self.E)
        sp.set_row_groups(self.tgt.to(DEV), self.A, max_rows=max_rows)
        return sp

    def alone(self, a):
        """Atom a as a problem of its own: its edges renumbered 0.. in the same order, its triplets in the same order."""
        es = torch.tensor(self.edges[a], dtype=torch.int64)
        local = torch.full((self.E,), -1, dtype=torch.int64)
        local[es] = torch.arange(es.shape[0])
        mine = torch.nonzero(self.tgt[self.red] == a).flatten()
        sp = SegmentPlan(local[self.red[mine]].to(DEV), local[self.exp[mine]].to(DEV), len(es), len(es))
        sp.set_row_groups(torch.zeros(len(es), dtype=torch.int64, device=DEV), 1)
        return sp, mine, es

    def bound(self, D, nb):
        mag = CK.bil_dy_multi([d.double().abs() for d in D[:nb]], [x.double().abs() for x in self.X[:nb]], self.cpu)
        k = 64.0 * nb
        return 2 * 2.0 ** -24 * k * mag + k * 2.0 ** -149

    def ref(self, D, nb):
        return CK.bil_dy_multi([d.double() for d in D[:nb]], [x.double() for x in self.X[:nb]], self.cpu)

    def rows_of(self, n):
        """The triplets whose edges end in the atom of n in-edges."""
        return torch.nonzero(self.tgt[self.red] == SIZES.index(n)).flatten().to(DEV)


_B = {}


def batch():
    if not _B:
        b = Batch()
        b.sp = b.plan()
        b.got = K.bil_dy_multi(f32(b.D), f32(b.X), b.sp)
        b.old = K.bil_dy_multi(f32(b.D), f32(b.X), b.plain)
        _B["b"] = b
    return _B["b"]


def test_the_batch_holds_what_it_is_for():
    b = batch()
    assert K.USE_DY_ATOMS
    assert {1, 2, 15, 16, 17, 29, 30, 31, 32, 33, 0} <= set(SIZES) and b.sp.groups[4] == 33
    for es in b.edges:            # scattered over the edge order
        assert len(es) < 2 or es[-1] - es[0] + 1 > len(es)
    assert int(b.n_trip[b.bare]) == 0 and int(b.n_trip[b.edges[1][0]]) == 0
    full = sum(n * (n - 1) for n in SIZES)
    assert 0.7 * full < b.T < 0.95 * full                                   # incomplete pair sets
    ent_off, ent_t, ent_bc = b.sp.group_entries
    assert sorted(ent_t.tolist()) == list(range(b.T))
    assert b.plain.groups is None


def _check(b, D, nb, tag, got=None, old=None):
    got = K.bil_dy_multi(f32(D[:nb]), f32(b.X[:nb]), b.sp) if got is None else got
    old = K.bil_dy_multi(f32(D[:nb]), f32(b.X[:nb]), b.plain) if old is None else old
    ref, bound = b.ref(D, nb), b.bound(D, nb)
    assert got.shape == (b.T, S)
    assert torch.isfinite(got).all()                            # (every row written: `empty` is NaN under the harness)
    err = (got.double().cpu() - ref).abs()
    err_o = (old.double().cpu() - ref).abs()
    diff = (got.double().cpu() - old.double().cpu()).abs()
    frac = lambda e, m=1: float((e / (m * bound).clamp_min(1e-300)).max())      # noqa: E731
    print(f"{tag}, nb = {nb}: max err {float(err.max()):.3e} = {frac(err):.3f} of the bound (per-edge launch {frac(err_o):.3f}); "
          f"against the per-edge launch {float(diff.max()):.3e} = {frac(diff, 2):.3f} of twice the bound; "
          f"bit-equal to it: {torch.equal(got, old)}")
    assert (err <= bound).all() and (err_o <= bound).all() and (diff <= 2 * bound).all()


@pytest.mark.parametrize("nb", [1, 2, 3, 4])
def test_against_float64_and_the_per_edge_launch(nb):
    b = batch()
    if nb == NB:
        _check(b, b.D, nb, "mixed groups", b.got, b.old)
    else:
        _check(b, b.D, nb, "mixed groups")


def test_rows_of_dSm_scaled_by_1e_minus_20_and_1e_plus_20():
    b = batch()
    scale = torch.ones(b.E, 1, 1)
    scale[0::3], scale[1::3] = 1e-20, 1e20
    _check(b, [(d * scale).contiguous() for d in b.D], NB, "rows x 1e-20 / 1e+20")


def test_two_runs_and_a_captured_replay_give_the_same_bits():
    b = batch()
    D, X = f32(b.D), f32(b.X)
    assert torch.equal(K.bil_dy_multi(D, X, b.sp), b.got)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.bil_dy_multi(D, X, b.sp)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = K.bil_dy_multi(D, X, b.sp)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, b.got)


def test_an_atom_alone_gives_the_bits_it_gives_inside_the_batch():
    b = batch()
    seen = 0
    for a, n in enumerate(SIZES):
        if n < 2:                        # the atom without edges and the 1-group: no triplets, nothing to compare
            continue
        sp, mine, es = b.alone(a)
        assert sp.groups[4] == n and mine.numel() > 0
        got = K.bil_dy_multi(f32([d[es] for d in b.D]), f32([x[es] for x in b.X]), sp)
        assert torch.equal(got, b.got[mine.to(DEV)]), (a, n)
        seen += 1
    assert seen == len(SIZES) - 2


@pytest.mark.parametrize("max_rows", [48, 91])
def test_a_static_row_bound_does_not_change_a_bit(max_rows):
    b = batch()
    sp = b.plan(max_rows=max_rows)
    assert sp.groups[4] == max_rows
    assert torch.equal(K.bil_dy_multi(f32(b.D), f32(b.X), sp), b.got)


def test_the_group_of_33_rows_keeps_the_per_edge_launchs_bits():
    b = batch()
    rows = b.rows_of(33)
    assert rows.numel() > 0 and torch.equal(b.got[rows], b.old[rows])


def test_with_the_switch_off_the_result_is_the_per_edge_launchs(monkeypatch):
    b = batch()
    monkeypatch.setattr(K, "USE_DY_ATOMS", False)
    assert torch.equal(K.bil_dy_multi(f32(b.D), f32(b.X), b.plan()), b.old)


# ------------------------------------------------------------------------------------------------------------------ model
@pytest.mark.parametrize("on", [True, False])
def test_model_matches_the_float64_oracle_with_the_switch_on_and_off(t_case, on, monkeypatch):  # noqa: F811
    model, inputs, E_ref, F_ref = t_case
    monkeypatch.setattr(K, "USE_DY_ATOMS", on)
    inputs = {k: v for k, v in inputs.items() if k != "_plan"}             # a plan of its own
    E, F = model(inputs)
    torch.cuda.synchronize()
    f_mae = float((F.detach().double().cpu() - F_ref).abs().mean())
    f_mean = float(F_ref.abs().mean())
    e_err = float((E.detach().double().cpu().reshape(E_ref.shape) - E_ref).abs().max())
    print(f"GEMNET_DY_ATOMS={int(on)}: force MAE {f_mae:.3e} at mean |F_ref| {f_mean:.3e}, energy err {e_err:.3e} "
          f"(max |E_ref| {float(E_ref.abs().max()):.3f})")
    assert f_mae <= 1e-5 * f_mean
    assert e_err <= 2e-5 * max(1.0, float(E_ref.abs().max()))


def test_padded_replay_equals_eager_bitwise(t_case, monkeypatch):  # noqa: F811
    model, inputs, _, _ = t_case
    monkeypatch.setattr(K, "USE_DY_ATOMS", True)
    inputs = {k: v for k, v in inputs.items() if k != "_plan"}
    inputs["R"] = inputs["R"].float()
    model.requires_grad_(False)
    try:
        E0, F0 = (t.detach().clone() for t in model(dict(inputs)))
        idx = {k: v for k, v in inputs.items() if k.startswith("id")}
        e_cap, t_cap = int(idx["id_c"].shape[0]) + 8, int(idx["id3_reduce_ca"].shape[0]) + 8
        runner = PaddedGraphRunner(model, inputs["Z"], inputs["N"], e_cap, t_cap)
        for _ in range(2):                                                    # capture, then replay
            E, F = runner(inputs["R"], idx, Z=inputs["Z"])
            torch.cuda.synchronize()
            assert torch.equal(E, E0) and torch.equal(F, F0)
    finally:
        model.requires_grad_(True)
