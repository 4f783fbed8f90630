"""-m gpu: the triplet x-adjoint per atom on the matrix cores (gn_bil_x_adjoint_atoms_f32 behind
kernels.bil_reduce_t, GEMNET_XADJ_MFMA).

Kernel level, ONE batch of thirteen atoms: groups of 1, 2, 15, 16, 17, 31, 32 and 33 in-edges (one M tile, its edge, two tiles,
two K chunks of 16 reduce edges, the largest matrix group, the first group of the scalar body), of 29 and 30 (the last group
whose LDS image holds all of K, the first that takes two chunks), two more of 5 and 9, and an atom without edges; the edges of
an atom scattered over the edge order; 85 % of the pairs c -> a <- b present, every
triplet of one expand row of the 17-group removed (a row without triplets; the lone edge of the 1-group is another).
  * against float64 (cpu_kernels.bil_reduce_t on the same fp32 operands): a row j whose sum has K_j = 7 x (triplets of j)
    terms is held to  |dx - dx64| <= 2 * 2^-24 * K_j * sum |Y| |dSm|  per element (+ K_j 2^-149 for terms that underflow).
    fp32 products and partial sums round once each (u = 2^-24): a sum of K terms in ANY order carries at most
    ((1 + u)^K - 1) sum |terms| ~ K u sum |terms| (the fused multiply-add of the scalar kernels and of the f32 matrix
    instruction round less often, never more); the factor 2 covers the second-order terms and an implementation that rounds
    the products on their own.  The zeros that pad the dense product add nothing.  A row without triplets is exactly zero;
  * against the ungrouped kernel (gn_bil_reduce_t_f32), which is held to the same bound: the two differ by at most twice it;
  * with rows of dSm scaled by 1e-20 and 1e+20 (the bound is linear in dSm; no zero of the padding may meet an Inf or NaN);
  * bitwise: two runs; a captured replay; every atom's rows when the atom is run alone (its edges renumbered from 0 in the same
    relative order); the static bounds max_rows = 48 and 91 against the exact 33; the 33-group with GEMNET_XADJ_MFMA=0.
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
S, C = 7, 64
SIZES = (17, 1, 33, 0, 16, 2, 31, 5, 15, 32, 9, 29, 30)        # in-edges of atom 0, 1, ...
BARE_ROW_OF = 0                                         # the atom (17 edges) one of whose expand rows loses every triplet


def f32(t):
    return put(t.to(torch.float32))


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
        self.Y = torch.randn(red.shape[0], S, generator=g, dtype=torch.float64).float()
        self.D = torch.randn(E, S, C, generator=g, dtype=torch.float64).float()
        self.cpu = SegmentPlan(self.red, self.exp, E, E)
        self.plain = SegmentPlan(self.red.to(DEV), self.exp.to(DEV), E, E)
        self.n_trip = torch.bincount(self.exp, minlength=E)

    def plan(self, max_rows=None):
        sp = SegmentPlan(self.red.to(DEV), self.exp.to(DEV), self.E, self.E)
        sp.set_row_groups(self.tgt.to(DEV), self.A, max_rows=max_rows)
        return sp

    def alone(self, a):
        """Atom a as a problem of its own: its edges renumbered 0.. in the same order, its triplets in the same order."""
        es = torch.tensor(self.edges[a])
        local = torch.full((self.E,), -1, dtype=torch.int64)
        local[es] = torch.arange(es.shape[0])
        mine = torch.nonzero(self.tgt[self.red] == a).flatten()
        sp = SegmentPlan(local[self.red[mine]].to(DEV), local[self.exp[mine]].to(DEV), len(es), len(es))
        sp.set_row_groups(torch.zeros(len(es), dtype=torch.int64, device=DEV), 1)
        return sp, self.Y[mine].contiguous(), self.D[es].contiguous(), es

    def bound(self, D):
        mag = CK.bil_reduce_t(self.Y.double().abs(), D.double().abs(), self.cpu)
        k = (S * self.n_trip).double().unsqueeze(1)
        return 2 * 2.0 ** -24 * k * mag + k * 2.0 ** -149


_B = {}


def batch():
    if not _B:
        b = Batch()
        b.sp = b.plan()
        b.got = K.bil_reduce_t(f32(b.Y), f32(b.D), b.sp)
        b.ref = CK.bil_reduce_t(b.Y.double(), b.D.double(), b.cpu)          # float64, once
        _B["b"] = b
    return _B["b"]


def test_the_batch_holds_what_it_is_for():
    b = batch()
    assert K.USE_XADJ_MFMA
    assert {1, 2, 15, 16, 17, 29, 30, 31, 32, 33, 0} <= set(SIZES) and b.sp.groups[4] == 33
    for es in b.edges:            # scattered over the edge order
        assert len(es) < 2 or es[-1] - es[0] + 1 > len(es)
    assert int(b.n_trip[b.bare]) == 0 and int(b.n_trip[b.edges[1][0]]) == 0
    full = sum(n * (n - 1) for n in SIZES)
    assert 0.7 * full < b.red.shape[0] < 0.95 * full                        # incomplete pair sets
    ent_off, ent_t, ent_bc = b.sp.group_entries
    assert sorted(ent_t.tolist()) == list(range(b.red.shape[0]))


def _check(b, got, D, tag):
    ref = CK.bil_reduce_t(b.Y.double(), D.double(), b.cpu) if D is not b.D else b.ref
    bound = b.bound(D)
    assert torch.isfinite(got).all()
    err = (got.double().cpu() - ref).abs()
    plain = K.bil_reduce_t(f32(b.Y), f32(D), b.plain)
    err_p = (plain.double().cpu() - ref).abs()
    diff = (got.double().cpu() - plain.double().cpu()).abs()
    frac = lambda e, m=1: float((e / (m * bound).clamp_min(1e-300)).max())      # noqa: E731
    print(f"{tag}: max err {float(err.max()):.3e} = {frac(err):.3f} of the bound (ungrouped kernel {frac(err_p):.3f}); "
          f"against the ungrouped kernel {float(diff.max()):.3e} = {frac(diff, 2):.3f} of twice the bound")
    assert (err <= bound).all() and (err_p <= bound).all() and (diff <= 2 * bound).all()
    empty = b.n_trip == 0
    assert float(got[empty.to(DEV)].abs().max()) == 0.0


def test_against_float64_and_the_ungrouped_kernel():
    b = batch()
    _check(b, b.got, b.D, "mixed groups")


def test_rows_of_dSm_scaled_by_1e_minus_20_and_1e_plus_20():
    b = batch()
    scale = torch.ones(b.E, 1, 1)
    scale[0::3], scale[1::3] = 1e-20, 1e20
    D = (b.D * scale).contiguous()
    _check(b, K.bil_reduce_t(f32(b.Y), f32(D), b.sp), D, "rows x 1e-20 / 1e+20")


def test_two_runs_and_a_captured_replay_give_the_same_bits():
    b = batch()
    Y, D = f32(b.Y), f32(b.D)
    assert torch.equal(K.bil_reduce_t(Y, D, b.sp), b.got)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.bil_reduce_t(Y, D, b.sp)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = K.bil_reduce_t(Y, D, b.sp)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, b.got)


def test_an_atom_alone_gives_the_bits_it_gives_inside_the_batch():
    b = batch()
    for a, n in enumerate(SIZES):
        if n == 0:
            continue
        sp, Y, D, es = b.alone(a)
        assert sp.groups[4] == n
        got = K.bil_reduce_t(f32(Y), f32(D), sp)
        assert torch.equal(got, b.got[es.to(DEV)]), (a, n)


@pytest.mark.parametrize("max_rows", [48, 91])
def test_a_static_row_bound_does_not_change_a_bit(max_rows):
    b = batch()
    sp = b.plan(max_rows=max_rows)
    assert sp.groups[4] == max_rows
    assert torch.equal(K.bil_reduce_t(f32(b.Y), f32(b.D), sp), b.got)


def test_the_group_of_33_rows_keeps_the_scalar_kernels_bits(monkeypatch):
    b = batch()
    monkeypatch.setattr(K, "USE_XADJ_MFMA", False)
    off = K.bil_reduce_t(f32(b.Y), f32(b.D), b.plan())
    es = torch.tensor(b.edges[SIZES.index(33)], device=DEV)
    assert torch.equal(off[es], b.got[es])
    others = torch.tensor(b.edges[SIZES.index(32)], device=DEV)
    assert not torch.equal(off[others], b.got[others])      # (the matrix path really ran: another order of summation)


# ------------------------------------------------------------------------------------------------------------------ model
@pytest.mark.parametrize("on", [True, False])
def test_model_matches_the_float64_oracle_with_the_switch_on_and_off(t_case, on, monkeypatch):  # noqa: F811
    model, inputs, E_ref, F_ref = t_case
    monkeypatch.setattr(K, "USE_XADJ_MFMA", on)
    inputs = {k: v for k, v in inputs.items() if k != "_plan"}             # a plan of its own: the entry list follows the switch
    E, F = model(inputs)
    torch.cuda.synchronize()
    f_mae = float((F.detach().double().cpu() - F_ref).abs().mean())
    f_mean = float(F_ref.abs().mean())
    e_err = float((E.detach().double().cpu().reshape(E_ref.shape) - E_ref).abs().max())
    print(f"GEMNET_XADJ_MFMA={int(on)}: force MAE {f_mae:.3e} at mean |F_ref| {f_mean:.3e}, energy err {e_err:.3e} "
          f"(max |E_ref| {float(E_ref.abs().max()):.3f})")
    assert f_mae <= 1e-5 * f_mean
    assert e_err <= 2e-5 * max(1.0, float(E_ref.abs().max()))


def test_padded_replay_equals_eager_bitwise(t_case, monkeypatch):  # noqa: F811
    model, inputs, _, _ = t_case
    monkeypatch.setattr(K, "USE_XADJ_MFMA", True)
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
