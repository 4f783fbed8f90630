"""The edge embedding inside the radial head launches (csrc/radial_head.hip, gn_radial_head_emb_fwd_f32 / _bwd_f32; DESIGN.md
section 19).  Kernel level: the projected outputs against `K.radial_head_fwd` (bit-equal), m0 against today's three launches
(atom-term GEMMs on the gathered rows -> small-K GEMM with both gathered adds and the activation: bit-equal), d0 against
float64 next to today's `gn_dssilu(z0)`, the adjoint against the float64 adjoint of the CPU restatement and against the old
adjoint, row independence and determinism.  Tables: the row identity in float64, the cache, and the table rows against today's
atom terms on the GPU.  Model level: the one-block 2 x 8-atom GemNet-T at the widths the path takes (128), switch on and off,
against the float64 oracle; captured replay == eager under the happens-before checker; the models that keep the old launches.
"""
import collections
import os
import re

import numpy as np
import pytest
import torch

import cpu_kernels as CK
from conftest import ROOT, SCALE_FILE
from gemnet_pytorch_amd import _lib, hbcheck, ops
from gemnet_pytorch_amd import kernels as K
from oracle import basis_oracle as B
from oracle import gemnet_oracle as GO
from oracle import index_oracle as IO
from redzone import put, redzone  # noqa: F401  (autouse: every test of this module runs under the red-zone harness)

gpu = pytest.mark.gpu
DEV = "cuda"
CUTOFF, P_ENV = 8.0, 5
NR, S, NI, NE, NZ = 6, 7, 16, 128, 93
SIZES = [1, 15, 16, 17, 33, 300]        # 16 edges per block: below, at and above one block, an odd count, 19 blocks


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_abi_declares_and_binds_both_entry_points_and_the_launchers_validate():
    with open(os.path.join(ROOT, "include", "gemnet_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name, nargs in (("gn_radial_head_emb_fwd_f32", 26), ("gn_radial_head_emb_bwd_f32", 25)):
        m = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name])
    g = torch.Generator().manual_seed(1)
    E, A = 5, 4
    R, ic, ia = torch.zeros(A, 3), torch.zeros(E, dtype=torch.int32), torch.ones(E, dtype=torch.int32)
    freq, z, nrm = torch.ones(NR), torch.ones(S, NR), torch.ones(S, NR, dtype=torch.float64)
    wcat = K.radial_head_weights(*([torch.randn(NI, NR, generator=g) for _ in range(3)] + [torch.randn(S, NR, NI, generator=g)]))
    zrow, T = torch.zeros(A, dtype=torch.int32), torch.zeros(NZ, NE)
    Wr = torch.zeros(NR, NE)
    fwd = lambda **kw: K.radial_head_emb_fwd(R, ic, ia, freq, z, nrm, wcat, kw.get("zrow", zrow), kw.get("Tc", T), T,     # noqa: E731
                                             kw.get("Wr", Wr), CUTOFF, P_ENV)
    with pytest.raises(ValueError):
        fwd(Wr=torch.zeros(NR, 64))                 # another edge width
    with pytest.raises(ValueError):
        fwd(Tc=torch.zeros(NZ, 64))                 # another atom width
    with pytest.raises(ValueError):
        fwd(zrow=zrow.long())
    with pytest.raises(ValueError):
        fwd(Tc=torch.zeros(NZ * NE + 1)[1:].view(NZ, NE))     # rows not 16-byte aligned
    with pytest.raises(RuntimeError):               # no CPU fallback
        fwd()
    d0, ga = torch.zeros(E, NE), torch.zeros(E, NE)
    bwd = lambda ga, d0, Wr=Wr: K.radial_head_emb_bwd(None, None, None, None, None, ga, None, d0, Wr, R, ic, ia, freq, z, nrm,   # noqa: E731
                                                      wcat, CUTOFF, P_ENV)
    with pytest.raises(ValueError):
        bwd(torch.zeros(E, 64), d0)
    with pytest.raises(ValueError):
        bwd(torch.zeros(E * NE + 1)[1:].view(E, NE), d0)      # an unaligned (E,128) cotangent
    with pytest.raises(ValueError):
        bwd(ga, torch.zeros(E * NE + 3)[3:].view(E, NE))
    with pytest.raises(ValueError):
        bwd(ga, None)
    with pytest.raises(ValueError):
        bwd(ga, d0, torch.zeros(NE, NR))
    with pytest.raises(RuntimeError):
        bwd(ga, d0)


def test_table_rows_are_the_atom_terms_exactly_in_float64():
    g = torch.Generator().manual_seed(2)
    emb = torch.rand(NZ, NE, generator=g, dtype=torch.float64) * 2 - 1
    Wc = torch.randn(NE, NE, generator=g, dtype=torch.float64)
    Z = torch.cat([torch.tensor([0, 92, 5, 5, 92]), torch.randint(0, NZ, (35,), generator=g)])
    rows = lambda x: (x[:, None, :] * Wc[None]).sum(-1)        # noqa: E731  x W_c^T, one row at a time
    assert torch.equal(rows(emb)[Z], rows(emb[Z]))


def test_tables_are_cached_per_weight_version(monkeypatch):
    calls = []

    def maker(emb_weight, W, A):
        calls.append(1)
        return emb_weight.detach() @ W.detach()[:, :A].t(), emb_weight.detach() @ W.detach()[:, A:2 * A].t(), \
            W.detach()[:, 2 * A:].t().contiguous()
    monkeypatch.setattr(ops, "_make_atom_tables", maker)
    emb = torch.nn.Parameter(torch.randn(NZ, NE))
    W = torch.nn.Parameter(torch.randn(NE, 2 * NE + NR))
    with ops.weight_cache({}):
        t0 = ops.atom_term_tables(emb, W, NE)
        t1 = ops.atom_term_tables(emb, W, NE)
        assert len(calls) == 1 and all(a is b for a, b in zip(t0, t1))
        with torch.no_grad():
            W.mul_(2.0)                                  # an in-place update of the Dense weight
        t2 = ops.atom_term_tables(emb, W, NE)
        assert len(calls) == 2 and torch.equal(t2[0], emb.detach() @ W.detach()[:, :NE].t())
        with torch.no_grad():
            emb.add_(1.0)                                # ... and of the embedding
        t3 = ops.atom_term_tables(emb, W, NE)
        assert len(calls) == 3 and torch.equal(t3[1], emb.detach() @ W.detach()[:, NE:2 * NE].t())
        ops.atom_term_tables(emb, W, NE)
        assert len(calls) == 3


# ------------------------------------------------------------------------------------------------------------- kernels
class Case:
    """40 atoms in a 6 A box (some distances exceed the cutoff) whose elements include table rows 0 and 92 and repeat, 300
    random edges, random weights and cotangents; the float64 references are computed once."""

    def __init__(self):
        g = torch.Generator().manual_seed(34)
        n_atoms, n_edges = 40, 300
        self.R = torch.rand(n_atoms, 3, generator=g, dtype=torch.float64) * 6.0
        ic = torch.randint(0, n_atoms, (n_edges,), generator=g)
        ia = (ic + 1 + torch.randint(0, n_atoms - 1, (n_edges,), generator=g)) % n_atoms    # != ic
        self.ic, self.ia = ic.int(), ia.int()
        self.zrow = torch.cat([torch.tensor([0, 92, 7, 7, 92, 0]), torch.randint(0, NZ, (n_atoms - 6,), generator=g)]).int()
        self.z, self.nrm = torch.tensor(B.jn_zeros(S, NR)), torch.tensor(B.sph_bessel_normalizer(S, NR))
        self.freq = torch.arange(1, NR + 1, dtype=torch.float64) * np.pi
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()          # noqa: E731
        self.W = [rn(NI, NR), rn(NI, NR), rn(NI, NR), rn(S, NR, NI)]
        self.emb = (torch.rand(NZ, NE, generator=g, dtype=torch.float64) * 2 - 1).float() * 3 ** 0.5
        self.W_emb = rn(NE, 2 * NE + NR) / (2 * NE + NR) ** 0.5 * 2.0       # z0 of order one, both signs
        self.g = dict(rbf=rn(n_edges, NR), rbf3=rn(n_edges, NI), rbf_h=rn(n_edges, NI), rbf_out=rn(n_edges, NI),
                      rbf_W1=rn(n_edges, S, NI), ga=rn(n_edges, NE), gb=rn(n_edges, NE))
        self.dev = dict(R=put(self.R.float()), ic=put(self.ic), ia=put(self.ia), freq=put(self.freq.float()),
                        z=put(self.z.float()), nrm=put(self.nrm), wcat=put(K.radial_head_weights(*self.W)),
                        zrow=put(self.zrow), emb=put(self.emb), W_emb=put(self.W_emb))
        d = self.dev
        # the tables by the maker the model uses; today's atom terms from the gathered rows by the same launcher
        self.T_c, self.T_a, self.W_r = ops._make_atom_tables(d["emb"], d["W_emb"], NE)
        h = K.gather(d["emb"], d["zrow"])
        self.g1 = K.gemm(h, d["W_emb"][:, :NE].contiguous())
        self.g2 = K.gemm(h, d["W_emb"][:, NE:2 * NE].contiguous())
        self._fwd = {}

    def fwd(self, E, want_rbf=True):
        d = self.dev
        return K.radial_head_emb_fwd(d["R"], d["ic"][:E], d["ia"][:E], d["freq"], d["z"], d["nrm"], d["wcat"], d["zrow"],
                                     self.T_c, self.T_a, self.W_r, CUTOFF, P_ENV, want_rbf=want_rbf)

    def old_fwd(self, E):
        d = self.dev
        return K.radial_head_fwd(d["R"], d["ic"][:E], d["ia"][:E], d["freq"], d["z"], d["nrm"], d["wcat"], CUTOFF, P_ENV)

    def today(self, E, rbf):
        """m0, z0, ssilu'(z0) of today's launches: the small-K GEMM with both gathered atom terms and the activation."""
        d = self.dev
        m, z0 = K.gemm(rbf, d["W_emb"][:, 2 * NE:], act=True, pre_out=True, gadd1=self.g1, gidx1=d["ic"][:E], gadd2=self.g2,
                       gidx2=d["ia"][:E])
        return m, z0, K.ssilu(z0, 1)

    def ref64(self, E, rbf):
        """float64 m0 / d0 from the fp32 operands the launches read (the kernel's own rbf values)."""
        W = self.W_emb.double()
        h = self.emb.double()[self.zrow.long()]
        z0 = rbf.double().cpu() @ W[:, 2 * NE:].t() + (h @ W[:, :NE].t())[self.ic[:E].long()] + (h @ W[:, NE:2 * NE].t())[self.ia[:E].long()]
        s = torch.sigmoid(z0)
        return z0 * s / 0.6, s * (1 + z0 * (1 - s)) / 0.6

    def bwd(self, E, names, d0):
        d = self.dev
        gs = [put(self.g[n][:E]) if n in names else None for n in ("rbf", "rbf3", "rbf_h", "rbf_out", "rbf_W1", "ga", "gb")]
        return K.radial_head_emb_bwd(*gs, d0, self.W_r, d["R"], d["ic"][:E], d["ia"][:E], d["freq"], d["z"], d["nrm"], d["wcat"],
                                     CUTOFF, P_ENV)

    def old_bwd(self, E, names):
        d = self.dev
        gs = [put(self.g[n][:E]) if n in names else None for n in ("rbf", "rbf3", "rbf_h", "rbf_out", "rbf_W1")]
        return K.radial_head_bwd(*gs, d["R"], d["ic"][:E], d["ia"][:E], d["freq"], d["z"], d["nrm"], d["wcat"], CUTOFF, P_ENV)

    def bwd_ref(self, E, names, d0):
        """CK.edge_basis_bwd on the cotangents composed in float64 (g_rbf_total, g_rad), the embedding term included, and
        the bound 2^-23 sum_i |g d0 W_r| of that term's fp32 sum carried through the rbf derivative."""
        W3, Wh, Wo, Wc = [w.double() for w in self.W]
        g = {n: self.g[n][:E].double() for n in names}
        terms = [g[n] @ W for n, W in (("rbf3", W3), ("rbf_h", Wh), ("rbf_out", Wo)) if n in g]
        if "rbf" in g:
            terms.append(g["rbf"])
        extra = torch.zeros(E, 1, dtype=torch.float64)
        if "ga" in g or "gb" in g:
            t = sum(g[n] for n in ("ga", "gb") if n in g) * d0.double().cpu()
            Wr = self.W_emb.double()[:, 2 * NE:]                   # (128, NR)
            terms.append(t @ Wr)
            Rd = self.R.float().double()
            D = torch.sqrt(((Rd[self.ia[:E].long()] - Rd[self.ic[:E].long()]) ** 2).sum(1))
            drbf = CK.bessel_rbf(D, self.freq.float().double(), CUTOFF, P_ENV, 1, 0)
            extra = (2.0 ** -23 * (t.abs() @ Wr.abs()) * drbf.abs()).sum(1, keepdim=True)
        g_rbf = sum(terms) if terms else None
        g_rad = torch.einsum("sri,esi->esr", Wc, g["rbf_W1"]) if "rbf_W1" in g else None
        if g_rbf is None and g_rad is None:
            return torch.zeros(E, 3, dtype=torch.float64), extra
        return CK.edge_basis_bwd(None, g_rbf, g_rad, self.R.float().double(), self.ic[:E], self.ia[:E], self.freq.float().double(),
                                 self.z.float(), self.nrm, CUTOFF, P_ENV), extra


@pytest.fixture(scope="module")
def case():
    return Case()


@gpu
def test_table_rows_equal_todays_atom_terms_bitwise(case):
    zr = case.dev["zrow"].long()
    assert set(case.zrow.tolist()) >= {0, 92} and len(set(case.zrow.tolist())) < len(case.zrow)
    assert torch.equal(case.T_c[zr], case.g1) and torch.equal(case.T_a[zr], case.g2)
    assert case.T_c.shape == (NZ, NE) and case.W_r.shape == (NR, NE) and case.W_r.is_contiguous()
    assert torch.equal(case.W_r, case.dev["W_emb"][:, 2 * NE:].t())


@gpu
@pytest.mark.parametrize("E", SIZES)
def test_forward_projections_and_m0_are_bit_equal_and_d0_meets_the_float64_bar(case, E):
    m0, d0, rbf3, rbf_h, rbf_out, rbf_W1, rbf = case.fwd(E)
    old = case.old_fwd(E)
    for new, ref in zip((rbf, rbf3, rbf_h, rbf_out, rbf_W1), old):
        assert torch.equal(new, ref)
    m_t, z_t, d_t = case.today(E, old[0])
    m64, d64 = case.ref64(E, old[0])
    err = lambda x, r: float((x.double().cpu() - r).abs().max())        # noqa: E731
    e_m, e_mt, e_d, e_dt = err(m0, m64), err(m_t, m64), err(d0, d64), err(d_t, d64)
    print(f"E={E}: max err vs float64  m0 new {e_m:.3e} today {e_mt:.3e}   d0 new {e_d:.3e} today {e_dt:.3e}   "
          f"m0 bit-equal {torch.equal(m0, m_t)}  max |z0| {float(z_t.abs().max()):.2f}")
    assert m0.shape == (E, NE) and d0.shape == (E, NE) and torch.isfinite(m0).all() and torch.isfinite(d0).all()
    assert torch.equal(m0, m_t)                  # the order of the small-K kernel and its epilogue is reproduced
    # d0 comes from the sigmoid of the same z0 by gn_ssilu_pair, today's from gn_dssilu: the same number of fp32 roundings
    # in another order
    assert e_m <= 2.0 * e_mt and e_d <= 2.0 * e_dt
    # without the rbf output nothing else changes
    again = case.fwd(E, want_rbf=False)
    assert again[6] is None and all(torch.equal(a, b) for a, b in zip(again[:6], (m0, d0, rbf3, rbf_h, rbf_out, rbf_W1)))


@gpu
def test_rows_do_not_depend_on_other_edges_and_runs_repeat_bitwise(case):
    full = case.fwd(300)
    for E in (17, 33):
        for a, b in zip(full, case.fwd(E)):
            assert torch.equal(a[:E], b)
    for a, b in zip(full, case.fwd(300)):
        assert torch.equal(a, b)
    names = ("rbf3", "rbf_h", "rbf_out", "rbf_W1", "ga", "gb")
    Wf = case.bwd(300, names, full[1])
    for E in (17, 33):
        assert torch.equal(Wf[:E], case.bwd(E, names, full[1][:E].contiguous()))
    assert torch.equal(Wf, case.bwd(300, names, full[1]))


OLD = ("rbf", "rbf3", "rbf_h", "rbf_out", "rbf_W1")
# cotangent sets: ga only / gb only / both / neither, and each of the five old cotangents absent at least once
SETS = [OLD + ("ga",), OLD + ("gb",), OLD + ("ga", "gb"), OLD, ("ga",), ("rbf3", "rbf_W1", "ga", "gb"),
        ("rbf", "rbf_h", "rbf_out", "gb"), ("rbf_h", "rbf_out", "rbf_W1", "ga")]


@gpu
@pytest.mark.parametrize("E", SIZES)
def test_adjoint_matches_the_float64_adjoint_and_the_old_kernel(case, E):
    d0 = case.fwd(E)[1]
    for names in SETS:
        W = case.bwd(E, names, d0)
        ref, extra = case.bwd_ref(E, names, d0)
        err = (W.double().cpu() - ref).abs()
        atol = 2e-4 * float(ref.abs().max())          # the bar of test_gpu_radial_head.py for the old adjoint
        print(f"E={E} {'+'.join(names)}: max err {float(err.max()):.3e}, atol {atol:.3e}, added bound {float(extra.max()):.3e}")
        assert float(ref.abs().max()) > 0 and torch.isfinite(W).all()
        assert (err <= atol + 2e-4 * ref.abs() + extra).all()
        if "ga" not in names and "gb" not in names:
            assert torch.equal(W, case.old_bwd(E, names))
    # today's launches: the adjoint GEMM of the Dense ((ga + gb) ssilu'(z0) W_r, added onto g_rbf) + the old kernel
    d = case.dev
    ga, gb, g_rbf = put(case.g["ga"][:E]), put(case.g["gb"][:E]), put(case.g["rbf"][:E])
    z0 = case.today(E, case.old_fwd(E)[0])[1]
    g_tot = K.gemm(ga + gb, case.W_r, a_dact_pre=z0, res2=g_rbf)
    W_today = K.radial_head_bwd(g_tot, None, None, None, None, d["R"], d["ic"][:E], d["ia"][:E], d["freq"], d["z"], d["nrm"],
                                d["wcat"], CUTOFF, P_ENV)
    W_new = case.bwd(E, ("rbf", "ga", "gb"), d0)
    ref, extra = case.bwd_ref(E, ("rbf", "ga", "gb"), d0)
    e_new, e_today = float((W_new.double().cpu() - ref).abs().max()), float((W_today.double().cpu() - ref).abs().max())
    print(f"E={E}: rbf+ga+gb max err new {e_new:.3e}, today's GEMM + old kernel {e_today:.3e} (max |W| {float(ref.abs().max()):.3e})")
    # all-null: zeros
    assert torch.equal(case.bwd(E, (), None), torch.zeros(E, 3, device=DEV))


# --------------------------------------------------------------------------------------------------------------- model
T_CFG = dict(num_spherical=7, num_radial=6, num_blocks=1, emb_size_atom=128, emb_size_edge=128, emb_size_trip=64,
             emb_size_quad=32, emb_size_rbf=16, emb_size_cbf=16, emb_size_sbf=32, emb_size_bil_trip=64, emb_size_bil_quad=32,
             num_before_skip=1, num_after_skip=1, num_concat=1, num_atom=2, triplets_only=True)


class Counter:
    """A tracer for `_lib.TRACE` that counts the C-ABI calls by name."""

    def __init__(self):
        self.names = collections.Counter()

    def touch(self, t):
        pass

    def note(self, reads=(), writes=()):
        pass

    def proxy(self, lib):
        outer = self

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(lib, name)

                def call(*args):
                    outer.names[name] += 1
                    return fn(*args)
                return call
        return Proxy()


def _count(model, inputs, redzone):        # noqa: F811
    c = Counter()
    with redzone.untraced():
        _lib.TRACE = c
        try:
            E, F = model(inputs)
            torch.cuda.synchronize()
        finally:
            _lib.TRACE = None
    return E.detach(), F.detach(), c.names


def _build(cfg, params):
    from gemnet_pytorch_amd.model.gemnet import GemNet
    model = GemNet(**cfg, scale_file=SCALE_FILE)
    model.load_state_dict(GO.expand_to_reference_state_dict({k: v.float() for k, v in params.items()}))
    return model.to(DEV).eval()


def _molecules():
    from gemnet_pytorch_amd.synthetic import make_molecule
    sizes = [8, 8]
    mols = [make_molecule(n, 200 + i) for i, n in enumerate(sizes)]
    R, Z = np.concatenate([m["R"] for m in mols]), np.concatenate([m["Z"] for m in mols])
    idx = IO.build_indices(R, np.array(sizes), 5.0, 10.0, True)
    inputs = {k: torch.tensor(v) for k, v in idx.items()}
    inputs.update(Z=torch.tensor(Z).long(), R=torch.tensor(R), N=torch.tensor(sizes))
    return inputs


@pytest.fixture(scope="module")
def t_case():
    inputs = _molecules()
    params = GO.make_params(T_CFG, 1, GO.load_scale_factors(SCALE_FILE))
    E_ref, F_ref = GO.forward(T_CFG, params, inputs)          # float64 oracle, once
    return _build(T_CFG, params), {k: v.to(DEV) for k, v in inputs.items()}, E_ref.detach().double(), F_ref.detach().double()


NEW = ("gn_radial_head_emb_fwd_f32", "gn_radial_head_emb_bwd_f32")
OLD_HEAD = ("gn_radial_head_fwd_f32", "gn_radial_head_bwd_f32")


@gpu
def test_model_meets_the_oracle_bar_with_the_switch_on_and_off(t_case, monkeypatch, redzone):    # noqa: F811
    model, inputs, E_ref, F_ref = t_case
    res = {}
    for on in (False, True):
        monkeypatch.setattr(ops, "USE_RADIAL_EMB", on)
        model(inputs)                          # (fills the weight cache: the tables are built here, once)
        builds = ops.ATOM_TABLE_BUILDS
        E, F, names = _count(model, inputs, redzone)
        assert ops.ATOM_TABLE_BUILDS == builds
        assert all(names[n] == (1 if on else 0) for n in NEW) and all(names[n] == (0 if on else 1) for n in OLD_HEAD)
        f_mae = float((F.double().cpu() - F_ref).abs().mean())
        e_err = float((E.double().cpu().reshape(E_ref.shape) - E_ref).abs().max())
        res[on] = (e_err, f_mae, names["gn_gemm_f32_cfg"],
                   sum(v for k, v in names.items() if k not in ("gn_error_string", "gn_abi_version")))
        print(f"GEMNET_RADIAL_EMB={int(on)}: energy err {e_err:.3e}, force MAE {f_mae:.3e} (mean |F_ref| {float(F_ref.abs().mean()):.3e}), "
              f"{res[on][3]} library launches, {res[on][2]} of them GEMMs")
        assert f_mae <= 1e-5 * max(1.0, float(F_ref.abs().mean())) and e_err <= 2e-5 * max(1.0, float(E_ref.abs().max()))
    assert res[True][0] <= 1.5 * res[False][0] and res[True][1] <= 1.5 * res[False][1]
    assert res[True][2] == res[False][2] - 4       # two atom-term GEMMs, the K = 6 GEMM and its adjoint GEMM are gone


@gpu
def test_captured_replay_equals_eager_bitwise_and_is_ordered(t_case, monkeypatch, redzone):  # noqa: F811
    model, inputs, _, _ = t_case
    monkeypatch.setattr(ops, "USE_RADIAL_EMB", True)
    model.requires_grad_(False)
    try:
        E0, F0 = (t.detach().clone() for t in model(inputs))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(inputs)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            with redzone.untraced(), hbcheck.record() as rec:      # the recorder takes the harness's tracer slot
                Eg, Fg = model(inputs)
        launched = [o.name for o in rec.ops]
        assert sum(n.startswith(NEW[0]) for n in launched) == 1 and sum(n.startswith(NEW[1]) for n in launched) == 1
        races, summary = rec.races(), rec.summary()
        print(rec.format(races))
        assert not races and summary["unresolved_pointers"] == 0 and summary["unrecorded_nodes"] == 0
        for _ in range(5):
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(Eg, E0) and torch.equal(Fg, F0)
    finally:
        model.requires_grad_(True)


@gpu
def test_other_models_keep_the_old_launches(t_case, monkeypatch, redzone):     # noqa: F811
    import pbc_common as P
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder
    monkeypatch.setattr(ops, "USE_RADIAL_EMB", True)
    model, inputs, _, _ = t_case
    scale = GO.load_scale_factors(SCALE_FILE)
    mol = {k: v.to(DEV) for k, v in _molecules().items()}
    # matmul_precision = "f32": the old head launches
    monkeypatch.setattr(model, "matmul_precision", "f32")
    _, F, names = _count(model, inputs, redzone)
    assert torch.isfinite(F).all() and not any(names[n] for n in NEW) and all(names[n] == 1 for n in OLD_HEAD)
    monkeypatch.setattr(model, "matmul_precision", None)
    # direct forces
    cfg = dict(T_CFG, direct_forces=True, forces_coupled=True)
    _, F, names = _count(_build(cfg, GO.make_params(cfg, 11, scale)), mol, redzone)
    assert torch.isfinite(F).all() and not any(names[n] for n in NEW + OLD_HEAD)
    # GemNet-Q
    cfg = dict(T_CFG, triplets_only=False)
    qin = _molecules()
    qin.update({k: torch.tensor(v) for k, v in IO.build_indices(qin["R"].numpy(), np.array([8, 8]), 5.0, 10.0, False).items()})
    _, F, names = _count(_build(cfg, GO.make_params(cfg, 5, scale)), {k: v.to(DEV) for k, v in qin.items()}, redzone)
    assert torch.isfinite(F).all() and not any(names[n] for n in NEW + OLD_HEAD)
    # a periodic batch of a model with the widths the path takes
    cfg = dict(P.CFG, emb_size_rbf=16, emb_size_cbf=16, emb_size_atom=128, emb_size_edge=128)
    pm = _build(cfg, GO.make_params(cfg, 3, scale))
    R, Z, cell, pbc = P.structure("small")
    b = PeriodicGraphBuilder([len(R)], P.CUTOFF, pbc=pbc[None], device=DEV)
    idx = b(torch.tensor(R, dtype=torch.float64, device=DEV), torch.tensor(cell[None], dtype=torch.float64, device=DEV))
    batch = dict(idx, R=torch.tensor(R, dtype=torch.float32, device=DEV), Z=torch.tensor(Z, device=DEV).long(),
                 N=torch.tensor([len(R)], device=DEV), cell=torch.tensor(cell[None], dtype=torch.float32, device=DEV))
    _, F, names = _count(pm, batch, redzone)
    assert torch.isfinite(F).all() and not any(names[n] for n in NEW + OLD_HEAD)
    # (and the molecular model does take the path: the counter is live)
    _, _, names = _count(model, inputs, redzone)
    assert all(names[n] == 1 for n in NEW)
