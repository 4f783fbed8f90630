"""The fused radial head (csrc/radial_head.hip): distances + both radial bases + their four frozen projections in one launch,
and its adjoint.  Kernel level: against edge_basis_fwd (bit-identical basis values), a float64 product with a derived bound,
and the float64 adjoint of the CPU restatement; row independence and determinism.  Model level: the one-block GemNet-T of
`smoke()` with the head on and off against the float64 oracle, captured replay == eager, and the cases that keep the old
path.  One CPU test: the ABI declares / binds the two entry points and the launcher validates its shapes."""
import os
import re

import numpy as np
import pytest
import torch

import cpu_kernels as CK
from conftest import ROOT, SCALE_FILE
from gemnet_pytorch_amd import _lib
from gemnet_pytorch_amd import kernels as K
from oracle import basis_oracle as B
from redzone import put, redzone  # noqa: F401  (autouse: every test of this module runs under the red-zone harness)

gpu = pytest.mark.gpu
DEV = "cuda"
CUTOFF, P_ENV = 8.0, 5
NR, S, NI = 6, 7, 16


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_abi_declares_and_binds_the_radial_head_and_the_launcher_checks_shapes():
    with open(os.path.join(ROOT, "include", "gemnet_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name, nargs in (("gn_radial_head_fwd_f32", 19), ("gn_radial_head_bwd_f32", 20)):
        m = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name])
    g = torch.Generator().manual_seed(1)
    W = [torch.randn(NI, NR, generator=g) for _ in range(3)] + [torch.randn(S, NR, NI, generator=g)]
    wcat = K.radial_head_weights(*W)
    assert wcat.shape == (3 + S, NR, NI) and wcat.is_contiguous()
    assert torch.equal(wcat[1], W[1].t()) and torch.equal(wcat[3:], W[3])
    with pytest.raises(ValueError):
        K.radial_head_weights(W[0].t(), W[1], W[2], W[3])
    with pytest.raises(RuntimeError):       # no CPU fallback
        K.radial_head_fwd(torch.zeros(2, 3), torch.zeros(1, dtype=torch.int32), torch.ones(1, dtype=torch.int32),
                          torch.ones(NR), torch.ones(S, NR), torch.ones(S, NR, dtype=torch.float64), wcat, CUTOFF, P_ENV)


# ------------------------------------------------------------------------------------------------------------- kernels
class Case:
    """40 atoms in a 6 A box (some distances exceed the cutoff), 300 random edges, random weights and cotangents; the
    float64 references are computed once."""

    def __init__(self):
        g = torch.Generator().manual_seed(33)
        n_atoms, n_edges = 40, 300
        self.R = torch.rand(n_atoms, 3, generator=g, dtype=torch.float64) * 6.0
        ic = torch.randint(0, n_atoms, (n_edges,), generator=g)
        ia = (ic + 1 + torch.randint(0, n_atoms - 1, (n_edges,), generator=g)) % n_atoms    # != ic
        self.ic, self.ia = ic.int(), ia.int()
        self.z, self.nrm = torch.tensor(B.jn_zeros(S, NR)), torch.tensor(B.sph_bessel_normalizer(S, NR))
        self.freq = torch.arange(1, NR + 1, dtype=torch.float64) * np.pi
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()          # noqa: E731
        self.W = [rn(NI, NR), rn(NI, NR), rn(NI, NR), rn(S, NR, NI)]
        self.g = dict(rbf=rn(n_edges, NR), rbf3=rn(n_edges, NI), rbf_h=rn(n_edges, NI), rbf_out=rn(n_edges, NI),
                      rbf_W1=rn(n_edges, S, NI))
        self.dev = dict(R=put(self.R.float()), ic=put(self.ic), ia=put(self.ia), freq=put(self.freq.float()),
                        z=put(self.z.float()), nrm=put(self.nrm), wcat=put(K.radial_head_weights(*self.W)))

    def fwd(self, E):
        d = self.dev
        return K.radial_head_fwd(d["R"], d["ic"][:E], d["ia"][:E], d["freq"], d["z"], d["nrm"], d["wcat"], CUTOFF, P_ENV)

    def bwd(self, E, names):
        d = self.dev
        gs = [put(self.g[n][:E]) if n in names else None for n in ("rbf", "rbf3", "rbf_h", "rbf_out", "rbf_W1")]
        return K.radial_head_bwd(*gs, d["R"], d["ic"][:E], d["ia"][:E], d["freq"], d["z"], d["nrm"], d["wcat"], CUTOFF, P_ENV)

    def bwd_ref(self, E, names):
        """CK.edge_basis_bwd on the cotangents composed in float64 (g_rbf_total, g_rad)."""
        W3, Wh, Wo, Wc = [w.double() for w in self.W]
        g = {n: self.g[n][:E].double() for n in names}
        terms = [g[n] @ W for n, W in (("rbf3", W3), ("rbf_h", Wh), ("rbf_out", Wo)) if n in g]
        if "rbf" in g:
            terms.append(g["rbf"])
        g_rbf = sum(terms) if terms else None
        g_rad = torch.einsum("sri,esi->esr", Wc, g["rbf_W1"]) if "rbf_W1" in g else None
        return CK.edge_basis_bwd(None, g_rbf, g_rad, self.R.float().double(), self.ic[:E], self.ia[:E], self.freq.float().double(),
                                 self.z.float(), self.nrm, CUTOFF, P_ENV)


@pytest.fixture(scope="module")
def case():
    return Case()


@gpu
@pytest.mark.parametrize("E", [1, 17, 300])
def test_forward_basis_is_bit_identical_and_projections_meet_the_fp32_bound(case, E):
    d = case.dev
    rbf, rbf3, rbf_h, rbf_out, rbf_W1 = case.fwd(E)
    _, _, rbf_ref, rad = K.edge_basis_fwd(d["R"], d["ic"][:E], d["ia"][:E], d["freq"], d["z"], d["nrm"], CUTOFF, P_ENV)
    assert torch.equal(rbf, rbf_ref)
    assert float(rbf.abs().max()) > 0 and float(rad.abs().max()) > 0
    # each output is one chain of six fp32 multiply-adds over r, then stored: |err| <= 8 * 2^-24 * sum_k |w_k| |b_k|
    # (gamma_6 plus the final rounding; the right-hand side in float64 from the f32 basis values the kernel itself used)
    b, r = rbf.double().cpu(), rad.double().cpu()
    eps = 8.0 * 2.0 ** -24
    for out, W in ((rbf3, case.W[0]), (rbf_h, case.W[1]), (rbf_out, case.W[2])):
        ref, mag = b @ W.double().t(), b.abs() @ W.double().abs().t()
        err = (out.double().cpu() - ref).abs()
        print(f"E={E}: (E,16) projection max err/bound {float((err / (eps * mag).clamp(min=1e-300)).max()):.3f}")
        assert (err <= eps * mag).all()
    Wc = case.W[3].double()
    ref, mag = torch.einsum("esr,sri->esi", r, Wc), torch.einsum("esr,sri->esi", r.abs(), Wc.abs())
    err = (rbf_W1.double().cpu() - ref).abs()
    print(f"E={E}: rbf_W1 max err/bound {float((err / (eps * mag).clamp(min=1e-300)).max()):.3f}")
    assert rbf_W1.shape == (E, S, NI) and (err <= eps * mag).all()


ALL = ("rbf", "rbf3", "rbf_h", "rbf_out", "rbf_W1")


@gpu
@pytest.mark.parametrize("E", [1, 17, 300])
@pytest.mark.parametrize("names", [ALL] + [(n,) for n in ALL], ids=lambda n: "+".join(n))
def test_adjoint_matches_the_float64_adjoint_of_the_composed_cotangents(case, E, names):
    W = case.bwd(E, names)
    ref = case.bwd_ref(E, names)
    err = (W.double().cpu() - ref).abs()
    atol = 2e-4 * float(ref.abs().max())          # the bar of test_edge_basis_fused_fwd_bwd
    print(f"E={E} {names}: max err {float(err.max()):.3e}, atol {atol:.3e}")
    assert float(ref.abs().max()) > 0
    assert (err <= atol + 2e-4 * ref.abs()).all()


@gpu
def test_rows_do_not_depend_on_other_edges_and_runs_repeat_bitwise(case):
    full, part = case.fwd(300), case.fwd(37)
    for a, b in zip(full, part):
        assert torch.equal(a[:37], b)
    Wf, Wp = case.bwd(300, ALL), case.bwd(37, ALL)
    assert torch.equal(Wf[:37], Wp)
    for a, b in zip(full, case.fwd(300)):
        assert torch.equal(a, b)
    assert torch.equal(Wf, case.bwd(300, ALL))


# --------------------------------------------------------------------------------------------------------------- model
SMOKE_CFG = dict(num_spherical=7, num_radial=6, num_blocks=1, emb_size_atom=64, emb_size_edge=64, emb_size_trip=32,
                 emb_size_quad=32, emb_size_rbf=16, emb_size_cbf=16, emb_size_sbf=32, emb_size_bil_quad=32, emb_size_bil_trip=32,
                 num_before_skip=1, num_after_skip=1, num_concat=1, num_atom=2, triplets_only=True)


def _build(cfg, params):
    from gemnet_pytorch_amd.model.gemnet import GemNet
    from oracle import gemnet_oracle as GO
    model = GemNet(**cfg, scale_file=SCALE_FILE)
    model.load_state_dict(GO.expand_to_reference_state_dict({k: v.float() for k, v in params.items()}))
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def smoke_case():
    """The molecule, parameters and float64 oracle result of `smoke()`."""
    from gemnet_pytorch_amd.synthetic import make_molecule
    from oracle import gemnet_oracle as GO
    from oracle import index_oracle as IO
    mol = make_molecule(12, 1000)
    idx = IO.build_indices(mol["R"], np.array([12]), 5.0, 10.0, True)
    inputs = {k: torch.tensor(v) for k, v in idx.items()}
    inputs.update(Z=torch.tensor(mol["Z"]).long(), R=torch.tensor(mol["R"]), N=torch.tensor([12]))
    params = GO.make_params(SMOKE_CFG, 1, GO.load_scale_factors(SCALE_FILE))
    E_ref, F_ref = GO.forward(SMOKE_CFG, params, inputs)
    return params, inputs, E_ref.detach(), F_ref.detach()


@pytest.fixture
def head_calls(monkeypatch):
    """Counts the launches of the fused forward."""
    calls, real = [], K.radial_head_fwd

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(K, "radial_head_fwd", counted)
    return calls


@gpu
@pytest.mark.parametrize("on", [True, False])
def test_model_meets_the_smoke_bar_with_the_head_on_and_off(smoke_case, head_calls, monkeypatch, on):
    from gemnet_pytorch_amd import ops
    params, inputs, E_ref, F_ref = smoke_case
    monkeypatch.setattr(ops, "USE_RADIAL_HEAD", on)
    model = _build(SMOKE_CFG, params)
    E, F = model({k: v.to(DEV) for k, v in inputs.items()})
    torch.cuda.synchronize()
    assert len(head_calls) == (1 if on else 0)
    f_mae = float((F.detach().cpu().double() - F_ref).abs().mean())
    e_err = float((E.detach().cpu().double() - E_ref).abs().max())
    scale = max(1.0, float(F_ref.abs().mean()))
    print(f"head {'on' if on else 'off'}: E err {e_err:.3e}, force MAE {f_mae:.3e} (scale {scale:.2f})")
    assert f_mae <= 1e-5 * scale and e_err <= 2e-5 * max(1.0, float(E_ref.abs().max()))


@gpu
def test_captured_replay_with_the_head_equals_eager_bitwise(smoke_case, head_calls):
    params, inputs, _, _ = smoke_case
    model = _build(SMOKE_CFG, params)
    model.requires_grad_(False)
    dev = {k: v.to(DEV) for k, v in inputs.items()}
    for _ in range(2):
        model(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model(dev)
    torch.cuda.current_stream().wait_stream(side)
    n = len(head_calls)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Eg, Fg = model(dev)
    assert len(head_calls) == n + 1            # the capture went through the fused head
    graph.replay()
    torch.cuda.synchronize()
    E, F = model(dev)
    assert torch.equal(E, Eg) and torch.equal(F, Fg)


@gpu
def test_direct_forces_and_periodic_batches_keep_the_old_path(smoke_case, head_calls):
    from oracle import gemnet_oracle as GO
    import pbc_common as P
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder
    _, inputs, _, _ = smoke_case
    scale = GO.load_scale_factors(SCALE_FILE)
    cfg = dict(SMOKE_CFG, direct_forces=True, forces_coupled=True)
    model = _build(cfg, GO.make_params(cfg, 11, scale))
    E, F = model({k: v.to(DEV) for k, v in inputs.items()})
    assert torch.isfinite(F).all() and len(head_calls) == 0
    # a periodic batch of a model with the widths the head takes
    cfg = dict(P.CFG, emb_size_rbf=16, emb_size_cbf=16)
    model = _build(cfg, GO.make_params(cfg, 3, scale))
    R, Z, cell, pbc = P.structure("small")
    b = PeriodicGraphBuilder([len(R)], P.CUTOFF, pbc=pbc[None], device=DEV)
    idx = b(torch.tensor(R, dtype=torch.float64, device=DEV), torch.tensor(cell[None], dtype=torch.float64, device=DEV))
    batch = dict(idx, R=torch.tensor(R, dtype=torch.float32, device=DEV), Z=torch.tensor(Z, device=DEV).long(),
                 N=torch.tensor([len(R)], device=DEV), cell=torch.tensor(cell[None], dtype=torch.float32, device=DEV))
    E, F = model(batch)
    assert torch.isfinite(F).all() and len(head_calls) == 0
    # (and the same model on a molecule does take it: the counter is live)
    mol = dict(SMOKE_CFG)
    model = _build(mol, GO.make_params(mol, 1, scale))
    model({k: v.to(DEV) for k, v in inputs.items()})
    assert len(head_calls) == 1
