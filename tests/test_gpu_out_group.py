"""The grouped output blocks: all OutputBlocks of a GemNet-T force pass as three launches forward and
three backward.  Kernel level: the grouped aggregation (csrc/aggregate.hip), the grouped chain launch (csrc/chain2.hip) and
the energy head (csrc/energy_head.hip) against the single launches they replace (bit for bit) resp. float64.  Model level:
the grouped path against GEMNET_OUT_GROUP=0 on the same model, captured replay == eager, and the passes that keep one set of
launches per block.  One CPU test: the ABI declares and binds the new entry points."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, SCALE_FILE
from gemnet_pytorch_amd import _lib
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd import ops
from redzone import put, redzone  # noqa: F401  (autouse: every test of this module runs under the red-zone harness)

gpu = pytest.mark.gpu
DEV = "cuda"
C, NR = 128, 16


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_abi_declares_and_binds_the_grouped_entry_points():
    with open(os.path.join(ROOT, "include", "gemnet_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name, nargs in (("gn_chain_split_grouped_f32", 6), ("gn_rbf_aggregate_grouped_fwd_f32", 12),
                        ("gn_rbf_aggregate_grouped_bwd_f32", 16), ("gn_energy_head_fwd_f32", 7), ("gn_energy_head_bwd_f32", 7)):
        m = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name])


# -------------------------------------------------------------------------------------------------------- aggregation
class AggCase:
    """37 atoms (not a multiple of 16), 200 edges: atom 0 has no incoming edge, atom 1 has 70, the rest are spread over
    atoms 2..36; five groups of (m, W, scale) share rbf and the CSR.  The single launches are computed once."""
    A, E, G = 37, 200, 5

    def __init__(self):
        g = torch.Generator().manual_seed(5)
        rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
        ia = torch.cat([torch.full((70,), 1), torch.randint(2, self.A, (self.E - 70,), generator=g)])
        self.ia = put(ia[torch.randperm(self.E, generator=g)].int())
        self.perm, self.seg = K.csr_build(self.ia, self.A)
        deg = torch.bincount(self.ia.long().cpu(), minlength=self.A)
        assert deg[0] == 0 and deg[1] > 64
        self.rbf = put(rn(self.E, NR))
        self.m = [put(rn(self.E, C)) for _ in range(self.G)]
        self.W = [put(rn(C, NR) / 4) for _ in range(self.G)]
        self.scales = put(0.5 + torch.rand(self.G, generator=g))
        self.sc = [float(v) for v in self.scales.cpu()]            # the same fp32 values as host scalars
        self.g_out = put(rn(self.G, self.A, C))
        self.prev_m = put(rn(self.E, C))                       # running gradient of the group with the accumulate bit
        self.out1 = [K.rbf_aggregate_fwd(self.m[i], self.rbf, self.W[i], self.perm, self.seg, self.A, self.sc[i])
                     for i in range(self.G)]
        self.acc_group = 1
        self.bwd1 = [K.rbf_aggregate_bwd(self.g_out[i], self.m[i], self.rbf, self.W[i], self.ia, self.sc[i],
                                         acc_m=self.prev_m.clone() if i == self.acc_group else None)
                     for i in range(self.G)]


@pytest.fixture(scope="module")
def agg():
    return AggCase()


@gpu
@pytest.mark.parametrize("G", [1, 2, 5])
def test_grouped_aggregation_forward_is_bit_identical_to_the_single_launches(agg, G):
    out = K.rbf_aggregate_grouped_fwd(agg.m[:G], agg.rbf, agg.W[:G], agg.scales[:G].contiguous(), agg.perm, agg.seg, agg.A)
    assert out.shape == (G, agg.A, C)
    for i in range(G):
        assert torch.equal(out[i], agg.out1[i]), f"group {i}"
    assert float(out[:, 0].abs().max()) == 0.0 and float(out[:, 1].abs().max()) > 0      # the empty and the 70-edge atom


@gpu
@pytest.mark.parametrize("A", [1, 17])
def test_grouped_aggregation_without_any_edge(A):
    """E = 0 (a single atom, a dissociated pair as a batch of its own): m, rbf and the CSR permutation are empty tensors.  The
    grouped forward returns the zeros of tests/cpu_kernels.py and of the single launches (it used to fail with hip error 1:
    an empty tensor has no address for the launcher's pointer table); the adjoint returns empty gradients."""
    import cpu_kernels as CK
    G = 3
    g = torch.Generator().manual_seed(A)
    ia = put(torch.zeros(0, dtype=torch.int32))
    perm, seg = K.csr_build(ia, A)
    m = [put(torch.zeros(0, C)) for _ in range(G)]
    W = [put(torch.randn(C, NR, generator=g) / 4) for _ in range(G)]
    rbf, scales = put(torch.zeros(0, NR)), put(0.5 + torch.rand(G, generator=g))
    out = K.rbf_aggregate_grouped_fwd(m, rbf, W, scales, perm, seg, A)
    assert out.shape == (G, A, C)
    seg_cpu = torch.zeros(A + 1, dtype=torch.int32)
    for i in range(G):
        ref = CK.rbf_aggregate_fwd(m[i].cpu().double(), rbf.cpu().double(), W[i].cpu().double(), None, seg_cpu, A, float(scales[i]))
        assert ref.shape == (A, C) and torch.equal(out[i].cpu().double(), ref) and not bool(ref.any())
        assert torch.equal(out[i], K.rbf_aggregate_fwd(m[i], rbf, W[i], perm, seg, A, float(scales[i])))
    g_m, g_rbf = K.rbf_aggregate_grouped_bwd(put(torch.randn(G, A, C, generator=g)), m, rbf, W, scales, ia)
    assert all(t.shape == (0, C) for t in g_m) and g_rbf.shape == (0, NR)


@gpu
@pytest.mark.parametrize("G", [1, 2, 5])
def test_grouped_aggregation_adjoint_matches_the_single_launches(agg, G):
    acc = [agg.prev_m.clone() if i == agg.acc_group else None for i in range(G)]
    g_m, g_rbf = K.rbf_aggregate_grouped_bwd(agg.g_out[:G].contiguous(), agg.m[:G], agg.rbf, agg.W[:G],
                                             agg.scales[:G].contiguous(), agg.ia, acc_m=acc)
    for i in range(G):
        assert torch.equal(g_m[i], agg.bwd1[i][0]), f"g_m of group {i}"
        assert acc[i] is None or g_m[i] is acc[i]
    # g_rbf = the G single-launch terms added in fp32, g = 0 .. G-1: against their float64 sum the rounding of a G-term
    # fp32 sum, G * 2^-23 * sum_g |term_g| per element
    terms = torch.stack([agg.bwd1[i][1].double() for i in range(G)])
    ref, mag = terms.sum(0), terms.abs().sum(0)
    err = (g_rbf.double() - ref).abs()
    print(f"G={G}: g_rbf max err / bound {float((err / (G * 2.0 ** -23 * mag).clamp(min=1e-300)).max()):.3f}")
    assert (err <= G * 2.0 ** -23 * mag).all()
    if G == 1:
        assert torch.equal(g_rbf, agg.bwd1[0][1])
    # the running-gradient form of g_rbf adds onto what is there
    prev = torch.ones_like(g_rbf)
    _, g_acc = K.rbf_aggregate_grouped_bwd(agg.g_out[:G].contiguous(), agg.m[:G], agg.rbf, agg.W[:G],
                                           agg.scales[:G].contiguous(), agg.ia, acc_rbf=prev)
    assert g_acc is prev and torch.equal(g_acc, 1.0 + g_rbf)


# -------------------------------------------------------------------------------------------------------- chain launch
def _weights(G, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [[put(torch.randn(C, C, generator=g) / C ** 0.5) for _ in range(G)] for _ in range(n)]


def _forward_program(M, x, Ws, packed, zs, y):
    """The output-block stack: Dense + two ResidualLayers, activations on, ssilu'(z) stored (ops._Stack.forward)."""
    prog = K.ChainProgram(M)
    prog.load(0, x)
    prog.gemm(Ws[0], packed=packed[0], a_slot=0, y_slot=1, act=True, pre_deriv=True, pre_out=zs[0])
    for k in range(2):
        prog.gemm(Ws[1 + 2 * k], packed=packed[1 + 2 * k], a_slot=1, y_slot=0, act=True, pre_out=zs[1 + 2 * k], pre_deriv=True)
        prog.gemm(Ws[2 + 2 * k], packed=packed[2 + 2 * k], a_slot=0, y_slot=1, act=True, pre_out=zs[2 + 2 * k], pre_deriv=True,
                  res=1, beta=2 ** -0.5, out=y if k == 1 else None)
    return prog


def _adjoint_program(M, g, Ws, packed, zs, gx):
    """Its adjoint with stored factors (ops._Stack.backward), fused as the product path fuses it."""
    prog = K.ChainProgram(M)
    prog.load(0, g)
    for k in (1, 0):
        prog.scale(0, 0, 2 ** -0.5, width=C)
        prog.scale(1, 0, 1.0, Z=zs[2 + 2 * k], mode=1)
        prog.gemm(Ws[2 + 2 * k], packed=packed[2 + 2 * k], a_slot=1, y_slot=1)
        prog.scale(1, 1, 1.0, Z=zs[1 + 2 * k], mode=1)
        prog.gemm(Ws[1 + 2 * k], packed=packed[1 + 2 * k], a_slot=1, y_slot=0, res=0, beta=1.0)
    prog.scale(1, 0, 1.0, Z=zs[0], width=C, mode=1)
    prog.gemm(Ws[0], packed=packed[0], a_slot=1, y_slot=-1, out=gx)
    return K.fuse_program(prog)


SENTINEL = 777.0


@gpu
@pytest.mark.parametrize("mode", ["h3", "split6"])
@pytest.mark.parametrize("tile", [16, 32])
@pytest.mark.parametrize("G", [2, 5])
def test_grouped_chain_is_bit_identical_to_separate_launches(mode, tile, G):
    fmt = K.SPLIT_FORMAT[mode]
    Ws = _weights(G, 5, 3)
    packed1 = [[K.pack_weight_split(W, fmt=fmt) for W in row] for row in Ws]
    stacked = [K.pack_weight_split_stacked(row, fmt=fmt) for row in Ws]
    g = torch.Generator().manual_seed(7)
    for rows in (16, 40, 48):      # 40: a partial tile at either height
        pitch = rows + 8           # eight rows between the groups that no launch may touch
        x = put(torch.randn(G, pitch, C, generator=g))
        fac = [put(0.1 + torch.rand(G, pitch, C, generator=g)) for _ in range(5)]       # stand-ins for ssilu'(z)
        for adjoint in (False, True):
            new = lambda: torch.full((G, pitch, C), SENTINEL, device=DEV)    # noqa: E731
            if adjoint:
                outs_g, outs_1 = [new()], [new()]
                build = lambda i, o, pk: _adjoint_program(rows, x[i, :rows], [r[i] for r in Ws], pk,       # noqa: E731
                                                          [f[i, :rows] for f in fac], o[0][i, :rows])
            else:
                outs_g, outs_1 = [new() for _ in range(6)], [new() for _ in range(6)]
                build = lambda i, o, pk: _forward_program(rows, x[i, :rows], [r[i] for r in Ws], pk,       # noqa: E731
                                                          [z[i, :rows] for z in o[:5]], o[5][i, :rows])
            for i in range(G):
                K.chain(build(i, outs_1, [r[i] for r in packed1]), mode=mode)
            K.chain(build(0, outs_g, stacked), mode=mode, groups=G, group_pitch=pitch, tile_rows=tile)
            for a, b in zip(outs_g, outs_1):
                assert torch.equal(a, b), (mode, tile, G, rows, adjoint)
                assert bool((a[:, rows:] == SENTINEL).all()) and bool((a[:, :rows] != SENTINEL).all())


@gpu
def test_grouped_chain_rejects_row_gathers_and_other_arithmetics():
    Ws = _weights(2, 1, 4)
    x = put(torch.randn(2, 16, C))
    y = torch.empty(2, 16, C, device=DEV)
    rows = torch.arange(16, dtype=torch.int32, device=DEV)
    prog = K.ChainProgram(16)
    prog.load(0, x[0], rows=rows)
    prog.gemm(Ws[0][0], packed=K.pack_weight_split_stacked(Ws[0], fmt=1), a_slot=0, y_slot=-1, out=y[0])
    with pytest.raises(RuntimeError, match="hip error 1 "):         # hipErrorInvalidValue
        K.chain(prog, mode="h3", groups=2, group_pitch=16)
    with pytest.raises(RuntimeError, match="no grouped launch"):
        K.chain(prog, mode="split3", groups=2, group_pitch=16)


# --------------------------------------------------------------------------------------------------------- energy head
@gpu
def test_energy_head_forward_and_adjoint_against_float64():
    G, A = 3, 37
    g = torch.Generator().manual_seed(2)
    x, w, gE = torch.randn(G, A, C, generator=g), torch.randn(G, C, generator=g) / C ** 0.5, torch.randn(A, 1, generator=g)
    E = K.energy_head_fwd(put(x), put(w))
    prod = x.double() * w.double()[:, None, :]
    ref, mag = prod.sum((0, 2)), prod.abs().sum((0, 2))
    # per group 128 rounded products folded by a tree of depth 7 (one add inside the lane, six across), then G - 1 adds in
    # block order: every term passes through at most 1 + 7 + (G - 1) roundings -> (7 + G) * 2^-24 * sum |x w| to first order;
    # one more unit covers the second-order terms
    eps = (8 + G) * 2.0 ** -24
    err = (E[:, 0].double().cpu() - ref).abs()
    print(f"energy head: max err / bound {float((err / (eps * mag)).max()):.3f}")
    assert E.shape == (A, 1) and (err <= eps * mag).all()
    gx = K.energy_head_bwd(put(gE), put(w))
    ref = gE.double()[None, :, :] * w.double()[:, None, :]
    assert gx.shape == (G, A, C) and ((gx.double().cpu() - ref).abs() <= 2.0 ** -24 * ref.abs()).all()     # one rounding


# --------------------------------------------------------------------------------------------------------------- model
T_CFG = dict(num_spherical=7, num_radial=6, num_blocks=2, emb_size_atom=128, emb_size_edge=128, emb_size_trip=64,
             emb_size_quad=32, emb_size_rbf=16, emb_size_cbf=16, emb_size_sbf=32, emb_size_bil_trip=64, emb_size_bil_quad=32,
             num_before_skip=1, num_after_skip=1, num_concat=1, num_atom=2, triplets_only=True, num_targets=1,
             direct_forces=False)


def _model(cfg, seed=3):
    from gemnet_pytorch_amd.model.gemnet import GemNet
    torch.manual_seed(seed)
    model = GemNet(**cfg, scale_file=SCALE_FILE).to(DEV).eval()
    return model


def _molecules(sizes, triplets_only=True):
    from gemnet_pytorch_amd.synthetic import make_molecule
    from oracle import index_oracle as IO
    mols = [make_molecule(n, 100 + n) for n in sizes]
    R, Z = np.concatenate([m["R"] for m in mols]), np.concatenate([m["Z"] for m in mols])
    idx = IO.build_indices(R, np.array(sizes), 5.0, 10.0, triplets_only)
    inputs = {k: torch.tensor(v) for k, v in idx.items()}
    inputs.update(Z=torch.tensor(Z).long(), R=torch.tensor(R), N=torch.tensor(sizes))
    return {k: v.to(DEV) for k, v in inputs.items()}


@pytest.fixture(scope="module")
def t_case():
    return _model(T_CFG), _molecules([5, 9, 12])


def _run(model, inputs, on, monkeypatch):
    monkeypatch.setattr(ops, "USE_OUT_GROUP", on)
    n = ops.OUT_GROUP_CALLS
    E, F = model(inputs)
    torch.cuda.synchronize()
    return E.detach(), F.detach(), ops.OUT_GROUP_CALLS - n


@gpu
def test_model_grouped_path_agrees_with_the_per_block_path(t_case, monkeypatch):
    model, inputs = t_case
    # the rows that enter the energy heads (identical in both paths: aggregation and chain are bit-identical), recorded
    # from the per-block path: sum_g |x_g| . |w_g| per atom bounds what a different summation order can change
    xs = []
    hooks = [ob.out_energy.register_forward_hook(lambda mod, a, out: xs.append(a[0].detach())) for ob in model.out_blocks]
    E0, F0, n0 = _run(model, inputs, False, monkeypatch)
    for h in hooks:
        h.remove()
    E1, F1, n1 = _run(model, inputs, True, monkeypatch)
    assert n0 == 0 and n1 == 1 and len(xs) == 3
    mag_a = sum(x.double().abs() @ ob.out_energy.weight.detach().double().abs().t() for x, ob in zip(xs, model.out_blocks))[:, 0]
    seg = torch.repeat_interleave(torch.arange(3, device=DEV), inputs["N"])
    mag = torch.zeros(3, dtype=torch.float64, device=DEV).index_add_(0, seg, mag_a)
    # E_mol is a sum of n_atoms * G * 128 products; each path rounds every term at most 1 + 7 (dot product tree, K order
    # free) + G (block sum) + n_atoms (molecule sum) times: the two orders differ by at most twice that many half-ulps of
    # sum |terms|
    n_round = 8 + 3 + int(inputs["N"].max())
    bound = 2 * n_round * 2.0 ** -24 * mag
    dE = (E1.double() - E0.double()).abs()[:, 0]
    f_mae, f_mean = float((F1 - F0).abs().mean()), float(F0.abs().mean())
    print(f"grouped vs per-block: max |dE| {float(dE.max()):.3e} (bound {float(bound.min()):.3e}), "
          f"force MAE {f_mae:.3e}, mean |F| {f_mean:.3e}")
    assert (dE <= bound).all()
    assert f_mae <= 1e-5 * f_mean


@gpu
def test_captured_replay_of_the_grouped_path_equals_eager_bitwise(t_case, monkeypatch):
    model, inputs = t_case
    monkeypatch.setattr(ops, "USE_OUT_GROUP", True)
    model = model.requires_grad_(False)
    E0, F0 = (t.detach().clone() for t in model(inputs))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model(inputs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    n = ops.OUT_GROUP_CALLS
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Eg, Fg = model(inputs)
    assert ops.OUT_GROUP_CALLS == n + 1
    for _ in range(10):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(Eg, E0) and torch.equal(Fg, F0)
    model.requires_grad_(True)


@gpu
@pytest.mark.parametrize("kind", ["direct", "Q", "training", "f32", "row", "no-aggregate"])
def test_other_passes_keep_one_set_of_launches_per_block(kind, monkeypatch):
    """Model kinds, and a chain arithmetic / kernel layout / aggregation switch without the grouped launches: the decision is
    taken before the first interaction block, so these passes are the GEMNET_OUT_GROUP=0 pass, launch for launch."""
    cfg = dict(T_CFG, num_blocks=1)
    if kind == "direct":
        cfg.update(direct_forces=True, forces_coupled=True)
    elif kind == "Q":
        cfg.update(triplets_only=False)
    model = _model(cfg, seed=5)
    inputs = _molecules([5, 9], triplets_only=kind != "Q")
    if kind == "training":
        model = model.train()
    elif kind == "f32":
        model.matmul_precision = "f32"
    elif kind == "row":
        monkeypatch.setattr(K, "CHAIN_LAYOUT", "row")
    elif kind == "no-aggregate":
        monkeypatch.setattr(ops, "USE_AGGREGATE", False)
    E1, F1, n1 = _run(model, inputs, True, monkeypatch)
    E0, F0, n0 = _run(model, inputs, False, monkeypatch)
    assert n1 == 0 and n0 == 0
    assert torch.isfinite(F1).all() and torch.equal(E1, E0) and torch.equal(F1, F0)
    if kind == "training":         # (the counter is live: the same model in eval mode does take the grouped path)
        assert _run(model.eval(), inputs, True, monkeypatch)[2] == 1
