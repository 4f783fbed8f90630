"""The first-order adjoint of the atom-row MLP stack on its own kernel (csrc/atom_stack.hip, gn_atom_stack_bwd_f32; DESIGN.md
section 25).  CPU: the header declares the entry point and the binding matches; `kernels.atom_stack_adjoint_match` takes exactly
the fused programs the kernel instantiates, `atom_stack_match` none of them.  GPU, kernel level (under the red-zone harness):
every (layers, tails, skip form) at row counts below, at and above one 16-row tile against the chain launch of the same fused
program (GEMNET_ATOM_STACK_BWD=0), bit for bit, on factors a real forward launch stored; a zero row and rows of extreme scale in
all cotangents; sentinels; row independence; determinism; captured replay == eager under the happens-before checker; the
launcher's refusals.  Model level: a two-block GemNet-T (both skip forms) against the float64 oracle with the switch on and off."""
import os
import re

import pytest
import torch

from conftest import ROOT, SCALE_FILE
from gemnet_pytorch_amd import _lib, hbcheck
from gemnet_pytorch_amd import kernels as K
from oracle import gemnet_oracle as GO
from redzone import put, redzone  # noqa: F401  (autouse: every test of this module runs under the red-zone harness)
from test_gpu_atom_stack import T_CFG, _build, _count, _molecules, _same

gpu = pytest.mark.gpu
DEV = "cuda"
C = 128
S = 2 ** -0.5          # ResidualLayer scale
SB = 2 ** -0.5         # skip_beta of the AtomUpdateBlock
NEW = "gn_atom_stack_bwd_f32"
FWD = "gn_atom_stack_fwd_f32"
OLD = "gn_chain_split_f32"
# (layers, tails, form): "A" the skip's gradient is an output of its own, "B" it is not wanted, "N" a stack without a skip
FORMS = [(L, T, f) for L in (1, 2) for T in (0, 2) for f in "ABN"]
SIZES = [1, 15, 16, 17, 33, 300]
SENTINEL = 12345.0


def _forward(M, x, Ws, zs, y, ts, L, res2=None, packed=None):
    """What ops._Stack.forward builds for an AtomUpdateBlock (the factors ssilu'(z) are stored into `zs`)."""
    pk = packed or [None] * len(Ws)
    p = K.ChainProgram(M)
    p.load(0, x)
    p.gemm(Ws[0], packed=pk[0], a_slot=0, y_slot=1, act=True, pre_deriv=True, pre_out=zs[0], out=None if L else y)
    for k in range(L):
        last = k + 1 == L
        p.gemm(Ws[1 + 2 * k], packed=pk[1 + 2 * k], a_slot=1, y_slot=0, act=True, pre_deriv=True, pre_out=zs[1 + 2 * k])
        p.gemm(Ws[2 + 2 * k], packed=pk[2 + 2 * k], a_slot=0, y_slot=1, act=True, pre_deriv=True, pre_out=zs[2 + 2 * k], res=1,
               beta=S, res2=res2 if last else None, beta2=SB, out=y if last else None)
    for i, t in enumerate(ts):
        p.gemm(Ws[1 + 2 * L + i], packed=pk[1 + 2 * L + i], a_slot=1, y_slot=-1, out=t)
    return p


def _adjoint(M, g, gts, Wt, zs, gx, g_skip, L, form, packed=None, zmode=1, width=C, dz0=None, prev=None, park=False):
    """The calls ops._Stack.backward makes (first = Dense with activation, L ResidualLayers, the last with a skip unless form "N",
    tails with live cotangents): Wt the TRANSPOSED weights in forward order [W0, (W1, W2) per layer, tails]; not yet fused."""
    pk = packed or [None] * len(Wt)
    p = K.ChainProgram(M)
    p.load(0, g)
    for i, gt in enumerate(gts):
        p.load(1, gt)
        p.gemm(Wt[1 + 2 * L + i], packed=pk[1 + 2 * L + i], a_slot=1, y_slot=0, res=0, beta=1.0)
    for k in range(L - 1, -1, -1):
        c = S
        if k == L - 1 and form != "N":
            if form == "A" and park:
                p.scale(2, 0, SB, width=width)
                c = S * SB
            elif form == "A":
                p.scale(0, 0, SB, out=g_skip, width=width)
            else:
                c = S * SB
        p.scale(0, 0, c, width=width)
        p.scale(1, 0, 1.0, Z=zs[2 + 2 * k], mode=zmode)
        p.gemm(Wt[2 + 2 * k], packed=pk[2 + 2 * k], a_slot=1, y_slot=1)
        p.scale(1, 1, 1.0, Z=zs[1 + 2 * k], mode=zmode)
        p.gemm(Wt[1 + 2 * k], packed=pk[1 + 2 * k], a_slot=1, y_slot=0, res=0, beta=1.0)
    p.scale(1, 0, 1.0, Z=zs[0], out=dz0, width=width, mode=zmode)
    p.gemm(Wt[0], packed=pk[0], a_slot=1, y_slot=-1, out=gx, res=2 if park else None, beta=1.0, res2=prev, beta2=1.0)
    return p


def _host_adjoint(M, L, T, form, width=C, **kw):
    e = lambda: torch.empty(M, width)      # noqa: E731
    Wt = [torch.empty(width, width) for _ in range(1 + 2 * L + 2)]
    return _adjoint(M, e(), [e() for _ in range(T)], Wt, [e() for _ in range(1 + 2 * L)], e(), e() if form == "A" else None, L, form,
                    width=width, **kw)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_abi_declares_and_binds_the_entry_point():
    with open(os.path.join(ROOT, "include", "gemnet_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(NEW + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{NEW} is not declared"
    assert len(m.group(1).split(",")) == 18 == len(_lib.SIGNATURES[NEW])
    kinds = dict(hbcheck.parse_header()[0][NEW])
    assert kinds["g"] == "r" and kinds["gt"] == "ra" and kinds["W"] == "ra" and kinds["F"] == "ra"
    assert kinds["g_skip"] == "w" and kinds["gx"] == "w" and kinds["stream"] == "stream"
    assert K.USE_ATOM_STACK_BWD == (os.environ.get("GEMNET_ATOM_STACK_BWD", "1") == "1")       # a switch of its own


@pytest.mark.parametrize("L,T,form", FORMS)
def test_matcher_accepts_the_fused_forms_of_the_adjoint(L, T, form):
    for M in (1, 1024, 4096):
        raw = _host_adjoint(M, L, T, form)
        p = K.fuse_program(raw)
        m = K.atom_stack_adjoint_match(p, "h3")
        assert m is not None and m["L"] == L and len(m["gt"]) == T and m["form"] == (form == "A")
        assert len(m["gemms"]) == T + 2 * L + 1 and len(m["F"]) == 2 * L + 1
        assert m["g"] is raw.ops[0]["src"] and m["gx"] is raw.ops[-1]["out"] and (m["g_skip"] is not None) == (form == "A")
        # the factors in the order of use: z2, z1 of the last layer first, the Dense's last
        zs = [o["Z"] for o in raw.ops if o["kind"] == "scale" and o["Z"] is not None]
        assert len(zs) == len(m["F"]) and all(a is b for a, b in zip(zs, m["F"]))
        c = {"A": S, "B": S * SB, "N": S}[form]
        if T == 0 and form != "A":
            assert m["alpha0"] == c and m["bt"] == [1.0, 1.0]
        elif T == 0:
            assert m["alpha0"] == 1.0 and m["a_out"] == SB and m["a_s"] == S
        elif form == "A":
            assert m["bt"] == [1.0, SB] and m["a_s"] == S and m["alpha0"] == 1.0
        else:
            assert m["bt"] == [1.0, c] and m["alpha0"] == 1.0
        assert m["bl"][:L] == ([S, 1.0] if L == 2 else [1.0])
        assert K.atom_stack_match(p, "h3") is None and K.atom_stack_match(raw, "h3") is None       # never the forward's kernel


def test_matcher_refuses_everything_else(monkeypatch):
    ok = lambda p, mode="h3": K.atom_stack_adjoint_match(p, mode) is not None      # noqa: E731
    fused = lambda *a, **kw: K.fuse_program(_host_adjoint(*a, **kw))               # noqa: E731
    e = lambda: torch.empty(64, C)      # noqa: E731
    rows = torch.zeros(64, dtype=torch.int32)
    assert ok(fused(64, 2, 2, "A")) and ok(fused(64, 2, 2, "B"))
    refused = [_host_adjoint(64, 2, 2, "A"), _host_adjoint(64, 2, 0, "N")]        # the unfused programs
    refused.append(fused(64, 2, 2, "A", prev=e()))                               # a running sum on the last GEMM
    refused.append(fused(64, 2, 2, "A", park=True))                              # a parked skip (skip_is_x)
    refused.append(fused(64, 2, 2, "B", dz0=e()))                                # the Dense's dz0 output (gathered adds of the forward)
    refused.append(fused(64, 2, 2, "B", zmode=0))                                # training sweeps: plain z stored
    refused.append(fused(64, 2, 2, "B", width=64))                               # another width
    refused.append(fused(4097, 2, 2, "A"))                                       # beyond the 16-row launches of the chain kernel
    refused.append(fused(64, 0, 0, "N"))                                         # no ResidualLayer
    for T1 in ("A", "B"):                                                        # one live tail cotangent
        p = _host_adjoint(64, 2, 2, T1)
        del p.ops[1:3]
        refused.append(K.fuse_program(p))

    def changed(i, form="B", **kw):
        p = fused(64, 2, 2, form)
        p.ops[i].update(kw)
        return p
    refused.append(changed(0, src=None))                                         # g is None
    refused.append(changed(0, rows=rows))
    refused.append(changed(2, gadd1=e(), gidx1=rows))                            # a gathered add
    refused.append(changed(2, res=e()))                                          # a global residual in place of the running gradient
    refused.append(changed(5, mul_mode=2))                                       # a factor that is not stored as ssilu'
    refused.append(changed(6, mode2=0))
    refused.append(changed(6, alpha2=0.5))
    refused.append(changed(9, out2=e()))
    refused.append(changed(9, act=True))
    refused.append(changed(5, form="A", Z=e()))                                  # form A's plain SCALE with a factor
    for p in refused:
        assert not ok(p)
        assert K.atom_stack_match(p, "h3") is None
    assert not ok(fused(64, 2, 2, "A"), "f32") and not ok(fused(64, 2, 2, "A"), "split6")
    p = fused(64, 2, 2, "A")
    p.store(0, e())
    assert not ok(p)
    # grouped launches never reach the matcher
    seen = []
    monkeypatch.setattr(K, "atom_stack_adjoint_match", lambda *a, **kw: seen.append(a))
    with pytest.raises(Exception):
        K.chain(fused(64, 2, 0, "N"), mode="h3", groups=2, group_pitch=64)
    assert not seen
    monkeypatch.undo()
    monkeypatch.setattr(K, "CHAIN_LAYOUT", "row")
    assert not ok(fused(64, 2, 2, "A"))


# -------------------------------------------------------------------------------------------------------- kernel, GPU
class Case:
    """Random weights, 300 benign input rows for the forward that stores the factors, and three cotangents (g, gt1, gt2) whose
    row 3 is zero, row 5 scaled by 1e-20, row 7 by 1e+20: a linear program in row-scaled planes, every row stays finite."""

    def __init__(self):
        gen = torch.Generator().manual_seed(23)
        self.W = [torch.randn(C, C, generator=gen) / C ** 0.5 for _ in range(7)]
        self.x = torch.randn(300, C, generator=gen)
        self.res2 = torch.randn(300, C, generator=gen)
        self.g = [torch.randn(300, C, generator=gen) for _ in range(3)]
        for g in self.g:
            g[3] = 0.0
            g[5] *= 1e-20
            g[7] *= 1e20
        self.factors = {}


@pytest.fixture(scope="module")
def case():
    return Case()


def _factors(case, L, T, skip):
    """ssilu' factors of all 300 rows as a real forward launch stores them (once per form, on the host)."""
    key = (L, T, skip)
    if key not in case.factors:
        Ws = [W.to(DEV) for W in case.W[:1 + 2 * L]] + [W.to(DEV) for W in case.W[5:5 + T]]
        outs = [torch.empty(300, C, device=DEV) for _ in range(2 + 2 * L + T)]
        K.chain(_forward(300, case.x.to(DEV), Ws, outs[:1 + 2 * L], outs[1 + 2 * L], outs[2 + 2 * L:], L,
                         res2=case.res2.to(DEV) if skip else None), mode="h3")
        torch.cuda.synchronize()
        case.factors[key] = [z.cpu() for z in outs[:1 + 2 * L]]
        assert all(bool(torch.isfinite(z).all()) for z in case.factors[key])
    return case.factors[key]


def _operands(case, M, L, T, form, rows=None):
    rows = slice(0, M) if rows is None else rows
    Wd = [put(W) for W in case.W[:1 + 2 * L]] + [put(W) for W in case.W[5:5 + T]]
    Wt = [W.t() for W in Wd]
    pk = [K.pack_weight_split(W, trans=True, fmt=K.SPLIT_FORMAT["h3"]) for W in Wd]
    zs = [put(z[rows].contiguous()) for z in _factors(case, L, T, form != "N")]
    g = put(case.g[0][rows].contiguous())
    gts = [put(case.g[1 + i][rows].contiguous()) for i in range(T)]
    gx = torch.full((M, C), SENTINEL, device=DEV)
    g_skip = torch.full((M, C), SENTINEL, device=DEV) if form == "A" else None
    return _adjoint(M, g, gts, Wt, zs, gx, g_skip, L, form, packed=pk), gx, g_skip


def _launch(case, M, L, T, form, on, monkeypatch, rows=None):
    """One launch of the fused adjoint on guarded tensors -> [gx, g_skip?] (each exactly M rows: the red zones begin at row M)."""
    raw, gx, g_skip = _operands(case, M, L, T, form, rows)
    p = K.fuse_program(raw)
    assert K.atom_stack_adjoint_match(p, "h3") is not None
    monkeypatch.setattr(K, "USE_ATOM_STACK_BWD", on)
    K.chain(p, mode="h3")
    torch.cuda.synchronize()
    return [gx] + ([g_skip] if g_skip is not None else [])


@gpu
@pytest.mark.parametrize("L,T,form", FORMS)
def test_every_output_is_bit_equal_to_the_chain_launch(case, L, T, form, monkeypatch, redzone):      # noqa: F811
    _factors(case, L, T, form != "N")
    for M in SIZES:
        n0 = redzone.n_launches
        new = _launch(case, M, L, T, form, True, monkeypatch)
        old = _launch(case, M, L, T, form, False, monkeypatch)
        assert redzone.n_launches - n0 == 2 * (1 + 2 * L + T + 1)               # per side: the packs and ONE launch
        assert len(new) == len(old) == 1 + (form == "A")
        for i, (a, b) in enumerate(zip(new, old)):
            assert a.shape == b.shape == (M, C) and torch.equal(a, b) and _same(a, b), (M, L, T, form, "output", i)
            # every element of every row < M written (the rows past M are the harness's red zone), and finite: the
            # program is linear and the planes are row-scaled
            assert bool(torch.isfinite(a).all()) and not bool((a == SENTINEL).any())
            if M > 7:
                assert not bool(a[3].any()) and float(a[7].abs().max()) > 1e15 and 0 < float(a[5].abs().max()) < 1e-15


@gpu
def test_rows_do_not_depend_on_their_position_or_the_row_count(case, monkeypatch, redzone):      # noqa: F811
    for T, form in ((2, "A"), (0, "A"), (2, "B")):
        full = _launch(case, 300, 2, T, form, True, monkeypatch)
        again = _launch(case, 300, 2, T, form, True, monkeypatch)
        for a, b in zip(full, again):
            assert _same(a, b)                                                    # two launches are bit-equal
        rows = torch.tensor([299, 0, 17, 16, 15, 5, 3, 7, 250, 31, 32, 100, 1, 2, 48, 64, 65])       # 17 rows: two tiles
        part = _launch(case, len(rows), 2, T, form, True, monkeypatch, rows=rows)
        for a, b in zip(part, full):
            assert _same(a, b[rows.to(DEV)])
        one = _launch(case, 1, 2, T, form, True, monkeypatch, rows=torch.tensor([299]))
        for a, b in zip(one, full):
            assert _same(a, b[299:300])


@gpu
@pytest.mark.parametrize("T,form", [(2, "A"), (2, "B")])
def test_captured_replay_equals_eager_and_is_ordered(case, T, form, monkeypatch, redzone):      # noqa: F811
    M, L = 300, 2
    eager = _launch(case, M, L, T, form, True, monkeypatch)
    raw, gx, g_skip = _operands(case, M, L, T, form)
    p = K.fuse_program(raw)
    outs = [gx] + ([g_skip] if g_skip is not None else [])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.chain(p, mode="h3")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for o in outs:
        o.fill_(float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with redzone.untraced(), hbcheck.record() as rec:      # the recorder takes the harness's tracer slot
            K.chain(p, mode="h3")
    launched = [o.name for o in rec.ops if o.name.startswith("gn_")]
    assert len(launched) == 1 and launched[0].startswith(NEW)
    races, summary = rec.races(), rec.summary()
    assert not races and summary["unresolved_pointers"] == 0 and summary["unrecorded_nodes"] == 0
    for _ in range(5):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert _same(a, b)


@gpu
def test_launcher_rejects_what_the_kernel_does_not_run(redzone):      # noqa: F811
    lib = _lib.load()
    x = torch.zeros(16, C, device=DEV)
    arr7 = (K.ctypes.c_void_p * 7)(*[x.data_ptr()] * 7)
    none7 = (K.ctypes.c_void_p * 7)()
    odd7 = (K.ctypes.c_void_p * 7)(*[x.data_ptr() + 4] * 7)
    px = _lib.ptr(x)

    def call(M=16, L=2, T=2, form=0, gt=arr7, W=arr7, F=arr7, g=px, g_skip=None, gx=px):
        return lib.gn_atom_stack_bwd_f32(g, M, L, T, form, gt, W, F, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, g_skip, gx, _lib.stream())
    bad = 1      # hipErrorInvalidValue
    assert call(M=4097) == bad
    assert call(L=0) == bad and call(L=3) == bad and call(T=1) == bad and call(T=3) == bad and call(form=2) == bad
    assert call(g=None) == bad and call(gx=None) == bad and call(W=none7) == bad and call(F=none7) == bad and call(gt=none7) == bad
    assert call(W=odd7) == bad and call(F=odd7) == bad and call(gt=odd7) == bad
    assert call(g=K.ctypes.c_void_p(x.data_ptr() + 4)) == bad and call(form=1, g_skip=K.ctypes.c_void_p(x.data_ptr() + 4)) == bad
    assert call(form=1) == bad                       # form A without g_skip
    assert call(form=0, g_skip=px) == bad            # and a g_skip nobody would write
    assert call(M=0) == 0 and call(M=0, form=1) == 0
    torch.cuda.synchronize()
    assert not bool(x.any())


# --------------------------------------------------------------------------------------------------------------- model
T2_CFG = dict(T_CFG, num_blocks=2)


@pytest.fixture(scope="module")
def t2_case():
    inputs = _molecules()
    params = GO.make_params(T2_CFG, 3, GO.load_scale_factors(SCALE_FILE))
    E_ref, F_ref = GO.forward(T2_CFG, params, inputs)          # float64 oracle, once
    return _build(T2_CFG, params), {k: v.to(DEV) for k, v in inputs.items()}, E_ref.detach().double(), F_ref.detach().double()


@gpu
def test_model_meets_the_oracle_bar_with_the_switch_on_and_off(t2_case, monkeypatch, redzone):    # noqa: F811
    model, inputs, E_ref, F_ref = t2_case
    res = {}
    for on in (False, True):
        monkeypatch.setattr(K, "USE_ATOM_STACK_BWD", on)
        model(inputs)                          # (fills the weight cache)
        E, F, names = _count(model, inputs, redzone)
        f_mae = float((F.double().cpu() - F_ref).abs().mean())
        e_err = float((E.double().cpu().reshape(E_ref.shape) - E_ref).abs().max())
        print(f"GEMNET_ATOM_STACK_BWD={int(on)}: energy err {e_err:.3e}, force MAE {f_mae:.3e} (mean |F_ref| {float(F_ref.abs().mean()):.3e}), "
              f"{names[NEW]} adjoint launches, {names[FWD]} forward launches, {names[OLD]} chain launches")
        assert f_mae <= 1e-5 * max(1.0, float(F_ref.abs().mean())) and e_err <= 2e-5 * max(1.0, float(E_ref.abs().max()))
        res[on] = (E, F, names)
    # one AtomUpdateBlock adjoint per interaction block (block 1: the skip's gradient is not wanted, block 2: it is) moves from
    # the chain launch to the new one; nothing else changes, bit for bit
    nb = T2_CFG["num_blocks"]
    assert res[False][2][NEW] == 0 and res[True][2][NEW] == nb
    assert res[True][2][OLD] == res[False][2][OLD] - nb and res[True][2][FWD] == res[False][2][FWD] == nb
    assert sum(res[True][2].values()) == sum(res[False][2].values())
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


@gpu
def test_other_passes_keep_the_chain_launches(t2_case, monkeypatch, redzone):     # noqa: F811
    monkeypatch.setattr(K, "USE_ATOM_STACK_BWD", True)
    model, inputs, _, _ = t2_case
    scale = GO.load_scale_factors(SCALE_FILE)
    monkeypatch.setattr(model, "matmul_precision", "f32")
    _, F, names = _count(model, inputs, redzone)
    assert torch.isfinite(F).all() and names[NEW] == 0 and names["gn_chain_f32"] > 0
    monkeypatch.setattr(model, "matmul_precision", None)
    model.train()          # a training step: weights with gradients, plain pre-activations stored
    try:
        E, F, names = _count(model, inputs, redzone)
        assert torch.isfinite(F).all() and names[NEW] == 0
    finally:
        model.eval()
    cfg = dict(T2_CFG, triplets_only=False, emb_size_atom=64)        # GemNet-Q with 64 atom features: another width
    qin = {k: v.to(DEV) for k, v in _molecules(False).items()}
    _, F, names = _count(_build(cfg, GO.make_params(cfg, 5, scale)), qin, redzone)
    assert torch.isfinite(F).all() and names[NEW] == 0 and names[OLD] > 0
    _, _, names = _count(model, inputs, redzone)                      # (the counter is live)
    assert names[NEW] == T2_CFG["num_blocks"]
