"""The forward of the atom-row MLP stack on its own kernel (csrc/atom_stack.hip).  CPU: the header
declares the entry point and the binding matches; the matcher of `kernels.chain` takes exactly the programs the kernel runs.
GPU, kernel level (under the red-zone harness): every (layers, tails, final skip) form at row counts below, at and above one
16-row tile against the chain launch of the same program (GEMNET_ATOM_STACK=0), bit for bit — outputs, tails and every stored
derivative factor; rows of extreme scale and a zero row; row independence; determinism; the stored factors under the old
adjoint program; captured replay == eager under the happens-before checker.  Model level: the one-block GemNet-T against the
float64 oracle with the switch on and off; the passes that keep the chain launches."""
import collections
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, SCALE_FILE
from gemnet_pytorch_amd import _lib, hbcheck
from gemnet_pytorch_amd import kernels as K
from oracle import gemnet_oracle as GO
from oracle import index_oracle as IO
from redzone import put, redzone  # noqa: F401  (autouse: every test of this module runs under the red-zone harness)

gpu = pytest.mark.gpu
DEV = "cuda"
C = 128
S = 2 ** -0.5
NEW = "gn_atom_stack_fwd_f32"
OLD = "gn_chain_split_f32"
# (layers, tails, final skip): every form the matcher accepts
FORMS = [(L, T, skip) for L in (0, 1, 2) for T in (0, 1, 2) for skip in ((False, True) if L else (False,))]
SIZES = [1, 15, 16, 17, 33, 300]


def _program(M, x, Ws, zs, y, ts, L, res2=None, packed=None, width=C, deriv=True):
    """What ops._Stack.forward builds for an AtomUpdateBlock: Dense, L ResidualLayers, the skip on the last op, tails."""
    pk = packed or [None] * len(Ws)
    p = K.ChainProgram(M)
    p.load(0, x)
    p.gemm(Ws[0], packed=pk[0], a_slot=0, y_slot=1, act=True, pre_deriv=deriv, pre_out=zs[0], out=None if L else y)
    for k in range(L):
        last = k + 1 == L
        p.gemm(Ws[1 + 2 * k], packed=pk[1 + 2 * k], a_slot=1, y_slot=0, act=True, pre_deriv=deriv, pre_out=zs[1 + 2 * k])
        p.gemm(Ws[2 + 2 * k], packed=pk[2 + 2 * k], a_slot=0, y_slot=1, act=True, pre_deriv=deriv, pre_out=zs[2 + 2 * k], res=1,
               beta=S, res2=res2 if last else None, beta2=0.8, out=y if last else None)
    for i, t in enumerate(ts):
        p.gemm(Ws[1 + 2 * L + i], packed=pk[1 + 2 * L + i], a_slot=1, y_slot=-1, out=t)
    return p


def _host_program(M, L, T, skip, width=C, **kw):
    e = lambda: torch.empty(M, width)      # noqa: E731
    Ws = [torch.empty(width, width) for _ in range(1 + 2 * L + T)]
    return _program(M, e(), Ws, [e() for _ in range(1 + 2 * L)], e(), [e() for _ in range(T)], L, res2=e() if skip else None,
                    width=width, **kw)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_abi_declares_and_binds_the_entry_point():
    with open(os.path.join(ROOT, "include", "gemnet_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(NEW + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{NEW} is not declared"
    assert len(m.group(1).split(",")) == 12 == len(_lib.SIGNATURES[NEW])
    kinds = dict(hbcheck.parse_header()[0][NEW])
    assert kinds["W"] == "ra" and kinds["z"] == "wa" and kinds["t"] == "wa" and kinds["x"] == "r" and kinds["res2"] == "r"
    assert kinds["y"] == "w" and kinds["stream"] == "stream"


@pytest.mark.parametrize("L,T,skip", FORMS)
def test_matcher_accepts_the_forms_of_the_atom_stack(L, T, skip):
    for M in (1, 1024, 4096):
        p = _host_program(M, L, T, skip)
        m = K.atom_stack_match(p, "h3")
        assert m is not None and m["L"] == L and len(m["t"]) == T and (m["res2"] is not None) == skip
        assert len(m["gemms"]) == 1 + 2 * L + T and len(m["z"]) == 1 + 2 * L and m["s"] == (S if L else 1.0)
        assert m["beta2"] == (0.8 if skip else 1.0) and m["y"] is p.ops[1 + 2 * L]["out"] and m["x"] is p.ops[0]["src"]


def test_matcher_refuses_everything_else(monkeypatch):
    ok = lambda p, mode="h3": K.atom_stack_match(p, mode) is not None      # noqa: E731
    assert ok(_host_program(64, 2, 2, True))
    assert not ok(_host_program(64, 2, 2, True, width=64))                     # width 64
    assert not ok(_host_program(64, 2, 2, True), "f32") and not ok(_host_program(64, 2, 2, True), "split6")
    assert not ok(_host_program(4097, 2, 2, True))                             # beyond the 16-row launches of the chain kernel
    assert not ok(_host_program(64, 2, 2, True, deriv=False))                  # plain z stored: the training programs
    e = lambda: torch.empty(64, C)      # noqa: E731
    rows = torch.zeros(64, dtype=torch.int32)

    def changed(i, **kw):
        p = _host_program(64, 2, 2, True)
        p.ops[i].update(kw)
        return p
    assert not ok(changed(1, gadd1=e(), gidx1=rows))                           # a gathered add
    assert not ok(changed(1, res=e())) and not ok(changed(1, res=e(), res_rows=rows))     # residuals of the Dense
    assert not ok(changed(3, res2=e()))                                        # a skip that is not on the last op
    assert not ok(changed(3, res=e()))                                         # a global residual in place of the LDS one
    assert not ok(changed(5, beta=0.5))                                        # layers with different scales
    assert not ok(changed(2, mul=e())) and not ok(changed(5, y2=0)) and not ok(changed(5, out2=e()))
    assert not ok(changed(0, rows=rows)) and not ok(changed(0, alpha=2.0))
    assert not ok(changed(6, act=True)) and not ok(changed(6, a_slot=0))
    # the adjoint programs: a parked skip (register slot 2), stand-alone SCALE ops, a STORE
    p = _host_program(64, 2, 0, False)
    p.scale(2, 1, 0.5, width=C)
    assert not ok(p)
    p = _host_program(64, 1, 0, False)
    p.store(1, e())
    assert not ok(p)
    p = K.ChainProgram(64)
    p.load(0, e())
    p.scale(1, 0, 1.0, Z=e(), mode=1)
    p.gemm(torch.empty(C, C), a_slot=1, y_slot=-1, out=e())
    assert not ok(p)
    # six main GEMMs / three tails / no Dense
    p = _host_program(64, 2, 2, False)
    p.gemm(torch.empty(C, C), a_slot=1, y_slot=-1, out=e())
    assert not ok(p)
    monkeypatch.setattr(K, "CHAIN_LAYOUT", "row")
    assert not ok(_host_program(64, 2, 2, True))


# -------------------------------------------------------------------------------------------------------- kernel, GPU
class Case:
    """Random weights and 300 input rows; row 3 is zero, row 5 scaled by 1e-20, row 7 by 1e+20 (beyond the fp16 planes: inf
    and NaN, the same in both launches)."""

    def __init__(self):
        g = torch.Generator().manual_seed(11)
        self.W = [torch.randn(C, C, generator=g) / C ** 0.5 for _ in range(7)]
        x = torch.randn(300, C, generator=g)
        x[3] = 0.0
        x[5] *= 1e-20
        x[7] *= 1e20
        self.x = x
        self.res2 = torch.randn(300, C, generator=g)


@pytest.fixture(scope="module")
def case():
    return Case()


def _launch(case, M, L, T, skip, on, monkeypatch, rows=None):
    """One launch on guarded tensors -> [z..., y, t...] (each exactly M rows: the red zones begin at row M)."""
    rows = slice(0, M) if rows is None else rows
    Ws = [put(W) for W in case.W[:1 + 2 * L]] + [put(W) for W in case.W[5:5 + T]]
    pk = [K.pack_weight_split(W, fmt=K.SPLIT_FORMAT["h3"]) for W in Ws]
    x, res2 = put(case.x[rows].contiguous()), put(case.res2[rows].contiguous())
    outs = [torch.empty(M, C, device=DEV) for _ in range(2 + 2 * L + T)]
    p = _program(M, x, Ws, outs[:1 + 2 * L], outs[1 + 2 * L], outs[2 + 2 * L:], L, res2=res2 if skip else None, packed=pk)
    assert K.atom_stack_match(p, "h3") is not None
    monkeypatch.setattr(K, "USE_ATOM_STACK", on)
    K.chain(p, mode="h3")
    torch.cuda.synchronize()
    return outs, p


def _same(a, b):
    """Bit for bit; two NaNs count as equal whatever their payload."""
    return bool(((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


@gpu
@pytest.mark.parametrize("L,T,skip", FORMS)
def test_every_output_is_bit_equal_to_the_chain_launch(case, L, T, skip, monkeypatch, redzone):      # noqa: F811
    for M in SIZES:
        n0 = redzone.n_launches
        new, _ = _launch(case, M, L, T, skip, True, monkeypatch)
        old, _ = _launch(case, M, L, T, skip, False, monkeypatch)
        assert redzone.n_launches - n0 == 2 * (1 + 1 + 2 * L + T)        # per side: the packs and ONE launch
        for i, (a, b) in enumerate(zip(new, old)):
            assert a.shape == b.shape and _same(a, b), (M, L, T, skip, "output", i)
        ok = [r for r in range(M) if r != 7]
        assert all(bool(torch.isfinite(a[ok]).all()) for a in new)                # every element written
        if M > 7:
            assert not bool(torch.isfinite(new[1 + 2 * L][7]).all())              # the 1e+20 row did leave the fp16 range


@gpu
def test_rows_do_not_depend_on_their_position_or_the_row_count(case, monkeypatch, redzone):      # noqa: F811
    full, _ = _launch(case, 300, 2, 2, True, True, monkeypatch)
    again, _ = _launch(case, 300, 2, 2, True, True, monkeypatch)
    for a, b in zip(full, again):
        assert _same(a, b)                                                        # two launches are bit-equal
    rows = torch.tensor([299, 0, 17, 16, 15, 5, 3, 7, 250, 31, 32, 100, 1, 2, 48, 64, 65])       # 17 rows: two tiles
    part, _ = _launch(case, len(rows), 2, 2, True, True, monkeypatch, rows=rows)
    for a, b in zip(part, full):
        assert _same(a, b[rows.to(DEV)])
    one, _ = _launch(case, 1, 2, 2, True, True, monkeypatch, rows=torch.tensor([299]))
    for a, b in zip(one, full):
        assert _same(a, b[299:300])


@gpu
def test_stored_factors_are_what_the_adjoint_program_consumes(case, monkeypatch, redzone):      # noqa: F811
    """The adjoint program of ops._Stack.backward (chain launch) on the factors the new forward stored against the same
    program on the chain forward's factors, and the factors against float64."""
    M, L = 33, 2
    gx = {}
    for on in (True, False):
        outs, p = _launch(case, M, L, 0, False, on, monkeypatch)
        zs = outs[:5]
        Ws = [o["W"] for o in p.ops[1:]]
        g = put(torch.randn(M, C, generator=torch.Generator().manual_seed(2)))
        gx[on] = torch.empty(M, C, device=DEV)
        q = K.ChainProgram(M)
        q.load(0, g)
        for k in (1, 0):
            q.scale(0, 0, S, width=C)
            q.scale(1, 0, 1.0, Z=zs[2 + 2 * k], mode=1)
            q.gemm(Ws[2 + 2 * k].t().contiguous(), a_slot=1, y_slot=1)
            q.scale(1, 1, 1.0, Z=zs[1 + 2 * k], mode=1)
            q.gemm(Ws[1 + 2 * k].t().contiguous(), a_slot=1, y_slot=0, res=0, beta=1.0)
        q.scale(1, 0, 1.0, Z=zs[0], width=C, mode=1)
        q.gemm(Ws[0].t().contiguous(), a_slot=1, y_slot=-1, out=gx[on])
        K.chain(K.fuse_program(q), mode="h3")
        torch.cuda.synchronize()
        if on:
            # d0 = ssilu'(x W0^T): the split operands carry 22 bits, the dot product of 128 terms of magnitude |x| |w|
            # accumulates in fp32 -> |dz| <= 2^-20 * sum |x w|, and |ssilu''| <= 0.84 (plus one fp32 rounding of the factor)
            x64, W64 = case.x[:M].double(), case.W[0].double()
            z = x64 @ W64.t()
            s = torch.sigmoid(z)
            ref = s * (1 + z * (1 - s)) / 0.6
            bound = 0.84 * 2.0 ** -20 * (x64.abs() @ W64.abs().t()) + 2.0 ** -22
            err = (zs[0].double().cpu() - ref).abs()
            keep = [r for r in range(M) if r != 7]
            print(f"stored factor of the Dense: max err / bound {float((err[keep] / bound[keep]).max()):.3f}")
            assert (err[keep] <= bound[keep]).all()
    assert _same(gx[True], gx[False]) and bool(torch.isfinite(gx[True][:7]).all())


@gpu
def test_captured_replay_equals_eager_and_is_ordered(case, monkeypatch, redzone):      # noqa: F811
    M, L, T = 300, 2, 2
    eager, _ = _launch(case, M, L, T, True, True, monkeypatch)
    Ws = [put(W) for W in case.W]
    pk = [K.pack_weight_split(W, fmt=K.SPLIT_FORMAT["h3"]) for W in Ws]
    x, res2 = put(case.x[:M].contiguous()), put(case.res2[:M].contiguous())
    outs = [torch.empty(M, C, device=DEV) for _ in range(2 + 2 * L + T)]
    p = _program(M, x, Ws, outs[:5], outs[5], outs[6:], L, res2=res2, packed=pk)
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
    arr = (K.ctypes.c_void_p * 1)(x.data_ptr())
    call = lambda M, L, T, res2=None: lib.gn_atom_stack_fwd_f32(_lib.ptr(x), M, L, T, arr, arr, 1.0, res2, 1.0, _lib.ptr(x), arr,   # noqa: E731
                                                                _lib.stream())
    assert call(4097, 0, 0) == 1 and call(16, 3, 0) == 1 and call(16, 0, 3) == 1 and call(16, 0, 0, _lib.ptr(x)) == 1      # hipErrorInvalidValue
    assert call(0, 0, 0) == 0


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


def _molecules(triplets_only=True):
    from gemnet_pytorch_amd.synthetic import make_molecule
    sizes = [8, 8]
    mols = [make_molecule(n, 200 + i) for i, n in enumerate(sizes)]
    R, Z = np.concatenate([m["R"] for m in mols]), np.concatenate([m["Z"] for m in mols])
    idx = IO.build_indices(R, np.array(sizes), 5.0, 10.0, triplets_only)
    inputs = {k: torch.tensor(v) for k, v in idx.items()}
    inputs.update(Z=torch.tensor(Z).long(), R=torch.tensor(R), N=torch.tensor(sizes))
    return inputs


@pytest.fixture(scope="module")
def t_case():
    inputs = _molecules()
    params = GO.make_params(T_CFG, 1, GO.load_scale_factors(SCALE_FILE))
    E_ref, F_ref = GO.forward(T_CFG, params, inputs)          # float64 oracle, once
    return _build(T_CFG, params), {k: v.to(DEV) for k, v in inputs.items()}, E_ref.detach().double(), F_ref.detach().double()


@gpu
def test_model_meets_the_oracle_bar_with_the_switch_on_and_off(t_case, monkeypatch, redzone):    # noqa: F811
    model, inputs, E_ref, F_ref = t_case
    res = {}
    for on in (False, True):
        monkeypatch.setattr(K, "USE_ATOM_STACK", on)
        model(inputs)                          # (fills the weight cache)
        E, F, names = _count(model, inputs, redzone)
        f_mae = float((F.double().cpu() - F_ref).abs().mean())
        e_err = float((E.double().cpu().reshape(E_ref.shape) - E_ref).abs().max())
        print(f"GEMNET_ATOM_STACK={int(on)}: energy err {e_err:.3e}, force MAE {f_mae:.3e} (mean |F_ref| {float(F_ref.abs().mean()):.3e}), "
              f"{names[NEW]} atom-stack launches, {names[OLD]} chain launches")
        assert f_mae <= 1e-5 * max(1.0, float(F_ref.abs().mean())) and e_err <= 2e-5 * max(1.0, float(E_ref.abs().max()))
        res[on] = (E, F, names)
    # one AtomUpdateBlock per interaction block moves from the chain launch to the new one; nothing else changes, bit for bit
    assert res[False][2][NEW] == 0 and res[True][2][NEW] == T_CFG["num_blocks"]
    assert res[True][2][OLD] == res[False][2][OLD] - T_CFG["num_blocks"]
    assert sum(res[True][2].values()) == sum(res[False][2].values())
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


@gpu
def test_other_passes_keep_the_chain_launches(t_case, monkeypatch, redzone):     # noqa: F811
    monkeypatch.setattr(K, "USE_ATOM_STACK", True)
    model, inputs, _, _ = t_case
    scale = GO.load_scale_factors(SCALE_FILE)
    # matmul_precision = "f32"
    monkeypatch.setattr(model, "matmul_precision", "f32")
    _, F, names = _count(model, inputs, redzone)
    assert torch.isfinite(F).all() and names[NEW] == 0 and names["gn_chain_f32"] > 0
    monkeypatch.setattr(model, "matmul_precision", None)
    # a training step: weights with gradients, plain pre-activations stored
    model.train()
    try:
        E, F, names = _count(model, inputs, redzone)
        assert torch.isfinite(F).all() and names[NEW] == 0
    finally:
        model.eval()
    # GemNet-Q with 64 atom features: another width
    cfg = dict(T_CFG, triplets_only=False, emb_size_atom=64)
    qin = {k: v.to(DEV) for k, v in _molecules(False).items()}
    _, F, names = _count(_build(cfg, GO.make_params(cfg, 5, scale)), qin, redzone)
    assert torch.isfinite(F).all() and names[NEW] == 0 and names[OLD] > 0
    # (and the molecular model does take the path: the counter is live)
    _, _, names = _count(model, inputs, redzone)
    assert names[NEW] == T_CFG["num_blocks"]
