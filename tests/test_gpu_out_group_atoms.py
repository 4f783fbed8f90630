"""The stage of the grouped OutputBlocks on grouped launches of the two atom-row kernels (csrc/atom_stack.hip,
gn_atom_stack_fwd_grouped_f32 / gn_atom_stack_bwd_grouped_f32).  CPU: the header declares the entry points
and the binding matches; `kernels.atom_stack_grouped_match` takes exactly the programs ops._OutputGroup builds, the two ungrouped
matchers none of them.  GPU, kernel level (under the red-zone harness): L in {1, 2}, G in {1, 2, 5}, A in {1, 15, 16, 17, 33} with
group_pitch = A (the tail of a group's last tile lies on the next group's rows) against the grouped chain launch of the same
program (GEMNET_OUT_GROUP_ATOMS=0) at both of its tile heights, bit for bit; a zero row and rows scaled by 1e-20 and 1e+20 in every
group of the inputs and of the cotangent (A = 1 has one row and holds none of them); sentinels; independence of A, position and
G; determinism; the seed formed in the LOAD against gn_energy_head_bwd_f32 + the tensor LOAD; captured replay == eager under the
happens-before checker; the launchers' refusals.  Model level: the two-block GemNet-T of tests/test_gpu_atom_stack_bwd.py
against the float64 oracle with the switch on and off."""
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
FWD = "gn_atom_stack_fwd_grouped_f32"
BWD = "gn_atom_stack_bwd_grouped_f32"
OLD = "gn_chain_split_grouped_f32"
SEED = "gn_energy_head_bwd_f32"
PLANE = 65536
SENTINEL = 12345.0
LS, GS, AS = (1, 2), (1, 2, 5), (1, 15, 16, 17, 33)
GMAX, AMAX = 5, 33


# ------------------------------------------------------------------------------------------------ the programs of ops._OutputGroup
def _forward(A, x0, Ws, packed, zs0, y0, L, act0=True):
    """_OutputGroup.forward: group 0's slab of every stacked operand, the stacked planes as `packed`."""
    p = K.ChainProgram(A)
    p.load(0, x0)
    p.gemm(Ws[0], packed=packed[0], a_slot=0, y_slot=1, act=act0, pre_deriv=act0, pre_out=zs0[0] if act0 else None,
           out=None if L else y0)
    for k in range(L):
        last = k + 1 == L
        p.gemm(Ws[1 + 2 * k], packed=packed[1 + 2 * k], a_slot=1, y_slot=0, act=True, pre_out=zs0[1 + 2 * k], pre_deriv=True)
        p.gemm(Ws[2 + 2 * k], packed=packed[2 + 2 * k], a_slot=0, y_slot=1, act=True, pre_out=zs0[2 + 2 * k], pre_deriv=True, res=1,
               beta=S, out=y0 if last else None)
    return p


def _adjoint(A, g0, seed, Wt, packed, zs0, gx0, L, z0=True):
    """_OutputGroup.backward, fused: the LOAD's cotangent is group 0's slab of a tensor or, with `seed` = (g_E, w_out), a view
    that only carries the shape."""
    p = K.ChainProgram(A)
    if seed is not None:
        p.load(0, seed[1][:1].expand(A, C))
        p.ops[0]["seed"] = seed
    else:
        p.load(0, g0)
    for k in range(L - 1, -1, -1):
        p.scale(0, 0, S, width=C)
        p.scale(1, 0, 1.0, Z=zs0[2 + 2 * k], mode=1)
        p.gemm(Wt[2 + 2 * k], packed=packed[2 + 2 * k], a_slot=1, y_slot=1)
        p.scale(1, 1, 1.0, Z=zs0[1 + 2 * k], mode=1)
        p.gemm(Wt[1 + 2 * k], packed=packed[1 + 2 * k], a_slot=1, y_slot=0, res=0, beta=1.0)
    src = 0
    if z0:
        p.scale(1, 0, 1.0, Z=zs0[0], width=C, mode=1)
        src = 1
    p.gemm(Wt[0], packed=packed[0], a_slot=src, y_slot=-1, out=gx0)
    return K.fuse_program(p)


def _host_planes(G, n, fmt=1):
    out = []
    for _ in range(n):
        t = torch.empty(G, PLANE, dtype=torch.uint8)
        t._gn_fmt = fmt
        out.append(t)
    return out


def _host(kind, L, G=5, A=37, width=C, fmt=1, seed=False, **kw):
    """A forward / fused adjoint program on host tensors, as _OutputGroup builds it for G blocks of A atoms."""
    e = lambda: torch.empty(G, A, width)      # noqa: E731
    Ws = [torch.empty(width, width) for _ in range(1 + 2 * L)]
    zs = [e()[0] for _ in range(1 + 2 * L)]
    pk = _host_planes(G, 1 + 2 * L, fmt)
    if kind == "fwd":
        return _forward(A, e()[0], Ws, pk, zs, e()[0], L, **kw)
    sd = (torch.empty(A, 1), torch.empty(G, width)) if seed else None
    return _adjoint(A, e()[0], sd, [W.t() for W in Ws], pk, zs, e()[0], L, **kw)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_abi_declares_and_binds_the_entry_points():
    with open(os.path.join(ROOT, "include", "gemnet_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    kinds = hbcheck.parse_header()[0]
    for name, nargs in ((FWD, 10), (BWD, 14)):
        m = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name])
    f, b = dict(kinds[FWD]), dict(kinds[BWD])
    assert f["x"] == "r" and f["W"] == "ra" and f["z"] == "wa" and f["y"] == "w" and f["stream"] == "stream"
    assert b["g"] == "r" and b["g_E"] == "r" and b["w_out"] == "r" and b["W"] == "ra" and b["F"] == "ra" and b["gx"] == "w"
    assert K.USE_ATOM_STACK_GROUPED == (os.environ.get("GEMNET_OUT_GROUP_ATOMS", "1") == "1")       # a switch of its own


@pytest.mark.parametrize("L", LS)
def test_matcher_accepts_the_programs_of_the_output_group(L):
    for G, A in ((1, 1), (5, 37), (8, 4096)):
        p = _host("fwd", L, G, A)
        kind, m = K.atom_stack_grouped_match(p, G, A, "h3")
        assert kind == "fwd" and m["L"] == L and len(m["gemms"]) == len(m["z"]) == 1 + 2 * L and m["s"] == S
        assert m["x"] is p.ops[0]["src"] and m["y"] is p.ops[-1]["out"] and not m["t"] and m["res2"] is None
        for seed in (False, True):
            p = _host("bwd", L, G, A, seed=seed)
            kind, m = K.atom_stack_grouped_match(p, G, A, "h3")
            assert kind == "bwd" and m["L"] == L and m["form"] == 0 and not m["gt"] and m["g_skip"] is None
            assert len(m["gemms"]) == len(m["F"]) == 1 + 2 * L and m["alpha0"] == S and m["bl"][:L] == ([S, 1.0] if L == 2 else [1.0])
            assert (m["seed"] is not None) == seed and m["gx"] is p.ops[-1]["out"]
            # a seeded LOAD is never the single launch's; neither program is the forward's
            assert (K.atom_stack_adjoint_match(p, "h3") is None) == seed and K.atom_stack_match(p, "h3") is None


def test_grouped_launches_never_reach_the_ungrouped_matchers(monkeypatch):
    """A program does not say whether it is group 0 of a grouped launch (the unseeded ones above look like single launches):
    the refusal is `chain`'s, which asks the ungrouped matchers for single launches only.  On host tensors the grouped matcher
    accepts and its launcher then refuses the operands."""
    seen = []
    monkeypatch.setattr(K, "atom_stack_match", lambda *a, **kw: seen.append(a))
    monkeypatch.setattr(K, "atom_stack_adjoint_match", lambda *a, **kw: seen.append(a))
    for on in (True, False):
        monkeypatch.setattr(K, "USE_ATOM_STACK_GROUPED", on)
        for p in (_host("fwd", 2), _host("bwd", 2), _host("bwd", 2, seed=True)):
            with pytest.raises(Exception):
                K.chain(p, mode="h3", groups=5, group_pitch=37)
    assert not seen


def test_matcher_refuses_everything_else(monkeypatch):
    ok = lambda p, G=5, A=37, mode="h3", pitch=None: K.atom_stack_grouped_match(p, G, pitch or A, mode) is not None      # noqa: E731
    assert ok(_host("fwd", 2)) and ok(_host("bwd", 2)) and ok(_host("bwd", 2, seed=True))
    assert not ok(_host("fwd", 2), pitch=40) and not ok(_host("bwd", 2), pitch=40)       # slabs the operands' storage does not hold
    assert not ok(_host("fwd", 2, act0=False))                               # no activation on the first Dense
    assert not ok(_host("bwd", 2, z0=False)) and not ok(_host("bwd", 2, seed=True, z0=False))
    assert not ok(_host("fwd", 0)) and not ok(_host("bwd", 0))               # no ResidualLayer
    p = _host("fwd", 2)                                                      # a tail
    p.gemm(torch.empty(C, C), packed=_host_planes(5, 1)[0], a_slot=1, y_slot=-1, out=torch.empty(5, 37, C)[0])
    assert not ok(p)
    p = _host("fwd", 2)                                                      # a skip
    p.ops[-1].update(res2=torch.empty(5, 37, C)[0], beta2=S)
    assert not ok(p)
    p = _host("bwd", 2)                                                      # a skip's gradient as an output (form A)
    p.ops[0].update(alpha=1.0, y2=-1, Z2=None)
    assert not ok(p)
    for kind in ("fwd", "bwd"):
        assert not ok(_host(kind, 2, width=64))                              # another width
        assert not ok(_host(kind, 2, A=4097), A=4097)                        # M out of range
        q = _host(kind, 2, A=1)
        q.M = 0
        assert not ok(q, A=0) and not ok(q, A=1)
        assert not ok(_host(kind, 2), G=0) and not ok(_host(kind, 2, G=9), G=9)
        assert not ok(_host(kind, 2), pitch=36)                              # slabs that overlap
        assert not ok(_host(kind, 2), mode="f32") and not ok(_host(kind, 2), mode="split6")
        assert not ok(_host(kind, 2, fmt=0))                                 # planes of another format
        assert not ok(_host(kind, 2, G=4), G=5)                              # fewer stacked weights / slabs than groups
        q = _host(kind, 2)
        q.ops[-1]["packed"] = None
        assert not ok(q)
    assert not ok(_host("bwd", 2, G=5, seed=True), G=4)                      # w_out of another group count
    monkeypatch.setattr(K, "CHAIN_LAYOUT", "row")
    assert not ok(_host("fwd", 2)) and not ok(_host("bwd", 2))


# -------------------------------------------------------------------------------------------------------- kernel, GPU
class Case:
    """Five groups of five 128 x 128 weights; inputs, a cotangent and a per-atom seed for 33 rows per group whose row 3 is zero,
    row 5 scaled by 1e-20 and row 7 by 1e+20; benign inputs for the forward that stores the factors of the adjoint cases."""

    def __init__(self):
        gen = torch.Generator().manual_seed(31)
        rn = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
        self.W = [[rn(C, C) / C ** 0.5 for _ in range(GMAX)] for _ in range(5)]
        self.W2 = [rn(C, C) / C ** 0.5 for _ in range(5)]      # other weights for one group
        self.x, self.xb, self.g = rn(GMAX, AMAX, C), rn(GMAX, AMAX, C), rn(GMAX, AMAX, C)
        self.g_E, self.w_out = rn(AMAX, 1), rn(GMAX, C) / C ** 0.5
        for t in (self.x, self.g):
            t[:, 3] = 0.0
            t[:, 5] *= 1e-20
            t[:, 7] *= 1e20
        self.g_E[3], self.g_E[5], self.g_E[7] = 0.0, 1e-20, 1e20
        self.factors, self.packs = {}, {}


@pytest.fixture(scope="module")
def case():
    return Case()


def _weights(case, L, groups, other=None):
    """(weights, stacked planes, stacked transposed planes) of the chosen groups, `other` with weights of its own; packed once."""
    key = (L, tuple(groups), other)
    if key not in case.packs:
        Wd = [[(case.W2[j] if g == other else case.W[j][g]).to(DEV) for g in groups] for j in range(1 + 2 * L)]
        case.packs[key] = (Wd, [K.pack_weight_split_stacked(row, fmt=1) for row in Wd],
                           [K.pack_weight_split_stacked(row, trans=True, fmt=1) for row in Wd])
    return case.packs[key]


def _run(p, G, A, on, monkeypatch, tile=None):
    assert K.atom_stack_grouped_match(p, G, A, "h3") is not None
    monkeypatch.setattr(K, "USE_ATOM_STACK_GROUPED", on)
    K.chain(p, mode="h3", groups=G, group_pitch=A, tile_rows=tile)
    torch.cuda.synchronize()


def _fwd(case, L, A, groups, on, monkeypatch, tile=None, x=None, other=None, rows=None):
    """One grouped forward launch on guarded tensors -> [z..., y], each (G, A, C) exactly: the red zones begin behind the last group."""
    G = len(groups)
    rows = slice(0, A) if rows is None else rows
    Wd, pk, _ = _weights(case, L, groups, other)
    xs = put((case.x if x is None else x)[list(groups)][:, rows].contiguous())
    outs = [torch.full((G, A, C), SENTINEL, device=DEV) for _ in range(2 + 2 * L)]
    p = _forward(A, xs[0], [row[0] for row in Wd], pk, [z[0] for z in outs[:-1]], outs[-1][0], L)
    _run(p, G, A, on, monkeypatch, tile)
    return outs


def _factors(case, L, monkeypatch):
    """ssilu' factors of all groups and rows as a real forward launch stores them (once per L, on the host)."""
    if L not in case.factors:
        outs = _fwd(case, L, AMAX, range(GMAX), False, monkeypatch, x=case.xb)
        case.factors[L] = [z.cpu() for z in outs[:-1]]
        assert all(bool(torch.isfinite(z).all()) for z in case.factors[L])
    return case.factors[L]


def _bwd_program(case, L, A, groups, monkeypatch, seed=False, g=None, other=None, rows=None):
    G = len(groups)
    rows = slice(0, A) if rows is None else rows
    Wd, _, pkt = _weights(case, L, groups, other)
    Fs = [put(z[list(groups)][:, rows].contiguous()) for z in _factors(case, L, monkeypatch)]
    gx = torch.full((G, A, C), SENTINEL, device=DEV)
    gs = put((case.g if g is None else g)[list(groups)][:, rows].contiguous())
    sd = (put(case.g_E[rows].contiguous()), put(case.w_out[list(groups)].contiguous())) if seed else None
    return _adjoint(A, gs[0], sd, [row[0].t() for row in Wd], pkt, [z[0] for z in Fs], gx[0], L), gx, (gs, Fs, sd)


def _bwd(case, L, A, groups, on, monkeypatch, tile=None, **kw):
    p, gx, keep = _bwd_program(case, L, A, groups, monkeypatch, **kw)
    _run(p, len(groups), A, on, monkeypatch, tile)
    return gx


@gpu
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("L", LS)
def test_forward_is_bit_equal_to_the_grouped_chain_launch(case, L, G, monkeypatch, redzone):      # noqa: F811
    for A in AS:
        _weights(case, L, range(G))
        n0 = redzone.n_launches
        new = _fwd(case, L, A, range(G), True, monkeypatch)
        assert redzone.n_launches - n0 == 1                                       # ONE launch
        for tile in (None, 16):
            old = _fwd(case, L, A, range(G), False, monkeypatch, tile=tile)
            for i, (a, b) in enumerate(zip(new, old)):
                assert a.shape == b.shape == (G, A, C) and _same(a, b), (L, G, A, tile, "output", i)
        ok = [r for r in range(A) if r != 7]
        for a in new:
            assert bool(torch.isfinite(a[:, ok]).all()) and not bool((a == SENTINEL).any())       # every element written
        if A > 7:
            assert not bool(torch.isfinite(new[-1][:, 7]).all(1).any())          # the 1e+20 rows did leave the fp16 range


@gpu
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("L", LS)
def test_adjoint_is_bit_equal_to_the_grouped_chain_launch(case, L, G, monkeypatch, redzone):      # noqa: F811
    _factors(case, L, monkeypatch)
    for A in AS:
        _weights(case, L, range(G))
        n0 = redzone.n_launches
        new = _bwd(case, L, A, range(G), True, monkeypatch)
        assert redzone.n_launches - n0 == 1
        for tile in (None, 16):
            old = _bwd(case, L, A, range(G), False, monkeypatch, tile=tile)
            assert new.shape == old.shape == (G, A, C) and torch.equal(new, old) and _same(new, old), (L, G, A, tile)
        # a linear program in row-scaled planes: every row stays finite
        assert bool(torch.isfinite(new).all()) and not bool((new == SENTINEL).any())
        if A > 7:
            assert not bool(new[:, 3].any()) and float(new[:, 7].abs().amax(1).min()) > 1e15
            assert 0 < float(new[:, 5].abs().amax(1).min()) and float(new[:, 5].abs().max()) < 1e-15


@gpu
@pytest.mark.parametrize("L", LS)
def test_one_group_is_bit_equal_to_the_single_launch(case, L, monkeypatch, redzone):      # noqa: F811
    """The grouped launch with G = 1 and the single launch of the same program (forward: T = 0, no skip; adjoint: T = 0, no skip
    gradient) are two instances of one kernel template: y, every factor and g_x agree bit for bit.  1 row: one partial tile;
    17: a tile pair whose second half is empty; 33: two pairs."""
    single = []
    for name in ("_atom_stack_fwd", "_atom_stack_bwd"):
        launch = getattr(K, name)
        monkeypatch.setattr(K, name, lambda M, m, name=name, launch=launch: (single.append(name), launch(M, m))[1])
    monkeypatch.setattr(K, "USE_ATOM_STACK", True)
    monkeypatch.setattr(K, "USE_ATOM_STACK_BWD", True)
    Wd, pk, _ = _weights(case, L, [0])
    for A in (1, 17, 33):
        grouped = _fwd(case, L, A, [0], True, monkeypatch)
        outs = [torch.full((1, A, C), SENTINEL, device=DEV) for _ in range(2 + 2 * L)]
        xs = put(case.x[:1, :A].contiguous())
        n0 = redzone.n_launches
        K.chain(_forward(A, xs[0], [row[0] for row in Wd], pk, [z[0] for z in outs[:-1]], outs[-1][0], L), mode="h3")
        torch.cuda.synchronize()
        assert redzone.n_launches - n0 == 1 and single == ["_atom_stack_fwd"]
        for i, (a, b) in enumerate(zip(grouped, outs)):
            assert a.shape == b.shape == (1, A, C) and _same(a, b) and not bool((b == SENTINEL).any()), (L, A, "output", i)
        grouped = _bwd(case, L, A, [0], True, monkeypatch)
        p, gx, keep = _bwd_program(case, L, A, [0], monkeypatch)
        n0 = redzone.n_launches
        K.chain(p, mode="h3")
        torch.cuda.synchronize()
        assert redzone.n_launches - n0 == 1 and single == ["_atom_stack_fwd", "_atom_stack_bwd"]
        assert grouped.shape == gx.shape == (1, A, C) and _same(grouped, gx) and torch.equal(grouped, gx), (L, A)
        assert bool(torch.isfinite(gx).all()) and not bool((gx == SENTINEL).any())
        single.clear()


@gpu
def test_rows_between_the_groups_are_not_touched(case, monkeypatch, redzone):      # noqa: F811
    """group_pitch > A: the eight rows behind every group's 17 belong to nobody and keep their sentinel."""
    L, G, A, pitch = 2, 2, 17, 25
    Wd, pk, pkt = _weights(case, L, range(G))
    fac = _factors(case, L, monkeypatch)
    res = {}
    for on in (True, False):
        pad = lambda t: put(torch.cat([t[:G, :A], torch.full((G, pitch - A, C), SENTINEL)], 1).contiguous())      # noqa: E731
        xs, Fs = pad(case.x), [pad(z) for z in fac]
        sd = (put(case.g_E[:A].contiguous()), put(case.w_out[:G].contiguous()))
        outs = [torch.full((G, pitch, C), SENTINEL, device=DEV) for _ in range(3 + 2 * L)]
        pf = _forward(A, xs[0, :A], [row[0] for row in Wd], pk, [z[0, :A] for z in outs[:1 + 2 * L]], outs[1 + 2 * L][0, :A], L)
        _run(pf, G, pitch, on, monkeypatch)
        if on:      # (the seeded LOAD is the new kernel's alone; its values are compared elsewhere)
            _run(_adjoint(A, None, sd, [row[0].t() for row in Wd], pkt, [z[0, :A] for z in Fs], outs[-1][0, :A], L), G, pitch, on, monkeypatch)
        res[on] = outs
    for a, b in zip(res[True][:-1], res[False][:-1]):
        assert _same(a, b)
    for a in res[True]:
        assert bool((a[:, A:] == SENTINEL).all()) and not bool((a[:, :A] == SENTINEL).any())


@gpu
@pytest.mark.parametrize("L", LS)
def test_the_seed_formed_in_the_load_is_bit_equal_to_the_energy_head_launch(case, L, monkeypatch, redzone):      # noqa: F811
    for G in GS:
        for A in AS:
            g_y = K.energy_head_bwd(put(case.g_E[:A].contiguous()), put(case.w_out[:G].contiguous()))
            torch.cuda.synchronize()
            g_full = torch.zeros(GMAX, AMAX, C)
            g_full[:G, :A] = g_y.cpu()
            old = _bwd(case, L, A, range(G), False, monkeypatch, g=g_full)            # energy_head_bwd + the chain's tensor LOAD
            tensor = _bwd(case, L, A, range(G), True, monkeypatch, g=g_full)          # ... + the new kernel's tensor LOAD
            n0 = redzone.n_launches
            new = _bwd(case, L, A, range(G), True, monkeypatch, seed=True)
            assert redzone.n_launches - n0 == 1                                   # no seed launch, no (G, A, 128) array
            assert _same(new, old) and _same(tensor, old) and torch.equal(new, old), (L, G, A)
            assert bool(torch.isfinite(new).all()) and not bool((new == SENTINEL).any())
            if A > 7:
                assert not bool(new[:, 3].any()) and float(new[:, 7].abs().amax(1).min()) > 1e15
                assert 0 < float(new[:, 5].abs().amax(1).min()) and float(new[:, 5].abs().max()) < 1e-15
    # a seeded LOAD exists on this kernel alone: no other launch takes it quietly
    p, _, _ = _bwd_program(case, L, 17, range(2), monkeypatch, seed=True)
    monkeypatch.setattr(K, "USE_ATOM_STACK_GROUPED", False)
    with pytest.raises(RuntimeError, match="seed"):
        K.chain(p, mode="h3", groups=2, group_pitch=17)


@gpu
@pytest.mark.parametrize("A", [17, 33])
def test_a_group_moves_with_its_own_operands_only(case, A, monkeypatch, redzone):      # noqa: F811
    L, G = 2, 5
    f0 = _fwd(case, L, A, range(G), True, monkeypatch)
    b0 = _bwd(case, L, A, range(G), True, monkeypatch, seed=True)
    t0 = _bwd(case, L, A, range(G), True, monkeypatch)
    for g in (0, 2, 4):
        rest = [i for i in range(G) if i != g]
        # the other groups' inputs / cotangents are a sentinel: group g does not move
        xs, gs = torch.full((GMAX, AMAX, C), SENTINEL), torch.full((GMAX, AMAX, C), SENTINEL)
        xs[g], gs[g] = case.x[g], case.g[g]
        for a, b in zip(_fwd(case, L, A, range(G), True, monkeypatch, x=xs), f0):
            assert _same(a[g], b[g])
        assert _same(_bwd(case, L, A, range(G), True, monkeypatch, g=gs)[g], t0[g])
        # group g alone gets other weights: the other groups do not move, group g does
        f1 = _fwd(case, L, A, range(G), True, monkeypatch, other=g)
        for a, b in zip(f1, f0):
            assert _same(a[rest], b[rest])
        assert not _same(f1[-1][g], f0[-1][g])
        for kw, ref in ((dict(seed=True), b0), (dict(), t0)):
            b1 = _bwd(case, L, A, range(G), True, monkeypatch, other=g, **kw)
            assert _same(b1[rest], ref[rest]) and not _same(b1[g], ref[g])


@gpu
def test_rows_do_not_depend_on_the_row_count_their_position_or_the_group_count(case, monkeypatch, redzone):      # noqa: F811
    L = 2
    f5 = _fwd(case, L, AMAX, range(5), True, monkeypatch)
    b5 = _bwd(case, L, AMAX, range(5), True, monkeypatch, seed=True)
    for a, b in zip(_fwd(case, L, AMAX, range(5), True, monkeypatch), f5):
        assert _same(a, b)                                                        # two launches are bit-equal
    assert _same(_bwd(case, L, AMAX, range(5), True, monkeypatch, seed=True), b5)
    for g in (0, 3, 4):                                                           # a group alone against the same group inside G = 5
        for a, b in zip(_fwd(case, L, AMAX, [g], True, monkeypatch), f5):
            assert _same(a[0], b[g])
        # (alone the group is group 0 of the launch: its seed row of w_out moves with it)
        assert _same(_bwd(case, L, AMAX, [g], True, monkeypatch, seed=True)[0], b5[g])
    for A in (1, 15, 17):                                                         # another row count
        for a, b in zip(_fwd(case, L, A, range(5), True, monkeypatch), f5):
            assert _same(a, b[:, :A])
        assert _same(_bwd(case, L, A, range(5), True, monkeypatch, seed=True), b5[:, :A])
    rows = torch.tensor([32, 0, 17, 16, 15, 5, 3, 7, 25, 31, 20, 10, 1, 2, 8, 6, 30])       # 17 rows: two tiles, another position
    for a, b in zip(_fwd(case, L, len(rows), range(5), True, monkeypatch, rows=rows), f5):
        assert _same(a, b[:, rows.to(DEV)])
    assert _same(_bwd(case, L, len(rows), range(5), True, monkeypatch, seed=True, rows=rows), b5[:, rows.to(DEV)])


@gpu
def test_captured_replay_equals_eager_and_is_ordered(case, monkeypatch, redzone):      # noqa: F811
    L, G, A = 2, 5, 33
    eager_f = _fwd(case, L, A, range(G), True, monkeypatch, x=case.xb)
    eager_b = _bwd(case, L, A, range(G), True, monkeypatch, seed=True)
    # the forward's factors feed the adjoint inside one capture
    Wd, pk, pkt = _weights(case, L, range(G))
    xs = put(case.xb.contiguous())
    outs = [torch.full((G, A, C), SENTINEL, device=DEV) for _ in range(2 + 2 * L)]
    gx = torch.full((G, A, C), SENTINEL, device=DEV)
    sd = (put(case.g_E.contiguous()), put(case.w_out.contiguous()))
    pf = _forward(A, xs[0], [row[0] for row in Wd], pk, [z[0] for z in outs[:-1]], outs[-1][0], L)
    pb = _adjoint(A, None, sd, [row[0].t() for row in Wd], pkt, [z[0] for z in outs[:-1]], gx[0], L)
    monkeypatch.setattr(K, "USE_ATOM_STACK_GROUPED", True)

    def both():
        K.chain(pf, mode="h3", groups=G, group_pitch=A)
        K.chain(pb, mode="h3", groups=G, group_pitch=A)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for o in outs + [gx]:
        o.fill_(float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with redzone.untraced(), hbcheck.record() as rec:      # the recorder takes the harness's tracer slot
            both()
    launched = [o.name for o in rec.ops if o.name.startswith("gn_")]
    assert len(launched) == 2 and launched[0].startswith(FWD) and launched[1].startswith(BWD)
    races, summary = rec.races(), rec.summary()
    assert not races and summary["unresolved_pointers"] == 0 and summary["unrecorded_nodes"] == 0
    for _ in range(5):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs + [gx], eager_f + [eager_b]):
            assert _same(a, b)


@gpu
def test_launchers_reject_what_the_kernels_do_not_run(redzone):      # noqa: F811
    lib = _lib.load()
    x = torch.zeros(2, 16, C, device=DEV)                      # every input
    out = torch.full((2, 16, C), SENTINEL, device=DEV)         # every output: a launch would overwrite the sentinel
    vp = K.ctypes.c_void_p
    arr5, none5, odd5 = (vp * 5)(*[x.data_ptr()] * 5), (vp * 5)(), (vp * 5)(*[x.data_ptr() + 4] * 5)
    out5, oddo5 = (vp * 5)(*[out.data_ptr()] * 5), (vp * 5)(*[out.data_ptr() + 4] * 5)
    px, odd, po, oddo = _lib.ptr(x), vp(x.data_ptr() + 4), _lib.ptr(out), vp(out.data_ptr() + 4)

    def fwd(M=16, G=2, pitch=16, L=2, W=arr5, z=out5, xx=px, y=po):
        return lib.gn_atom_stack_fwd_grouped_f32(xx, M, G, pitch, L, W, z, 1.0, y, _lib.stream())

    def bwd(M=16, G=2, pitch=16, L=2, W=arr5, F=arr5, g=px, g_E=None, w_out=None, gx=po):
        return lib.gn_atom_stack_bwd_grouped_f32(g, g_E, w_out, M, G, pitch, L, W, F, 1.0, 1.0, 1.0, gx, _lib.stream())
    bad = 1      # hipErrorInvalidValue
    for call in (fwd, bwd):
        assert call(M=4097, pitch=4097) == bad                                   # M out of range
        assert call(G=0) == bad and call(G=9) == bad                             # G out of range
        assert call(pitch=15) == bad and call(L=0) == bad and call(L=3) == bad
        assert call(W=none5) == bad and call(W=odd5) == bad
        assert call(M=0) == 0 and call(M=-1) == 0
    assert fwd(xx=odd) == bad and fwd(y=oddo) == bad and fwd(z=oddo5) == bad and fwd(z=none5) == bad     # misaligned pointers
    assert fwd(xx=None) == bad and fwd(y=None) == bad
    assert bwd(g=odd) == bad and bwd(gx=oddo) == bad and bwd(F=odd5) == bad and bwd(F=none5) == bad and bwd(gx=None) == bad
    assert bwd(g=None) == bad                                                    # neither a cotangent nor a seed
    assert bwd(g_E=px, w_out=px) == bad                                          # both
    assert bwd(g=None, g_E=px) == bad and bwd(g=None, w_out=px) == bad           # half a seed
    assert bwd(g=None, g_E=px, w_out=odd) == bad
    torch.cuda.synchronize()
    assert not bool(x.any()) and bool((out == SENTINEL).all())                   # nothing was launched


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
        monkeypatch.setattr(K, "USE_ATOM_STACK_GROUPED", on)
        model(inputs)                          # (fills the weight cache)
        E, F, names = _count(model, inputs, redzone)
        f_mae = float((F.double().cpu() - F_ref).abs().mean())
        e_err = float((E.double().cpu().reshape(E_ref.shape) - E_ref).abs().max())
        print(f"GEMNET_OUT_GROUP_ATOMS={int(on)}: energy err {e_err:.3e}, force MAE {f_mae:.3e} (mean |F_ref| {float(F_ref.abs().mean()):.3e}), "
              f"{names[FWD]} + {names[BWD]} grouped atom-row launches, {names[OLD]} grouped chain launches, {names[SEED]} seed launches")
        assert f_mae <= 1e-5 * max(1.0, float(F_ref.abs().mean())) and e_err <= 2e-5 * max(1.0, float(E_ref.abs().max()))
        res[on] = (E, F, names)
    # the stage's two grouped chain launches move to the new kernels and the seed launch goes; nothing else changes, bit for bit
    off, new = res[False][2], res[True][2]
    assert off[FWD] == off[BWD] == 0 and off[OLD] == 2 and off[SEED] == 1
    assert new[FWD] == new[BWD] == 1 and new[OLD] == 0 and new[SEED] == 0
    assert sum(new.values()) == sum(off.values()) - 1
    assert {k: v for k, v in new.items() if k not in (FWD, BWD)} == {k: v for k, v in off.items() if k not in (OLD, SEED)}
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


@gpu
def test_other_passes_keep_the_chain_launches(t2_case, monkeypatch, redzone):     # noqa: F811
    monkeypatch.setattr(K, "USE_ATOM_STACK_GROUPED", True)
    model, inputs, _, _ = t2_case
    scale = GO.load_scale_factors(SCALE_FILE)
    monkeypatch.setattr(model, "matmul_precision", "f32")
    _, F, names = _count(model, inputs, redzone)
    assert torch.isfinite(F).all() and names[FWD] == names[BWD] == 0 and names["gn_chain_f32"] > 0
    monkeypatch.setattr(model, "matmul_precision", None)
    model.train()          # a training step: weights with gradients, plain pre-activations stored
    try:
        E, F, names = _count(model, inputs, redzone)
        assert torch.isfinite(F).all() and names[FWD] == names[BWD] == 0
    finally:
        model.eval()
    cfg = dict(T2_CFG, triplets_only=False, emb_size_atom=64)        # GemNet-Q with 64 atom features: another width
    qin = {k: v.to(DEV) for k, v in _molecules(False).items()}
    _, F, names = _count(_build(cfg, GO.make_params(cfg, 5, scale)), qin, redzone)
    assert torch.isfinite(F).all() and names[FWD] == names[BWD] == 0
    _, _, names = _count(model, inputs, redzone)                      # (the counter is live)
    assert names[FWD] == names[BWD] == 1


@gpu
def test_captured_model_step_equals_eager_and_is_ordered(t2_case, monkeypatch, redzone):      # noqa: F811
    """The whole forward+force of the fixture in one captured graph with the switch on: g_E comes from the model's own launches
    on the model's streams and the seeded LOAD reads it where energy_head_bwd used to."""
    monkeypatch.setattr(K, "USE_ATOM_STACK_GROUPED", True)
    model, inputs, _, _ = t2_case
    model.requires_grad_(False)          # inference: only dE/dR, as the captured step of bench.py
    try:
        E0, F0 = (t.detach().clone() for t in model(inputs))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                model(inputs)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            with redzone.untraced(), hbcheck.record() as rec:      # the recorder takes the harness's tracer slot
                Eg, Fg = model(inputs)
    finally:
        model.requires_grad_(True)
    names = [o.name for o in rec.ops if o.name.startswith("gn_")]
    count = lambda n: sum(x.startswith(n) for x in names)      # noqa: E731
    assert count(FWD) == 1 and count(BWD) == 1 and count(SEED) == 0 and count(OLD) == 0
    races, summary = rec.races(), rec.summary()
    print(rec.format(races))
    assert not races and summary["unresolved_pointers"] == 0 and summary["unrecorded_nodes"] == 0
    for _ in range(5):
        graph.replay()
        torch.cuda.synchronize()
        assert _same(Eg, E0) and _same(Fg, F0)
