"""The first-order adjoint of the atom-row MLP stack on its own kernel (gn_atom_stack_bwd_f32, csrc/atom_stack.hip) against
the chain launch it replaces (gn_chain_split_f32, GEMNET_ATOM_STACK_BWD=0), stand-alone: the two fused adjoint programs of the
headline's AtomUpdateBlock (2 tails + 2 ResidualLayers + Dense = 7 GEMMs of 128 x 128; form A: the skip's gradient is an output,
form B: it is not wanted) and the output-block stack (no tails, no skip), at M = 1 024 atom rows, 200 launches captured into one
graph, best of three replays, both in one session; bit-equality of gx and g_skip.  Factors from a real forward launch.
    python tools/atom_stack_bwd_bench.py [rounds] [M]
What bounds the new kernel: knock-out builds of csrc/atom_stack.hip (-DAS_BWD_EXP=1 no weight fetch, 2 no factor loads, 3 no
row-scale reductions, 4 no barriers between the ops; -DAS_BWD_AHEAD=n weight sets requested ahead), each a library of its own
next to the product library, selected with GEMNET_HIP_LIB (their outputs are NOT the product's: the bit-equality column may
say False):
    python -c "import __graft_entry__ as g; g.build_hip_library(lib='tools/exp/bin/libgemnet_hip_asb1.so',
               extra=('-DAS_BWD_EXP=1',), objdir='tools/exp/bin/obj_asb1')"
    GEMNET_HIP_LIB=tools/exp/bin/libgemnet_hip_asb1.so python tools/atom_stack_bwd_bench.py 1"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gemnet_pytorch_amd import kernels as K
from tools.gemm_bench import graph_best

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
M = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
C = 128
S = SB = 2 ** -0.5
gen = torch.Generator(device="cuda").manual_seed(0)
rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)      # noqa: E731


def program(L, T, form):
    """(fused adjoint program, outputs) as ops._Stack.backward + kernels.fuse_program build it."""
    Ws = [rn(C, C) / C ** 0.5 for _ in range(1 + 2 * L + T)]
    zs = [torch.empty(M, C, device="cuda") for _ in range(1 + 2 * L)]
    y, ts = torch.empty(M, C, device="cuda"), [torch.empty(M, C, device="cuda") for _ in range(T)]
    f = K.ChainProgram(M)
    f.load(0, rn(M, C))
    f.gemm(Ws[0], a_slot=0, y_slot=1, act=True, pre_deriv=True, pre_out=zs[0])
    for k in range(L):
        last = k + 1 == L
        f.gemm(Ws[1 + 2 * k], a_slot=1, y_slot=0, act=True, pre_deriv=True, pre_out=zs[1 + 2 * k])
        f.gemm(Ws[2 + 2 * k], a_slot=0, y_slot=1, act=True, pre_deriv=True, pre_out=zs[2 + 2 * k], res=1, beta=S,
               res2=rn(M, C) if (last and form != "N") else None, beta2=SB, out=y if last else None)
    for i in range(T):
        f.gemm(Ws[1 + 2 * L + i], a_slot=1, y_slot=-1, out=ts[i])
    K.chain(f, mode="h3")
    pk = [K.pack_weight_split(W, trans=True, fmt=K.SPLIT_FORMAT["h3"]) for W in Ws]
    Wt = [W.t() for W in Ws]
    gx = torch.empty(M, C, device="cuda")
    g_skip = torch.empty(M, C, device="cuda") if form == "A" else None
    p = K.ChainProgram(M)
    p.load(0, rn(M, C))
    for i in range(T):
        p.load(1, rn(M, C))
        p.gemm(Wt[1 + 2 * L + i], packed=pk[1 + 2 * L + i], a_slot=1, y_slot=0, res=0, beta=1.0)
    for k in range(L - 1, -1, -1):
        c = S
        if k == L - 1 and form == "A":
            p.scale(0, 0, SB, out=g_skip, width=C)
        elif k == L - 1 and form == "B":
            c = S * SB
        p.scale(0, 0, c, width=C)
        p.scale(1, 0, 1.0, Z=zs[2 + 2 * k], mode=1)
        p.gemm(Wt[2 + 2 * k], packed=pk[2 + 2 * k], a_slot=1, y_slot=1)
        p.scale(1, 1, 1.0, Z=zs[1 + 2 * k], mode=1)
        p.gemm(Wt[1 + 2 * k], packed=pk[1 + 2 * k], a_slot=1, y_slot=0, res=0, beta=1.0)
    p.scale(1, 0, 1.0, Z=zs[0], width=C, mode=1)
    p.gemm(Wt[0], packed=pk[0], a_slot=1, y_slot=-1, out=gx)
    return K.fuse_program(p), [gx] + ([g_skip] if form == "A" else [])


def run(p, on):
    K.USE_ATOM_STACK_BWD = on
    try:
        K.chain(p, mode="h3")
    finally:
        K.USE_ATOM_STACK_BWD = True


print(f"M = {M} rows, {-(-M // 16)} workgroups")
for L, T, form in ((2, 2, "A"), (2, 2, "B"), (2, 0, "N")):
    p, outs = program(L, T, form)
    assert K.atom_stack_adjoint_match(p, "h3") is not None
    run(p, False)
    old = [o.clone() for o in outs]
    for o in outs:
        o.fill_(float("nan"))
    run(p, True)
    same = all(torch.equal(a, b) for a, b in zip(old, outs))
    n = 1 + 2 * L + T
    for r in range(ROUNDS):
        t_old, t_new = graph_best(lambda: run(p, False)), graph_best(lambda: run(p, True))
        print(f"L={L} T={T} form {form} ({n} GEMMs, {len(p.ops)} ops) round {r}: chain launch {t_old:6.2f} us, atom-stack kernel "
              f"{t_new:6.2f} us ({t_old / n:.2f} -> {t_new / n:.2f} us per GEMM); outputs bit-equal: {same}")
