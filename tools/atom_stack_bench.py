"""The forward of the atom-row MLP stack on its own kernel (gn_atom_stack_fwd_f32, csrc/atom_stack.hip) against the chain
launch it replaces (gn_chain_split_f32, GEMNET_ATOM_STACK=0), stand-alone: the AtomUpdateBlock program of the headline
(Dense + 2 ResidualLayers + final skip + 2 tail projections = 7 GEMMs of 128 x 128) and the shorter forms, at M = 1 024 atom
rows, 200 launches captured into one graph, best of three replays, both in one session; bit-equality of every output.
    python tools/atom_stack_bench.py [rounds] [M]
What bounds the new kernel: knock-out builds of csrc/atom_stack.hip (-DAS_EXP=1 no weight fetch, 2 no activation arithmetic,
3 no MFMAs, 4 no barriers between the ops; -DAS_AHEAD=n weight sets requested ahead), each a library of its own next to the
product library, selected with GEMNET_HIP_LIB (their outputs are NOT the product's: the bit-equality column says False):
    python -c "import __graft_entry__ as g; g.build_hip_library(lib='tools/exp/bin/libgemnet_hip_as1.so',
               extra=('-DAS_EXP=1',), objdir='tools/exp/bin/obj_as1')"
    GEMNET_HIP_LIB=tools/exp/bin/libgemnet_hip_as1.so python tools/atom_stack_bench.py 1"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gemnet_pytorch_amd import kernels as K
from tools.gemm_bench import graph_best

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
M = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
C = 128
g = torch.Generator(device="cuda").manual_seed(0)
rn = lambda *s: torch.randn(*s, device="cuda", generator=g)      # noqa: E731


def program(L, T, skip):
    x, res2 = rn(M, C), rn(M, C)
    Ws = [rn(C, C) / C ** 0.5 for _ in range(1 + 2 * L + T)]
    pk = [K.pack_weight_split(W, fmt=K.SPLIT_FORMAT["h3"]) for W in Ws]
    outs = [torch.empty(M, C, device="cuda") for _ in range(2 + 2 * L + T)]
    zs, y, ts = outs[:1 + 2 * L], outs[1 + 2 * L], outs[2 + 2 * L:]
    p = K.ChainProgram(M)
    p.load(0, x)
    p.gemm(Ws[0], packed=pk[0], a_slot=0, y_slot=1, act=True, pre_deriv=True, pre_out=zs[0], out=None if L else y)
    for k in range(L):
        last = k + 1 == L
        p.gemm(Ws[1 + 2 * k], packed=pk[1 + 2 * k], a_slot=1, y_slot=0, act=True, pre_deriv=True, pre_out=zs[1 + 2 * k])
        p.gemm(Ws[2 + 2 * k], packed=pk[2 + 2 * k], a_slot=0, y_slot=1, act=True, pre_deriv=True, pre_out=zs[2 + 2 * k], res=1,
               beta=2 ** -0.5, res2=res2 if (last and skip) else None, beta2=2 ** -0.5, out=y if last else None)
    for i in range(T):
        p.gemm(Ws[1 + 2 * L + i], packed=pk[1 + 2 * L + i], a_slot=1, y_slot=-1, out=ts[i])
    return p, outs


def run(p, on):
    K.USE_ATOM_STACK = on
    try:
        K.chain(p, mode="h3")
    finally:
        K.USE_ATOM_STACK = True


print(f"M = {M} rows, {-(-M // 16)} workgroups")
for L, T, skip in ((2, 2, True), (2, 0, False), (1, 0, False), (0, 0, False)):
    p, outs = program(L, T, skip)
    assert K.atom_stack_match(p, "h3") is not None
    run(p, False)
    old = [o.clone() for o in outs]
    for o in outs:
        o.fill_(float("nan"))
    run(p, True)
    same = all(torch.equal(a, b) for a, b in zip(old, outs))
    n = 1 + 2 * L + T
    for r in range(ROUNDS):
        t_old, t_new = graph_best(lambda: run(p, False)), graph_best(lambda: run(p, True))
        print(f"L={L} T={T} skip={int(skip)} ({n} GEMMs) round {r}: chain launch {t_old:6.2f} us, atom-stack kernel {t_new:6.2f} us "
              f"({t_old / n:.2f} -> {t_new / n:.2f} us per GEMM); outputs bit-equal: {same}")
