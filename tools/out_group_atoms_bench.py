"""The stage of the grouped OutputBlocks (ops._OutputGroup: G = 5 stacks of Dense + 2 ResidualLayers, 5 GEMMs of 128 x 128 each, on
A = 1 024 atom rows per group) on the grouped launches of the atom-row kernels (gn_atom_stack_fwd_grouped_f32 /
gn_atom_stack_bwd_grouped_f32, csrc/atom_stack.hip) against the grouped chain launches they replace (gn_chain_split_grouped_f32 at
its default tile and at 16 rows, GEMNET_OUT_GROUP_ATOMS=0), stand-alone: 200 launches captured into one graph, best of three
replays, both in one session; bit-equality of every stored factor, y and g_x.  The adjoint in both forms: its cotangent read from
the (G, A, 128) tensor that gn_energy_head_bwd_f32 writes (that launch timed beside it), and formed in the LOAD from g_E and w_out.
The same stack as ONE group of A rows on the single launches (gn_atom_stack_fwd_f32 / gn_atom_stack_bwd_f32) for the ratio
grouped / single.  Factors from a real forward launch.
    python tools/out_group_atoms_bench.py [rounds] [A] [G]
What bounds the new launches: knock-out builds of csrc/atom_stack.hip without the weight fetch (-DAS_EXP=1 -DAS_BWD_EXP=1), a
library of its own next to the product library, selected with GEMNET_HIP_LIB (its outputs are NOT the product's: the bit-equality
column says False):
    python -c "import __graft_entry__ as g; g.build_hip_library(lib='tools/exp/bin/libgemnet_hip_oga1.so',
               extra=('-DAS_EXP=1', '-DAS_BWD_EXP=1'), objdir='tools/exp/bin/obj_oga1')"
    GEMNET_HIP_LIB=tools/exp/bin/libgemnet_hip_oga1.so python tools/out_group_atoms_bench.py 1"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gemnet_pytorch_amd import kernels as K
from tools.gemm_bench import graph_best

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
A = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
G = int(sys.argv[3]) if len(sys.argv) > 3 else 5
C, L = 128, 2
S = 2 ** -0.5
gen = torch.Generator(device="cuda").manual_seed(0)
rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)      # noqa: E731
FMT = K.SPLIT_FORMAT["h3"]


def programs(G):
    """(forward, adjoint on a tensor, adjoint with the seed in its LOAD, seed launch, outputs) as ops._OutputGroup builds them."""
    Ws = [[rn(C, C) / C ** 0.5 for _ in range(G)] for _ in range(1 + 2 * L)]
    pk = [K.pack_weight_split_stacked(row, fmt=FMT) for row in Ws]
    pkt = [K.pack_weight_split_stacked(row, trans=True, fmt=FMT) for row in Ws]
    x, zs, y = rn(G, A, C), [torch.empty(G, A, C, device="cuda") for _ in range(1 + 2 * L)], torch.empty(G, A, C, device="cuda")
    f = K.ChainProgram(A)
    f.load(0, x[0])
    f.gemm(Ws[0][0], packed=pk[0], a_slot=0, y_slot=1, act=True, pre_deriv=True, pre_out=zs[0][0])
    for k in range(L):
        f.gemm(Ws[1 + 2 * k][0], packed=pk[1 + 2 * k], a_slot=1, y_slot=0, act=True, pre_deriv=True, pre_out=zs[1 + 2 * k][0])
        f.gemm(Ws[2 + 2 * k][0], packed=pk[2 + 2 * k], a_slot=0, y_slot=1, act=True, pre_deriv=True, pre_out=zs[2 + 2 * k][0], res=1,
               beta=S, out=y[0] if k + 1 == L else None)
    g_E, w_out = rn(A, 1), rn(G, C) / C ** 0.5
    g_y = K.energy_head_bwd(g_E, w_out)
    g_x = torch.empty(G, A, C, device="cuda")

    def adjoint(seed):
        p = K.ChainProgram(A)
        if seed:
            p.load(0, w_out[:1].expand(A, C))
            p.ops[0]["seed"] = (g_E, w_out)
        else:
            p.load(0, g_y[0])
        for k in range(L - 1, -1, -1):
            p.scale(0, 0, S, width=C)
            p.scale(1, 0, 1.0, Z=zs[2 + 2 * k][0], mode=1)
            p.gemm(Ws[2 + 2 * k][0].t(), packed=pkt[2 + 2 * k], a_slot=1, y_slot=1)
            p.scale(1, 1, 1.0, Z=zs[1 + 2 * k][0], mode=1)
            p.gemm(Ws[1 + 2 * k][0].t(), packed=pkt[1 + 2 * k], a_slot=1, y_slot=0, res=0, beta=1.0)
        p.scale(1, 0, 1.0, Z=zs[0][0], width=C, mode=1)
        p.gemm(Ws[0][0].t(), packed=pkt[0], a_slot=1, y_slot=-1, out=g_x[0])
        return K.fuse_program(p)
    return f, adjoint(False), adjoint(True), (lambda: K.energy_head_bwd(g_E, w_out)), zs + [y], [g_x]


def run(p, G, on, tile=None):
    K.USE_ATOM_STACK_GROUPED = on
    try:
        K.chain(p, mode="h3", groups=G, group_pitch=A, tile_rows=tile)
    finally:
        K.USE_ATOM_STACK_GROUPED = True


def single(p):
    """Group 0 of a grouped program as the single launch of the atom-row kernels (its `packed` are the stacked planes, whose
    first 64 KiB are group 0's)."""
    q = K.ChainProgram(p.M)
    q.ops = [dict(o, packed=o["packed"][0]) if o["kind"] == "gemm" else o for o in p.ops]
    for o in q.ops:
        if o["kind"] == "gemm":
            o["packed"]._gn_fmt = FMT
    return q


print(f"G = {G} groups of A = {A} rows: {G * -(-A // 16)} workgroups of 16 rows, {G * -(-A // 32)} of 32")
f, b_t, b_s, seed_launch, f_outs, b_outs = programs(G)
for p in (f, b_t, b_s):
    assert K.atom_stack_grouped_match(p, G, A, "h3") is not None
same = {}
for name, p, outs in (("forward", f, f_outs), ("adjoint", b_t, b_outs)):
    run(p, G, False)
    old = [o.clone() for o in outs]
    ok = True
    for q in ((p, b_s) if name == "adjoint" else (p,)):
        for o in outs:
            o.fill_(float("nan"))
        run(q, G, True)
        ok = ok and all(torch.equal(a, b) for a, b in zip(old, outs))
    same[name] = ok
f_1, b_1 = single(f), single(b_t)
if K.atom_stack_match(f_1, "h3") is None or K.atom_stack_adjoint_match(b_1, "h3") is None:
    raise SystemExit("the single launches do not take group 0's program")
for r in range(ROUNDS):
    t = dict(f_old=graph_best(lambda: run(f, G, False)), f_old16=graph_best(lambda: run(f, G, False, 16)),
             f_new=graph_best(lambda: run(f, G, True)), f_one=graph_best(lambda: K.chain(f_1, mode="h3")),
             b_old=graph_best(lambda: run(b_t, G, False)), b_old16=graph_best(lambda: run(b_t, G, False, 16)),
             b_new=graph_best(lambda: run(b_t, G, True)), b_seed=graph_best(lambda: run(b_s, G, True)),
             b_one=graph_best(lambda: K.chain(b_1, mode="h3")), seed=graph_best(seed_launch))
    print(f"round {r}: forward  chain grouped {t['f_old']:6.2f} us (16-row tiles {t['f_old16']:6.2f}), atom-row grouped {t['f_new']:6.2f} us, "
          f"one group alone {t['f_one']:6.2f} us (x{t['f_new'] / t['f_one']:.2f}); outputs bit-equal: {same['forward']}")
    print(f"round {r}: adjoint  chain grouped {t['b_old']:6.2f} us (16-row tiles {t['b_old16']:6.2f}), atom-row grouped {t['b_new']:6.2f} us, "
          f"seed in the LOAD {t['b_seed']:6.2f} us, one group alone {t['b_one']:6.2f} us (x{t['b_new'] / t['b_one']:.2f}); "
          f"energy_head_bwd {t['seed']:5.2f} us; outputs bit-equal: {same['adjoint']}")
    print(f"round {r}: both stage launches {t['f_old'] + t['b_old']:6.2f} -> {t['f_new'] + t['b_new']:6.2f} us "
          f"({t['f_old'] + t['b_old'] - t['f_new'] - t['b_new']:+.2f} us saved); with the seed launch "
          f"{t['f_old'] + t['b_old'] + t['seed']:6.2f} -> {t['f_new'] + t['b_seed']:6.2f} us")
