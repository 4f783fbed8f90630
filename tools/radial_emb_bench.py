"""The radial head with the edge embedding inside against the launches it replaces, on the bench batch: forward
(gn_radial_head_emb_fwd_f32 against gn_radial_head_fwd_f32 + the two atom-term GEMMs on the gathered rows + the small-K GEMM
with both gathered adds) and adjoint (gn_radial_head_emb_bwd_f32 against the adjoint GEMM of the Dense + gn_radial_head_bwd_f32),
200 launches in one graph, best of three replays, all in one session.
    python tools/radial_emb_bench.py [rounds]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd import ops
from gemnet_pytorch_amd.graph import GraphPlan
from tools.gemm_bench import graph_best
import bench

cfg = dict(bench.GEMNET_T)
torch.manual_seed(1234)
from gemnet_pytorch_amd.model.gemnet import GemNet
model = GemNet(**cfg, scale_file=bench.SCALE_FILE).to("cuda")
inputs, _ = bench.make_batch(cfg, 32, 32, 0, "cuda")
plan = GraphPlan.from_inputs(inputs, True)
R = inputs["R"].float().contiguous()
ic, ia, zrow = plan.id_c.idx32, plan.id_a.idx32, plan.z_rows.idx32
E, A = ic.shape[0], R.shape[0]
b3 = model.cbf_basis3
freq, z, nrm, cutoff, p = model.rbf_basis.frequencies.detach(), b3.z_ln, b3.n_ln, float(b3.cutoff), int(b3.p)
wcat = K.radial_head_weights(*[d.weight.detach() for d in (model.mlp_rbf3, model.mlp_rbf_h, model.mlp_rbf_out)],
                             model.mlp_cbf3.weight.detach())
emb, W = model.atom_emb.embeddings.weight.detach(), model.edge_emb.dense.weight.detach()
NE = 128
T_c, T_a, W_r = ops._make_atom_tables(emb, W, NE)
Wc, Wa, Wm = W[:, :NE].contiguous(), W[:, NE:2 * NE].contiguous(), W[:, 2 * NE:]
h = K.gather(emb, zrow)
g = torch.Generator(device="cuda").manual_seed(0)
rn = lambda *s: torch.randn(*s, device="cuda", generator=g)      # noqa: E731
g3, gh, go, gW1, ga = rn(E, 16), rn(E, 16), rn(E, 16), rn(E, 7, 16), rn(E, NE)
print(f"E={E} atoms={A}")


def old_fwd():
    rbf, rbf3, rbf_h, rbf_out, rbf_W1 = K.radial_head_fwd(R, ic, ia, freq, z, nrm, wcat, cutoff, p)
    g1, g2 = K.gemm(h, Wc), K.gemm(h, Wa)
    m, z0 = K.gemm(rbf, Wm, act=True, pre_out=True, gadd1=g1, gidx1=ic, gadd2=g2, gidx2=ia)
    return m, z0


def new_fwd():
    return K.radial_head_emb_fwd(R, ic, ia, freq, z, nrm, wcat, zrow, T_c, T_a, W_r, cutoff, p)


m_old, z0 = old_fwd()
m_new, d0 = new_fwd()[:2]


def old_bwd():
    g_rbf = K.gemm(ga, W_r, a_dact_pre=z0)
    return K.radial_head_bwd(g_rbf, g3, gh, go, gW1, R, ic, ia, freq, z, nrm, wcat, cutoff, p)


def new_bwd():
    return K.radial_head_emb_bwd(None, g3, gh, go, gW1, ga, None, d0, W_r, R, ic, ia, freq, z, nrm, wcat, cutoff, p)


for _ in range(int(sys.argv[1]) if len(sys.argv) > 1 else 3):
    for name, fn in (("forward: head only (gn_radial_head_fwd_f32)           ", lambda: K.radial_head_fwd(R, ic, ia, freq, z, nrm, wcat, cutoff, p)),
                     ("forward: head + 2 atom-term GEMMs + small-K GEMM       ", old_fwd),
                     ("forward: head with the embedding inside                ", new_fwd),
                     ("adjoint: old kernel only, four cotangents              ", lambda: K.radial_head_bwd(None, g3, gh, go, gW1, R, ic, ia, freq, z, nrm, wcat, cutoff, p)),
                     ("adjoint: Dense adjoint GEMM + old kernel               ", old_bwd),
                     ("adjoint: kernel with the embedding adjoint inside      ", new_bwd)):
        print(f"{name}: {graph_best(fn):7.2f} us (200 launches in one graph, best of 3)")
W_old, W_new = old_bwd(), new_bwd()
print(f"m0 bit-equal: {torch.equal(m_old, m_new)}; max |W new - W old| {float((W_new - W_old).abs().max()):.3e} at max |W| "
      f"{float(W_old.abs().max()):.3e}")
