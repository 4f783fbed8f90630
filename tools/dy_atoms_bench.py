"""The triplet Y gradient of four blocks on the bench batch: the per-edge launch (gn_bil_dy_multi_f32) against the per-atom
matrix-core launch (gn_bil_dy_atoms_f32), 200 launches in one graph, best of three replays, both in one session.
    python tools/dy_atoms_bench.py [rounds]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd.graph import GraphPlan
from tools.gemm_bench import graph_best
import bench

cfg = {"cutoff": 5.0, "int_cutoff": 10.0, "triplets_only": True}
inputs, _ = bench.make_batch(cfg, 32, 32, 0, "cuda")
sp = GraphPlan(inputs, True).trip
rows, off, _, _, max_rows = sp.groups
n = (off[1:] - off[:-1]).to(torch.int64)
E, T, NB = sp.n_reduce, sp.size, 4
print(f"E={E} T={T} atoms={n.shape[0]} max_rows={max_rows} mean in-degree {float(n.float().mean()):.1f}; "
      f"atoms with > 16 in-edges: {int((n > 16).sum())}, with 7n > 128 (two output tiles per wave): {int((7 * n > 128).sum())}, "
      f"with > 32: {int((n > 32).sum())}")
g = torch.Generator(device="cuda").manual_seed(0)
dS = [torch.randn(E, 7, 64, device="cuda", generator=g) for _ in range(NB)]
xs = [torch.randn(E, 64, device="cuda", generator=g) for _ in range(NB)]
sp.group_entries        # (built before the timed launches)
out = {}
for _ in range(int(sys.argv[1]) if len(sys.argv) > 1 else 2):
    for on, name in ((False, "per-edge launch (GEMNET_DY_ATOMS=0)"), (True, "per-atom matrix-core launch        ")):
        K.USE_DY_ATOMS = on            # (read at call time: GEMNET_DY_ATOMS only sets its initial value)
        out[on] = K.bil_dy_multi(dS, xs, sp)
        print(f"{name}: {graph_best(lambda: K.bil_dy_multi(dS, xs, sp)):7.2f} us (200 launches in one graph, best of 3)")
d = (out[True] - out[False]).abs()
print(f"max |new - per-edge| {float(d.max()):.3e} at max |dY| {float(out[False].abs().max()):.3e}; bit-equal: "
      f"{torch.equal(out[True], out[False])}")
