"""Index construction time for the headline batch: device builder (csrc/index_gpu.hip) vs host builder.

`--ragged` times the force evaluation on a loader's batches: 32 molecules per batch whose sizes are drawn per batch from
{16, 24, 32} atoms, the 4-block GemNet-T of the headline at cutoff 5.0, four routes alternating in one process, three rounds:
  ragged_eager_ms    a DeviceGraphBuilder constructed per batch + the eager model
  ragged_padded_ms   the same builder + PaddedGraphRunner(a_cap=)(R, idx, Z=, N=): one graph, lists handed in
  ragged_graph_ms    run_positions(R, Z=, N=): layout, lists, plan and model in one replay (DeviceCapacityGraphBuilder)
  fixed_graph_ms     the floor: a fixed-layout run_positions at the same capacities on batches of 32 x 32 atoms
The edge / triplet capacities come from the first 8 of 16 batches and from the floor's 32 x 32 batches, which must fit the same
capacities (PaddedGraphRunner.suggest_capacities); a_cap = 32 x 32 atoms, n_max = 32; later batches that do not fit are left out
of the stream (`batches_left_out`).  One JSON line: the medians with the rounds beside them,
the shares of filler atoms / pad edges / pad triplets, the peak memory.  `--only ROUTE` runs one route alone (kernel trace).

`--ragged --quad` does the same for a 4-block GemNet-Q (the first three routes; DeviceCapacityQuadGraphBuilder, all sixteen lists
inside the replay).  The interaction cutoff is the largest of INT_CUTOFFS whose quadruplet capacity stays below 3e7; all five
capacities come from the first 8 of 16 batches.  The JSON line also holds the pad shares of all five families and whether the range
flag tripped (pad quadruplets summed on few pad edges have pushed a periodic model off the fp16 planes before)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gemnet_pytorch_amd.synthetic import make_dataset, make_molecule
from gemnet_pytorch_amd.index_device import DeviceCapacityGraphBuilder, DeviceCapacityQuadGraphBuilder, DeviceGraphBuilder
from gemnet_pytorch_amd.training.data_container import build_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMNET_T = dict(num_spherical=7, num_radial=6, num_blocks=4, emb_size_atom=128, emb_size_edge=128, emb_size_trip=64,
                emb_size_quad=32, emb_size_rbf=16, emb_size_cbf=16, emb_size_sbf=32, emb_size_bil_trip=64, emb_size_bil_quad=32,
                num_before_skip=1, num_after_skip=1, num_concat=1, num_atom=2, triplets_only=True, cutoff=5.0)
IDX_KEYS = ("id_c", "id_a", "id_swap", "id_undir", "id3_reduce_ca", "id3_expand_ba")
INT_CUTOFFS = (10.0, 8.0, 6.0, 5.0, 4.5, 4.0, 3.5, 3.0, 2.5)       # --quad: candidates, largest first
Q_CAP_LIMIT = 3e7


def build_times():
    for n_atoms, B in ((32, 32), (64, 8)):
        data = make_dataset(B, n_atoms=n_atoms)
        R = torch.tensor(data["R"], device="cuda")
        for to in (True, False):
            bld = DeviceGraphBuilder(data["N"], 5.0, 10.0, to)
            out = bld(R, dtype=torch.int32); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                out = bld(R, dtype=torch.int32)
            torch.cuda.synchronize()
            tg = (time.perf_counter() - t0) / 10
            t0 = time.perf_counter()
            ref = build_indices(data["R"], data["N"], 5.0, 10.0, to)
            th = time.perf_counter() - t0
            same = all(np.array_equal(out[k].cpu().numpy(), ref[k]) for k in ref)
            sizes = {k: int(out[k].numel()) for k in ("id_a", "id3_reduce_ca") + (() if to else ("id4_reduce_ca",))}
            print(f"B={B} x {n_atoms} atoms {'T' if to else 'Q'}: device {tg*1e3:.3f} ms  host {th*1e3:.1f} ms  identical={same}  {sizes}", flush=True)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def make_batch(sizes, first):
    """One batch on the device + its host sizes: molecule k of `sizes[k]` atoms, seeded by its number in the stream."""
    mols = [make_molecule(int(n), 2000 + first + k) for k, n in enumerate(sizes)]
    Nh = [int(n) for n in sizes]
    return dict(R=torch.tensor(np.concatenate([m["R"] for m in mols]), dtype=torch.float32, device="cuda"),
                Z=torch.tensor(np.concatenate([m["Z"] for m in mols]), device="cuda").long(), N=torch.tensor(Nh, device="cuda"),
                Nh=Nh)


def ragged_times(args, n_mol=32, n_batches=16, sized_on=8, cutoff=5.0):
    from gemnet_pytorch_amd.model.gemnet import GemNet
    from gemnet_pytorch_amd.padded import PaddedGraphRunner
    torch.cuda.reset_peak_memory_stats()
    rs = np.random.RandomState(9)
    batches = [make_batch(rs.choice([16, 24, 32], n_mol), 100 * b) for b in range(n_batches)]
    full = [make_batch([32] * n_mol, 100 * (n_batches + b)) for b in range(4)]       # the floor: the fixed layout 32 x 32
    lists = lambda b: DeviceGraphBuilder(b["Nh"], cutoff, cutoff, True, device="cuda")(b["R"], dtype=torch.int32)  # noqa: E731
    for b in batches + full:
        b["idx"] = lists(b)
    sizes = [PaddedGraphRunner.sizes_of(b["idx"]) for b in batches]
    e_cap, t_cap = PaddedGraphRunner.suggest_capacities(sizes[:sized_on] + [PaddedGraphRunner.sizes_of(b["idx"]) for b in full])
    a_cap, n_max = n_mol * 32, 32
    deg = n_max - 1
    # dummy groups for the largest padding: a small batch leaves most of e_cap to the pad edges, deg of them per dummy atom
    pad_max = e_cap - int(min(s[0] for s in sizes[:sized_on]) * 0.75)
    groups = max(1, -(-(pad_max // 2) // deg))
    torch.manual_seed(1234)
    model = GemNet(**GEMNET_T, scale_file=os.path.join(ROOT, "gemnet_pytorch_amd", "scaling_factors.json")).to("cuda").eval()
    model.requires_grad_(False)

    def runner(b0, **kw):
        return PaddedGraphRunner(model, b0["Z"], b0["N"], e_cap, t_cap, max_in_degree=deg, n_groups=groups, **kw)

    padded, graph, fixed = runner(batches[0], a_cap=a_cap), runner(batches[0], a_cap=a_cap), runner(full[0])
    ok = [sum(b["Nh"]) <= a_cap and padded.fits(s) for b, s in zip(batches, sizes)]
    keep, used = [b for b, k in zip(batches, ok) if k], [s for s, k in zip(sizes, ok) if k]
    out = {"molecules_per_batch": n_mol, "batches": len(keep), "batches_left_out": n_batches - len(keep),
           "atoms": sorted({sum(b["Nh"]) for b in keep}), "a_cap": a_cap, "n_max": n_max, "e_cap": e_cap, "t_cap": t_cap,
           "max_in_degree": deg, "dummy_groups": padded.G,
           "filler_atom_share": round(1.0 - float(np.mean([sum(b["Nh"]) for b in keep])) / a_cap, 4),
           "pad_edge_share": round(1.0 - float(np.mean([s[0] for s in used])) / e_cap, 4),
           "pad_triplet_share": round(1.0 - float(np.mean([s[1] for s in used])) / t_cap, 4)}
    print(json.dumps(out), flush=True)
    b0 = keep[0]
    graph._fill(b0["R"], {k: b0["idx"][k] for k in IDX_KEYS}, b0["Z"], b0["N"])
    graph.attach_builder(DeviceCapacityGraphBuilder(n_mol, a_cap, n_max, cutoff, device="cuda"))
    f0 = full[0]
    fixed._fill(f0["R"], {k: f0["idx"][k] for k in IDX_KEYS}, f0["Z"], f0["N"])
    fixed.attach_builder(DeviceGraphBuilder(f0["Nh"], cutoff, cutoff, True, device="cuda"))
    pos = {k: 0 for k in ("ragged_eager", "ragged_padded", "ragged_graph", "fixed_graph")}

    def nxt(k, stream=keep):
        pos[k] = (pos[k] + 1) % len(stream)
        return stream[pos[k]]

    def f_eager():
        b = nxt("ragged_eager")
        return model(dict(R=b["R"], Z=b["Z"], N=b["N"], **lists(b)))

    def f_padded():
        b = nxt("ragged_padded")
        idx = lists(b)
        return padded(b["R"], {k: idx[k] for k in IDX_KEYS}, Z=b["Z"], N=b["N"])

    def f_graph():
        b = nxt("ragged_graph")
        return graph.run_positions(b["R"], Z=b["Z"], N=b["N"])

    def f_fixed():
        b = nxt("fixed_graph", full)
        return fixed.run_positions(b["R"], Z=b["Z"])

    fns = {"ragged_eager": f_eager, "ragged_padded": f_padded, "ragged_graph": f_graph, "fixed_graph": f_fixed}
    if args.only:
        fns = {args.only: fns[args.only]}
    times = {k: [] for k in fns}
    for _ in range(1 if args.only else 3):
        for k, fn in fns.items():
            times[k].append(timed(fn, args.steps, args.warmup))
    for k, v in times.items():
        out[f"{k}_ms"], out[f"{k}_rounds"] = round(float(np.median(v)), 4), [round(x, 4) for x in v]
    torch.cuda.synchronize()
    out["index_error"] = {"ragged_graph": int(graph.index_error()), "fixed_graph": int(fixed.index_error())}
    out["index_sizes_last"] = list(graph.index_sizes())
    out["range_trips"] = {"ragged_padded": padded.flag.trips, "ragged_graph": graph.flag.trips, "fixed_graph": fixed.flag.trips}
    out["peak_memory_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)
    return out


def ragged_quad_times(args, n_mol=32, n_batches=16, sized_on=8, cutoff=5.0):
    from gemnet_pytorch_amd.kernels import PADDED_Q_KEYS
    from gemnet_pytorch_amd.model.gemnet import GemNet
    from gemnet_pytorch_amd.padded import PaddedGraphRunner
    torch.cuda.reset_peak_memory_stats()
    rs = np.random.RandomState(9)
    batches = [make_batch(rs.choice([16, 24, 32], n_mol), 100 * b) for b in range(n_batches)]
    for int_cutoff in INT_CUTOFFS:
        lists = lambda b: DeviceGraphBuilder(b["Nh"], cutoff, int_cutoff, False, device="cuda")(b["R"], dtype=torch.int32)  # noqa: E731
        sizes = [PaddedGraphRunner.sizes_of(lists(b)) for b in batches]
        e_cap, t_cap, quad_caps = PaddedGraphRunner.suggest_capacities(sizes[:sized_on])
        if quad_caps[2] < Q_CAP_LIMIT:
            break
    else:
        raise SystemExit(f"no interaction cutoff of {INT_CUTOFFS} keeps q_cap below {Q_CAP_LIMIT:g}")
    caps = (e_cap, t_cap) + tuple(quad_caps)
    a_cap, n_max = n_mol * 32, 32
    deg = n_max - 1
    # dummy groups for the largest padding: a unit of six pad edges puts two on atoms a and b of its group, deg at the most
    pad_max = e_cap - int(min(s[0] for s in sizes[:sized_on]) * 0.75)
    groups = max(1, -(-(-(-pad_max // 6)) // (deg // 2)))
    torch.manual_seed(1234)
    cfg = dict(GEMNET_T, triplets_only=False, int_cutoff=int_cutoff)
    model = GemNet(**cfg, scale_file=os.path.join(ROOT, "gemnet_pytorch_amd", "scaling_factors.json")).to("cuda").eval()
    model.requires_grad_(False)

    def runner(b0):
        return PaddedGraphRunner(model, b0["Z"], b0["N"], e_cap, t_cap, max_in_degree=deg, n_groups=groups, a_cap=a_cap,
                                 quad_caps=quad_caps)

    padded, graph = runner(batches[0]), runner(batches[0])
    ok = [sum(b["Nh"]) <= a_cap and padded.fits(s) for b, s in zip(batches, sizes)]
    keep, used = [b for b, k in zip(batches, ok) if k], [s for s, k in zip(sizes, ok) if k]
    share = lambda k: round(1.0 - float(np.mean([s[k] for s in used])) / caps[k], 4)  # noqa: E731
    out = {"model": "GemNet-Q, 4 blocks", "cutoff": cutoff, "int_cutoff": int_cutoff, "molecules_per_batch": n_mol,
           "batches": len(keep), "batches_left_out": n_batches - len(keep), "atoms": sorted({sum(b["Nh"]) for b in keep}),
           "a_cap": a_cap, "n_max": n_max, "e_cap": e_cap, "t_cap": t_cap, "eint_cap": quad_caps[0], "i_cap": quad_caps[1],
           "q_cap": quad_caps[2], "max_in_degree": deg, "dummy_groups": padded.G,
           "filler_atom_share": round(1.0 - float(np.mean([sum(b["Nh"]) for b in keep])) / a_cap, 4),
           "pad_edge_share": share(0), "pad_triplet_share": share(1), "pad_int_edge_share": share(2),
           "pad_intm_triplet_share": share(3), "pad_quadruplet_share": share(4)}
    print(json.dumps(out), flush=True)
    b0 = keep[0]
    idx0 = lists(b0)
    graph._fill(b0["R"], {k: idx0[k] for k in PADDED_Q_KEYS}, b0["Z"], b0["N"])
    graph.attach_builder(DeviceCapacityQuadGraphBuilder(n_mol, a_cap, n_max, cutoff, int_cutoff, device="cuda"))
    pos = {k: 0 for k in ("ragged_eager", "ragged_padded", "ragged_graph")}

    def nxt(k):
        pos[k] = (pos[k] + 1) % len(keep)
        return keep[pos[k]]

    def f_eager():
        b = nxt("ragged_eager")
        return model(dict(R=b["R"], Z=b["Z"], N=b["N"], **lists(b)))

    def f_padded():
        b = nxt("ragged_padded")
        idx = lists(b)
        return padded(b["R"], {k: idx[k] for k in PADDED_Q_KEYS}, Z=b["Z"], N=b["N"])

    def f_graph():
        b = nxt("ragged_graph")
        return graph.run_positions(b["R"], Z=b["Z"], N=b["N"])

    fns = {"ragged_eager": f_eager, "ragged_padded": f_padded, "ragged_graph": f_graph}
    if args.only:
        fns = {args.only: fns[args.only]}
    times = {k: [] for k in fns}
    for _ in range(1 if args.only else 3):
        for k, fn in fns.items():
            times[k].append(timed(fn, args.steps, args.warmup))
    for k, v in times.items():
        out[f"{k}_ms"], out[f"{k}_rounds"] = round(float(np.median(v)), 4), [round(x, 4) for x in v]
    torch.cuda.synchronize()
    out["index_error"] = {"ragged_graph": int(graph.index_error())}
    out["index_sizes_last"] = list(graph.index_sizes())
    # (a trip seen after the last replay has not gone through recover() yet: count it as well)
    out["range_trips"] = {k: r.flag.trips + int(r.flag.tripped()) for k, r in (("ragged_padded", padded), ("ragged_graph", graph))}
    out["matmul_precision_after"] = getattr(model, "matmul_precision", None) or "default"      # 'split6': a trip moved the model
    out["peak_memory_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ragged", action="store_true", help="force evaluation on batches of 32 molecules of changing sizes: builder + "
                    "eager, builder + padded replay, layout and lists inside the replay, and the fixed-layout floor")
    ap.add_argument("--quad", action="store_true", help="--ragged for a 4-block GemNet-Q: builder + eager, builder + padded replay, "
                    "layout and all sixteen lists inside the replay")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["ragged_eager", "ragged_padded", "ragged_graph", "fixed_graph"],
                    help="--ragged: one route alone, one round (for a kernel trace)")
    args = ap.parse_args()
    if args.quad and (not args.ragged or args.only == "fixed_graph"):
        ap.error("--quad goes with --ragged and has no fixed_graph route")
    if args.ragged:
        print(json.dumps(ragged_quad_times(args) if args.quad else ragged_times(args)))
    else:
        build_times()


if __name__ == "__main__":
    main()
