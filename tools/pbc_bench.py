#!/usr/bin/env python
"""Periodic forward + force + stress of GemNet-T on a water-like box, eager and replayed from a captured graph (runtime.
ForceGraphs), against the molecular forward + force on the same positions (no cell; fewer edges: no image pairs).
An MD loop on the same box — a short random walk of the positions, so that the neighbour list really changes — is timed two ways:
`md_eager_ms`: what `md.predict_periodic` did per step before the in-graph list (a new PeriodicGraphBuilder, the list with its two
size read-backs, ONE eager forward); `md_graph_exact_ms`: `runtime.DynamicForceField(cell=)`, list + model as one replayed graph,
in the default mode (`exact=True`: the host waits for every step and reads the report of its index build — what `predict()`
runs); `md_graph_ms`: the same with `exact=False` (nothing waits; comparable with `graph_periodic_ms`); `recaptures`: graphs
captured after the first.
`--train` times the TRAINING step instead (training/periodic.PeriodicTrainStep: energy + force + stress loss, rho_stress > 0, fused
optimizer) on the same box, eager (`train_eager_ms`) and replayed from its captured graph (`train_graph_ms`), next to the
molecular `TrainStep` on the same atoms without a cell (`train_molecular_*_ms`: fewer edges, no stress).
`--direct` times a DIRECT-FORCE model of the same architecture (`direct_forces=True`, GemNet.periodic_direct_forces: no backward
pass, forces from the edge head of csrc/direct_force.hip, no stress) on the same structures — `direct_*_ms`: eager call, fixed-list
replay, MD step with `exact=False` and `exact=True` — beside the autograd-force model (`autograd_*_ms`) timed in the same process:
the two alternate in rounds and the median round is reported (`*_rounds`: every round).  `--direct --eager-only` runs nothing but
eager periodic direct-force calls (for a kernel trace: launches per call = calls of a kernel / (warmup + steps)).
`--train --direct` times the TRAINING step of the direct-force model (PeriodicTrainStep on a `direct_forces=True` model: energy +
force loss, ONE first-order backward, fused optimizer) beside the autograd-force PeriodicTrainStep of `--train` in the same
process, in alternating rounds — `direct_train_eager_ms` / `autograd_train_eager_ms`, `*_train_graph_ms` (captured step), `*_rounds`;
with `--eager-only` nothing but eager direct-force training steps (for a kernel trace).
`--quad --int-cutoff X` times GemNet-Q (the same architecture with `triplets_only=False`, GemNet.periodic_quadruplets; index arrays of
pbc.PeriodicQuadGraphBuilder) on the box: `quad_eager_ms` (E, F, S), `quad_graph_ms` (fixed-list replay), `quad_build_ms` (the index
build with its read-backs), the edge / interaction-edge / intermediate-triplet / quadruplet counts and the peak device memory.
The quadruplet count grows like cutoff^6 int_cutoff^3: at the reference's int_cutoff = 10 a 192-atom box has ~1e8; the default
X = 5.0 keeps it below 3e7.
`--train --quad` times the TRAINING step of GemNet-Q on the box (PeriodicTrainStep on a `triplets_only=False` model: the second-order
force graph on the edge and interaction-edge vectors, energy + force + stress loss, fused optimizer), eager and captured
(`quad_train_eager_ms` / `quad_train_graph_ms`), beside the molecular `TrainStep` of the same model on the same atoms without a
cell (`quad_train_molecular_*_ms`), alternating in one process (`*_rounds`), + the counts of both graphs and the peak memory;
with `--eager-only` nothing but eager periodic steps (for a kernel trace).
`--train --stream [--direct]` times training on a NEW frame every step (positions walk, the cell is strained, the image list
changes): `stream_eager_ms` (PeriodicGraphBuilder + eager PeriodicTrainStep), `stream_padded_ms` (builder +
PeriodicPaddedTrainStep.step: one graph, lists handed in), `stream_graph_ms` (step_positions: the list built inside the replay)
and `fixed_captured_ms` (the fixed-list captured step on frame 0: the floor), alternating in one process (`*_rounds`), optimizer
included, + the capacities, the report of the in-graph build and the peak memory.
`--ragged [--direct]` times the force evaluation on batches of a periodic DATASET: four water boxes per batch, their sides drawn from
{2, 3, 4} per slot and per batch (24 / 81 / 192 atoms: sizes, species, cells and lists all change), three ways in alternating
rounds: `ragged_eager_ms` (pbc.PeriodicCapacityGraphBuilder + eager model: all the fixed layout offers for this workload),
`ragged_padded_ms` (builder + PaddedGraphRunner(a_cap=, cell=): one graph, lists handed in) and `ragged_graph_ms` (`run_positions`:
layout and list built inside the replay), + the capacities (from the first 8 batches), the share of pad rows and filler atoms,
the report of the in-graph build and the peak memory.
`--fit [--quad]` times one FIT-MODE forward (scale-factor fitting on the box, GemNet.periodic_scale_fitting) with the bilinear
sum's factor of block 1 active: `fit_kernel_ms` (the statistic of csrc/fit_stat.hip, rows read through the expand index) against
`fit_aten_ms` (GEMNET_FIT_STAT=0: a materialised gather + torch.var), alternating, + the peak memory of one pass of each.
Prints one JSON line.  The share of the periodic kernels comes from a separate kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/pbc_bench.py --steps 20
(kernel names pbc_* / *_vec_* are the periodic path; edge_basis_* / trip_basis_* without _vec are its molecular twins)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def water_box(n_side, seed=0):
    """n_side^3 H2O molecules on a jittered grid, 3.1 A apart (about liquid density)."""
    rs = np.random.RandomState(seed)
    a = 3.1
    O = np.array([[i, j, k] for i in range(n_side) for j in range(n_side) for k in range(n_side)], np.float64) * a
    O += rs.uniform(-0.2, 0.2, O.shape)
    R, Z = [], []
    for o in O:
        d1 = rs.normal(size=3); d1 /= np.linalg.norm(d1)
        d2 = rs.normal(size=3); d2 -= d2.dot(d1) * d1; d2 /= np.linalg.norm(d2)
        h1 = o + 0.96 * d1
        h2 = o + 0.96 * (np.cos(1.82) * d1 + np.sin(1.82) * d2)
        R += [o, h1, h2]
        Z += [8, 1, 1]
    return np.array(R), np.array(Z), np.eye(3) * a * n_side


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


def make_model(cutoff=5.0, direct=False, coupled=False, quad=False, int_cutoff=10.0, scale_file=None):
    """The 4-block, 128-wide GemNet-T of this tool (seeded weights, fitted scale factors), on the host; `direct`: the
    direct-force model of the same architecture with the periodic switch set.  `scale_file`: another scale json than the
    package's (--fit: one factor missing)."""
    from gemnet_pytorch_amd.model.gemnet import GemNet
    from oracle import gemnet_oracle as GO
    cfg = dict(num_spherical=7, num_radial=6, num_blocks=4, emb_size_atom=128, emb_size_edge=128, emb_size_trip=64,
               emb_size_quad=32, emb_size_rbf=16, emb_size_cbf=16, emb_size_sbf=32, emb_size_bil_quad=32, emb_size_bil_trip=64,
               num_before_skip=1, num_after_skip=1, num_concat=1, num_atom=2, triplets_only=True, cutoff=cutoff)
    if direct:
        cfg.update(direct_forces=True, forces_coupled=bool(coupled))
    if quad:
        cfg.update(triplets_only=False, int_cutoff=float(int_cutoff))
    scale_file = scale_file or os.path.join(ROOT, "gemnet_pytorch_amd", "scaling_factors.json")
    params = GO.make_params(cfg, 1, GO.load_scale_factors(scale_file), dtype=torch.float32)
    model = GemNet(**cfg, scale_file=scale_file)
    model.load_state_dict(GO.expand_to_reference_state_dict(params))
    model.periodic_direct_forces = bool(direct)
    model.periodic_quadruplets = bool(quad)
    return model


def quad_times(R, Rd, Zd, Nd, celld, A, args):
    """GemNet-Q on the periodic box: index build, eager call and fixed-list replay, the four counts and the peak memory; then the
    MD loop (positions walk, all arrays rebuilt every step): builder + eager call, and the one-replay step of
    runtime.DynamicForceField (exact=False / True) with the index build inside the graph."""
    from gemnet_pytorch_amd.pbc import PeriodicQuadGraphBuilder
    from gemnet_pytorch_amd.runtime import DynamicForceField, ForceGraphs
    torch.cuda.reset_peak_memory_stats()
    builder = PeriodicQuadGraphBuilder([A], args.cutoff, args.int_cutoff, device="cuda")
    idx = builder(Rd, celld, dtype=torch.int32)
    out = {"int_cutoff": args.int_cutoff, "edges": int(idx["id_a"].shape[0]), "interaction_edges": int(idx["id4_int_a"].shape[0]),
           "intermediate_triplets": int(idx["id4_expand_intm_db"].shape[0]), "quadruplets": int(idx["id4_reduce_ca"].shape[0])}
    print(json.dumps(out), flush=True)
    out["quad_build_ms"] = timed(lambda: builder(Rd, celld, dtype=torch.int32), max(args.steps // 5, 2), 1)
    model = make_model(args.cutoff, quad=True, int_cutoff=args.int_cutoff).to("cuda").eval()
    per = dict(R=Rd, Z=Zd, N=Nd, cell=celld, **idx)
    out["quad_eager_ms"] = timed(lambda: model(per, stress=True), args.steps, args.warmup)
    fg = ForceGraphs(model, [per])
    out["quad_graph_ms"] = timed(fg.replay, args.steps, args.warmup)
    out["quad_graph_ns_per_quadruplet"] = 1e6 * out["quad_graph_ms"] / max(out["quadruplets"], 1)
    out["peak_memory_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
    walk = random_walk(R, args.steps + args.warmup)
    state = {"i": 0}

    def nxt():
        state["i"] = (state["i"] + 1) % len(walk)
        return walk[state["i"]]

    def md_eager():
        Rs = nxt()
        return model(dict(R=Rs, Z=Zd, N=Nd, cell=celld, **builder(Rs, celld, dtype=torch.int32)), stress=True)

    out["md_eager_ms"] = timed(md_eager, args.steps, args.warmup)
    model.periodic_quadruplets_dynamic = True
    ff = DynamicForceField(model, Zd, [A], args.cutoff, args.int_cutoff, cell=celld)
    ff(walk[0])
    state["i"] = 0
    out["md_graph_ms"] = timed(lambda: ff(nxt(), exact=False), args.steps, args.warmup)
    torch.cuda.synchronize()
    out["md_graph_exact_ms"] = timed(lambda: ff(nxt()), args.steps, args.warmup)
    out["recaptures"] = int(ff.recaptures)
    out["md_index_failed"] = bool(ff.index_failed())
    out["md_sizes"] = list(ff.runner.index_sizes())
    return out


def random_walk(R, n, sigma=0.02, seed=5):
    """n + 1 position sets (float32, on the device): R and n steps of a Gaussian walk — the neighbour list changes on the way."""
    rs = np.random.RandomState(seed)
    out, R = [], np.asarray(R, np.float64)
    for _ in range(n + 1):
        out.append(torch.tensor(R, dtype=torch.float32, device="cuda"))
        R = R + rs.normal(0, sigma, R.shape)
    return out


def train_times(per, mol, args):
    """Eager and captured step time of PeriodicTrainStep on `per` and of the molecular TrainStep on `mol` (optimizer included)."""
    from gemnet_pytorch_amd.training.ddp import TrainStep
    from gemnet_pytorch_amd.training.periodic import PeriodicTrainStep
    g = torch.Generator().manual_seed(2)
    A = per["R"].shape[0]
    targets = {"E": torch.randn(1, 1, generator=g).cuda(), "F": torch.randn(A, 3, generator=g).cuda(),
               "S": 0.01 * torch.randn(1, 3, 3, generator=g).cuda()}
    out = {}
    for key, inputs, make in (("train", per, lambda m: PeriodicTrainStep(m, rho_stress=0.01, fused_optimizer=True)),
                              ("train_molecular", mol, lambda m: TrainStep(m, fused_optimizer=True))):
        ts = make(make_model(args.cutoff).to("cuda"))
        out[f"{key}_eager_ms"] = timed(lambda: ts(inputs, targets), args.steps, args.warmup)
        ts.capture(inputs, targets)
        out[f"{key}_graph_ms"] = timed(lambda: ts(inputs, targets), args.steps, args.warmup)
        out[f"{key}_loss"] = float(ts.last_loss)
    return out


def quad_train_times(Rd, Zd, Nd, celld, A, args):
    """Eager and captured training step of GemNet-Q on the periodic box beside the molecular TrainStep of the same model on the
    same atoms without a cell, alternating in one process; optimizer included."""
    from gemnet_pytorch_amd.index_device import build_indices_device
    from gemnet_pytorch_amd.pbc import PeriodicQuadGraphBuilder
    from gemnet_pytorch_amd.training.ddp import TrainStep
    from gemnet_pytorch_amd.training.periodic import PeriodicTrainStep
    torch.cuda.reset_peak_memory_stats()
    idx = PeriodicQuadGraphBuilder([A], args.cutoff, args.int_cutoff, device="cuda")(Rd, celld, dtype=torch.int32)
    mix = build_indices_device(Rd, np.array([A]), args.cutoff, args.int_cutoff, False, dtype=torch.int32)
    out = {"int_cutoff": args.int_cutoff}
    for tag, d in (("periodic", idx), ("molecular", mix)):
        out.update({f"edges_{tag}": int(d["id_a"].shape[0]), f"interaction_edges_{tag}": int(d["id4_int_a"].shape[0]),
                    f"quadruplets_{tag}": int(d["id4_reduce_ca"].shape[0])})
    print(json.dumps(out), flush=True)
    g = torch.Generator().manual_seed(2)
    targets = {"E": torch.randn(1, 1, generator=g).cuda(), "F": torch.randn(A, 3, generator=g).cuda(),
               "S": 0.01 * torch.randn(1, 3, 3, generator=g).cuda()}
    new = lambda: make_model(args.cutoff, quad=True, int_cutoff=args.int_cutoff).to("cuda")      # noqa: E731
    steps = {"quad_train": PeriodicTrainStep(new(), rho_stress=0.01, fused_optimizer=True)}
    inputs = {"quad_train": dict(R=Rd, Z=Zd, N=Nd, cell=celld, **idx)}
    if args.eager_only:
        for _ in range(args.warmup + args.steps):
            steps["quad_train"](inputs["quad_train"], targets)
        torch.cuda.synchronize()
        out["eager_steps"] = args.warmup + args.steps
        return out
    steps["quad_train_molecular"] = TrainStep(new(), fused_optimizer=True)
    inputs["quad_train_molecular"] = dict(R=Rd, Z=Zd, N=Nd, **mix)

    def record(tag, res):
        for k, (med, rounds) in res.items():
            out[f"{k}_{tag}_ms"], out[f"{k}_{tag}_rounds"] = med, rounds

    fns = {k: (lambda ts=ts, k=k: ts(inputs[k], targets)) for k, ts in steps.items()}
    record("eager", alternated(fns, args.steps, args.warmup))
    out["peak_memory_eager_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
    for k, ts in steps.items():
        ts.capture(inputs[k], targets)
    record("graph", alternated(fns, args.steps, args.warmup))
    for k, ts in steps.items():
        out[f"{k}_loss"] = float(ts.last_loss)
        out[f"{k}_precision"] = str(ts.model.matmul_precision)
    out["peak_memory_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
    return out


def train_direct_times(per, args):
    """Eager and captured training step of the direct-force model beside the autograd-force model's (energy + force + stress
    loss, as `--train`), alternating in one process; optimizer included."""
    from gemnet_pytorch_amd.training.periodic import PeriodicTrainStep
    g = torch.Generator().manual_seed(2)
    A = per["R"].shape[0]
    targets = {"E": torch.randn(1, 1, generator=g).cuda(), "F": torch.randn(A, 3, generator=g).cuda(),
               "S": 0.01 * torch.randn(1, 3, 3, generator=g).cuda()}
    steps = {"direct": PeriodicTrainStep(make_model(args.cutoff, direct=True, coupled=args.coupled).to("cuda"), fused_optimizer=True),
             "autograd": PeriodicTrainStep(make_model(args.cutoff).to("cuda"), rho_stress=0.01, fused_optimizer=True)}
    inputs = {k: dict(per) for k in steps}
    out = {"forces_coupled": bool(args.coupled), "autograd_rho_stress": 0.01}
    if args.eager_only:
        for _ in range(args.warmup + args.steps):
            steps["direct"](inputs["direct"], targets)
        torch.cuda.synchronize()
        out["eager_steps"] = args.warmup + args.steps
        return out

    def record(tag, res):
        for k, (med, rounds) in res.items():
            out[f"{k}_train_{tag}_ms"], out[f"{k}_train_{tag}_rounds"] = med, rounds

    fns = {k: (lambda ts=ts, k=k: ts(inputs[k], targets)) for k, ts in steps.items()}
    record("eager", alternated(fns, args.steps, args.warmup))
    for k, ts in steps.items():
        ts.capture(inputs[k], targets)
    record("graph", alternated(fns, args.steps, args.warmup))
    for k, ts in steps.items():
        out[f"{k}_train_loss"] = float(ts.last_loss)
    return out


def stream_frames(R, cell, n, sigma=0.02, strain=2e-4, seed=5):
    """n frames of a trajectory (numpy, float32-rounded): the positions take a Gaussian walk, the cell gets a small random strain
    every step — positions, cell and the image neighbour list all change from frame to frame."""
    rs = np.random.RandomState(seed)
    R, cell = np.asarray(R, np.float64), np.asarray(cell, np.float64)
    out = []
    for _ in range(n):
        out.append((R.astype(np.float32), cell.astype(np.float32)))
        R = R + rs.normal(0, sigma, R.shape)
        cell = cell @ (np.eye(3) + rs.normal(0, strain, (3, 3)))
    return out


def stream_train_times(R, Zd, Nd, cell, A, args, sized_on=8):
    """`--train --stream`: a NEW frame (positions, cell, list) every training step, optimizer included, four ways in alternating
    rounds: PeriodicGraphBuilder + eager PeriodicTrainStep (`stream_eager_ms`: all the parent offered for this workload), builder +
    PeriodicPaddedTrainStep.step (`stream_padded_ms`: one graph, lists handed in), step_positions (`stream_graph_ms`: the list
    built inside the replay) and, as the floor, the fixed-list captured PeriodicTrainStep on frame 0 (`fixed_captured_ms`).  The
    capacities come from the first `sized_on` frames (PaddedGraphRunner.suggest_capacities / in_degree_of)."""
    from gemnet_pytorch_amd.padded import PaddedGraphRunner
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder
    from gemnet_pytorch_amd.training.periodic import PeriodicPaddedTrainStep, PeriodicTrainStep
    torch.cuda.reset_peak_memory_stats()
    frames = [(torch.tensor(r, device="cuda"), torch.tensor(c[None], device="cuda"))
              for r, c in stream_frames(R, cell, args.steps + args.warmup + 1)]
    builder = PeriodicGraphBuilder([A], args.cutoff, device="cuda")
    lists = [builder(r, c, dtype=torch.int32) for r, c in frames[:sized_on]]
    sizes = [PaddedGraphRunner.sizes_of(ix) for ix in lists]
    e_cap, t_cap = PaddedGraphRunner.suggest_capacities(sizes)
    deg = int(max(PaddedGraphRunner.in_degree_of(ix) for ix in lists) * 1.08) + 1
    # dummy groups for the padding left when the list shrinks to 3/4 of the smallest seen: two incoming edges per pad quad
    pad_max = e_cap - int(min(s[0] for s in sizes) * 0.75)
    groups = max(1, -(-(-(-pad_max // 4)) // max(deg // 2, 1)))
    rho_s = 0.0 if args.direct else 0.01
    g = torch.Generator().manual_seed(2)
    Et, Ft = torch.randn(1, 1, generator=g).cuda(), torch.randn(A, 3, generator=g).cuda()
    St = None if args.direct else 0.01 * torch.randn(1, 3, 3, generator=g).cuda()
    targets = {"E": Et, "F": Ft} if args.direct else {"E": Et, "F": Ft, "S": St}
    new = lambda: make_model(args.cutoff, direct=args.direct, coupled=args.coupled).to("cuda")      # noqa: E731
    out = {"direct": bool(args.direct), "rho_stress": rho_s, "frames": len(frames), "sizes_first_frames": [list(s) for s in sizes],
           "e_cap": e_cap, "t_cap": t_cap, "max_in_degree": deg, "dummy_groups": groups}
    print(json.dumps(out), flush=True)
    eager = PeriodicTrainStep(new(), rho_stress=rho_s, fused_optimizer=True)
    fixed = PeriodicTrainStep(new(), rho_stress=rho_s, fused_optimizer=True)
    kw = dict(cell=frames[0][1], max_in_degree=deg, n_groups=groups, rho_stress=rho_s, fused_optimizer=True)
    padded = PeriodicPaddedTrainStep(new(), Zd, Nd, e_cap, t_cap, **kw)
    graph = PeriodicPaddedTrainStep(new(), Zd, Nd, e_cap, t_cap, **kw)
    graph.pad._fill(frames[0][0], lists[0], cell=frames[0][1])
    graph.attach_builder(builder)
    fixed_inputs = dict(R=frames[0][0], Z=Zd, N=Nd, cell=frames[0][1], **lists[0])
    fixed.capture(fixed_inputs, targets)
    pos = {k: 0 for k in ("stream_eager", "stream_padded", "stream_graph")}

    def nxt(k):
        pos[k] = (pos[k] + 1) % len(frames)
        return frames[pos[k]]

    def f_eager():
        r, c = nxt("stream_eager")
        return eager(dict(R=r, Z=Zd, N=Nd, cell=c, **builder(r, c, dtype=torch.int32)), targets)

    def f_padded():
        r, c = nxt("stream_padded")
        return padded.step(r, builder(r, c, dtype=torch.int32), c, Et, Ft, St)

    def f_graph():
        r, c = nxt("stream_graph")
        return graph.step_positions(r, c, Et, Ft, St)

    fns = {"stream_eager": f_eager, "stream_padded": f_padded, "stream_graph": f_graph,
           "fixed_captured": lambda: fixed(fixed_inputs, targets)}
    for k, (med, rounds) in alternated(fns, args.steps, args.warmup).items():
        out[f"{k}_ms"], out[f"{k}_rounds"] = med, rounds
    torch.cuda.synchronize()
    out["index_error"] = int(graph.pad.index_error())
    out["index_sizes_last"] = list(graph.pad.index_sizes())
    out["losses"] = {"stream_eager": float(eager.last_loss), "stream_padded": float(padded.last_loss),
                     "stream_graph": float(graph.last_loss), "fixed_captured": float(fixed.last_loss)}
    out["range_trips"] = {"stream_eager": eager.flag.trips, "stream_padded": padded.flag.trips, "stream_graph": graph.flag.trips,
                          "fixed_captured": fixed.flag.trips}
    out["peak_memory_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
    return out


def ragged_times(args, n_mol=4, n_batches=16, sized_on=8):
    """`--ragged`: a NEW batch of `n_mol` water boxes of different sizes every call (E, F, S; `--direct`: E, F), three ways in
    alternating rounds: capacity builder + eager model, builder + padded replay, `run_positions`.  The capacities come from the
    first `sized_on` batches (PaddedGraphRunner.suggest_capacities / in_degree_of, the largest atom count); later batches that
    do not fit them are left out of the stream (`batches_left_out`)."""
    from gemnet_pytorch_amd.padded import PaddedGraphRunner
    from gemnet_pytorch_amd.pbc import PeriodicCapacityGraphBuilder, PeriodicGraphBuilder
    torch.cuda.reset_peak_memory_stats()
    rs = np.random.RandomState(9)
    batches = []
    for b in range(n_batches):
        parts = [water_box(int(side), seed=100 * b + k) for k, side in enumerate(rs.choice([2, 3, 4], n_mol))]
        Nh = [len(p[0]) for p in parts]
        R = torch.tensor(np.concatenate([p[0] for p in parts]), dtype=torch.float32, device="cuda")
        cell = torch.tensor(np.stack([p[2] for p in parts]), dtype=torch.float32, device="cuda")
        batches.append(dict(R=R, Z=torch.tensor(np.concatenate([p[1] for p in parts]), device="cuda").long(),
                            N=torch.tensor(Nh, device="cuda"), Nh=Nh, cell=cell,
                            idx=PeriodicGraphBuilder(Nh, args.cutoff, device="cuda")(R, cell, dtype=torch.int32)))
    sizes = [PaddedGraphRunner.sizes_of(b["idx"]) for b in batches]
    degs = [PaddedGraphRunner.in_degree_of(b["idx"]) for b in batches]
    e_cap, t_cap = PaddedGraphRunner.suggest_capacities(sizes[:sized_on])
    deg = int(max(degs[:sized_on]) * 1.08) + 1
    a_cap = max(sum(b["Nh"]) for b in batches[:sized_on])
    pad_max = e_cap - int(min(s[0] for s in sizes[:sized_on]) * 0.75)
    groups = max(1, -(-(-(-pad_max // 4)) // max(deg // 2, 1)))
    model = make_model(args.cutoff, direct=args.direct, coupled=args.coupled).to("cuda").eval()
    model.periodic_atom_capacity = True
    kw = {} if args.direct else dict(stress=True)

    def runner():
        b0 = batches[0]
        return PaddedGraphRunner(model, b0["Z"], b0["N"], e_cap, t_cap, max_in_degree=deg, n_groups=groups, a_cap=a_cap,
                                 cell=b0["cell"])

    padded, graph = runner(), runner()
    keep = [b for b, s, d in zip(batches, sizes, degs) if sum(b["Nh"]) <= a_cap and padded.fits(s) and d <= deg]
    used = [s for b, s, d in zip(batches, sizes, degs) if sum(b["Nh"]) <= a_cap and padded.fits(s) and d <= deg]
    out = {"direct": bool(args.direct), "structures_per_batch": n_mol, "batches": len(keep), "batches_left_out": n_batches - len(keep),
           "atoms": sorted({sum(b["Nh"]) for b in keep}), "a_cap": a_cap, "e_cap": e_cap, "t_cap": t_cap, "max_in_degree": deg,
           "dummy_groups": groups, "filler_atom_share": 1.0 - float(np.mean([sum(b["Nh"]) for b in keep])) / a_cap,
           "pad_edge_share": 1.0 - float(np.mean([s[0] for s in used])) / e_cap,
           "pad_triplet_share": 1.0 - float(np.mean([s[1] for s in used])) / t_cap}
    print(json.dumps(out), flush=True)
    cb = PeriodicCapacityGraphBuilder(n_mol, a_cap, args.cutoff, device="cuda")
    cb_graph = PeriodicCapacityGraphBuilder(n_mol, a_cap, args.cutoff, device="cuda")
    b0 = keep[0]
    graph._fill(b0["R"], b0["idx"], b0["Z"], b0["N"], b0["cell"])
    graph.attach_builder(cb_graph)
    pos = {k: 0 for k in ("ragged_eager", "ragged_padded", "ragged_graph")}

    def nxt(k):
        pos[k] = (pos[k] + 1) % len(keep)
        return keep[pos[k]]

    def lists(b):
        cb.set_layout(b["Nh"])
        return cb(b["R"], b["cell"], dtype=torch.int32)

    def f_eager():
        b = nxt("ragged_eager")
        return model(dict(R=b["R"], Z=b["Z"], N=b["N"], cell=b["cell"], **lists(b)), **kw)

    def f_padded():
        b = nxt("ragged_padded")
        return padded(b["R"], lists(b), Z=b["Z"], N=b["N"], cell=b["cell"])

    def f_graph():
        b = nxt("ragged_graph")
        return graph.run_positions(b["R"], Z=b["Z"], N=b["N"], cell=b["cell"])

    fns = {"ragged_eager": f_eager, "ragged_padded": f_padded, "ragged_graph": f_graph}
    for k, (med, rounds) in alternated(fns, args.steps, args.warmup).items():
        out[f"{k}_ms"], out[f"{k}_rounds"] = med, rounds
    torch.cuda.synchronize()
    out["index_error"] = int(graph.index_error())
    out["index_sizes_last"] = list(graph.index_sizes())
    out["range_trips"] = {"ragged_padded": padded.flag.trips, "ragged_graph": graph.flag.trips}
    out["peak_memory_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
    return out


def alternated(fns, steps, warmup, rounds=3):
    """{name: fn} timed in turns, `rounds` times each -> {name: (median ms, [ms of every round])}."""
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, steps, warmup))
    return {k: (float(np.median(v)), [round(x, 4) for x in v]) for k, v in times.items()}


def direct_times(per, R, A, Zd, Nd, celld, args):
    """The direct-force model beside the autograd-force model: eager, fixed-list replay, MD step (exact=False / True)."""
    from gemnet_pytorch_amd.runtime import DynamicForceField, ForceGraphs
    models = {"direct": make_model(args.cutoff, direct=True, coupled=args.coupled).to("cuda").eval(),
              "autograd": make_model(args.cutoff).to("cuda").eval()}
    stress = {"direct": False, "autograd": True}
    out = {"forces_coupled": bool(args.coupled)}
    if args.eager_only:
        for _ in range(args.warmup + args.steps):
            models["direct"](per)
        torch.cuda.synchronize()
        out["eager_calls"] = args.warmup + args.steps
        return out

    def record(tag, res):
        for k, (med, rounds) in res.items():
            out[f"{k}_{tag}_ms"], out[f"{k}_{tag}_rounds"] = med, rounds

    record("eager", alternated({k: (lambda m=m, k=k: m(per, stress=stress[k])) for k, m in models.items()},
                               args.steps, args.warmup))
    graphs = {k: ForceGraphs(m, [per]) for k, m in models.items()}
    record("graph", alternated({k: g.replay for k, g in graphs.items()}, args.steps, args.warmup))
    walk = random_walk(R, args.steps + args.warmup)
    state = {"i": 0}

    def nxt():
        state["i"] = (state["i"] + 1) % len(walk)
        return walk[state["i"]]

    fields = {k: DynamicForceField(m, Zd, [A], args.cutoff, 10.0, cell=celld) for k, m in models.items()}
    for ff in fields.values():
        ff(walk[0])
    record("md_graph", alternated({k: (lambda ff=ff: ff(nxt(), exact=False)) for k, ff in fields.items()},
                                  args.steps, args.warmup))
    torch.cuda.synchronize()
    record("md_graph_exact", alternated({k: (lambda ff=ff: ff(nxt())) for k, ff in fields.items()}, args.steps, args.warmup))
    out["recaptures"] = {k: int(ff.recaptures) for k, ff in fields.items()}
    out["md_index_failed"] = {k: bool(ff.index_failed()) for k, ff in fields.items()}
    return out


def fit_times(per, args):
    """--fit [--quad]: one fit-mode forward (GemNet.periodic_scale_fitting) on the box with the bilinear sum's factor of block 1
    (`TripInteraction_1_sum_cbf`, --quad: `QuadInteraction_1_sum_sbf`) as the active one: the kernel statistic (GEMNET_FIT_STAT=1:
    rows read through the expand index, gn_col_var_f32) against the ATen statistic (=0: materialised gather + torch.var),
    alternating in one process, three rounds; + the peak device memory of one pass of each."""
    import tempfile

    from gemnet_pytorch_amd.model import scaling
    from gemnet_pytorch_amd.model.scaling import AutomaticFit
    from gemnet_pytorch_amd.model.utils import write_json
    from oracle import gemnet_oracle as GO
    target = "QuadInteraction_1_sum_sbf" if args.quad else "TripInteraction_1_sum_cbf"
    have = GO.load_scale_factors(os.path.join(ROOT, "gemnet_pytorch_amd", "scaling_factors.json"))
    have.pop(target)
    out = {"active_factor": target}
    old = scaling.USE_FIT_STAT
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scaling.json")
        write_json(path, dict(comment="pbc_bench --fit", **have))
        AutomaticFit.set2fitmode()
        try:
            model = make_model(args.cutoff, quad=args.quad, int_cutoff=args.int_cutoff, scale_file=path).to("cuda").eval()
            model.periodic_scale_fitting = True
            assert AutomaticFit.activeVar.name == target and not AutomaticFit.queue

            def run(flag):
                scaling.USE_FIT_STAT = flag
                return model(per, stress=True)

            for tag, flag in (("kernel", True), ("aten", False)):
                run(flag)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                run(flag)
                torch.cuda.synchronize()
                out[f"fit_{tag}_peak_memory_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
            res = alternated({"fit_kernel": lambda: run(True), "fit_aten": lambda: run(False)}, args.steps, args.warmup)
            for k, (med, rounds) in res.items():
                out[f"{k}_ms"], out[f"{k}_rounds"] = med, rounds
        finally:
            scaling.USE_FIT_STAT = old
            AutomaticFit.fitting_mode = False
            AutomaticFit.reset()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cutoff", type=float, default=5.0)
    ap.add_argument("--train", action="store_true", help="time the periodic training step instead of the force evaluation")
    ap.add_argument("--stream", action="store_true", help="--train: a new frame (positions, cell, list) every step — eager, padded, "
                    "in-graph list, and the fixed-list captured step as the floor; with --direct for the direct-force model")
    ap.add_argument("--ragged", action="store_true", help="force evaluation on batches of four water boxes of changing sizes: capacity "
                    "builder + eager, padded replay, layout + list inside the replay; with --direct for the direct-force model")
    ap.add_argument("--direct", action="store_true", help="time a direct-force model beside the autograd-force model")
    ap.add_argument("--coupled", action="store_true", help="--direct: forces_coupled=True")
    ap.add_argument("--quad", action="store_true", help="time GemNet-Q (periodic_quadruplets) on the box")
    ap.add_argument("--int-cutoff", type=float, default=5.0, help="--quad: the interaction cutoff (quadruplets ~ int_cutoff^3)")
    ap.add_argument("--eager-only", action="store_true", help="--direct / --train --quad: only eager direct-force calls / training steps (for a kernel trace)")
    ap.add_argument("--fit", action="store_true", help="time one fit-mode forward (scale-factor fitting) with the kernel statistic "
                    "against the ATen statistic; with --quad for GemNet-Q")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from gemnet_pytorch_amd.index_device import build_indices_device
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder
    from gemnet_pytorch_amd.runtime import DynamicForceField, ForceGraphs

    if args.ragged:
        if args.train or args.stream or args.quad:
            ap.error("--ragged times the force evaluation of GemNet-T / GemNet-dT: use it alone or with --direct")
        print(json.dumps(dict({"cutoff": args.cutoff}, **ragged_times(args))))
        return
    R, Z, cell = water_box(args.side)
    A = len(R)
    Rd = torch.tensor(R, dtype=torch.float32, device="cuda")
    Zd = torch.tensor(Z, device="cuda").long()
    Nd = torch.tensor([A], device="cuda")
    celld = torch.tensor(cell[None], dtype=torch.float32, device="cuda")
    if args.fit:
        from gemnet_pytorch_amd.pbc import PeriodicQuadGraphBuilder
        if args.quad:
            idx = PeriodicQuadGraphBuilder([A], args.cutoff, args.int_cutoff, device="cuda")(Rd, celld, dtype=torch.int32)
            sizes = {"int_cutoff": args.int_cutoff, "quadruplets": int(idx["id4_reduce_ca"].shape[0])}
        else:
            idx = PeriodicGraphBuilder([A], args.cutoff, device="cuda")(Rd, celld, dtype=torch.int32)
            sizes = {"triplets": int(idx["id3_reduce_ca"].shape[0])}
        res = fit_times(dict(R=Rd, Z=Zd, N=Nd, cell=celld, **idx), args)
        print(json.dumps(dict({"atoms": A, "cutoff": args.cutoff, "edges": int(idx["id_a"].shape[0])}, **sizes, **res)))
        return
    if args.quad:
        res = quad_train_times(Rd, Zd, Nd, celld, A, args) if args.train else quad_times(R, Rd, Zd, Nd, celld, A, args)
        print(json.dumps(dict({"atoms": A, "cutoff": args.cutoff}, **res)))
        return
    if args.stream:
        if not args.train:
            ap.error("--stream times the training step: use it with --train")
        res = stream_train_times(R, Zd, Nd, cell, A, args)
        print(json.dumps(dict({"atoms": A, "cutoff": args.cutoff}, **res)))
        return
    model = make_model(args.cutoff).to("cuda").eval()
    idx = PeriodicGraphBuilder([A], args.cutoff, device="cuda")(Rd, celld, dtype=torch.int32)
    per = dict(R=Rd, Z=Zd, N=Nd, cell=celld, **idx)
    mol = dict(R=Rd, Z=Zd, N=Nd, **build_indices_device(Rd, np.array([A]), args.cutoff, 10.0, True, dtype=torch.int32))

    out = {"atoms": A, "cutoff": args.cutoff, "edges_periodic": int(idx["id_a"].shape[0]),
           "triplets_periodic": int(idx["id3_reduce_ca"].shape[0]), "edges_molecular": int(mol["id_a"].shape[0]),
           "triplets_molecular": int(mol["id3_reduce_ca"].shape[0])}
    if args.train:
        out.update(train_direct_times(per, args) if args.direct else train_times(per, mol, args))
        print(json.dumps(out))
        return
    if args.direct:
        out.update(direct_times(per, R, A, Zd, Nd, celld, args))
        print(json.dumps(out))
        return
    out["eager_periodic_ms"] = timed(lambda: model(per, stress=True), args.steps, args.warmup)
    out["eager_molecular_ms"] = timed(lambda: model(mol), args.steps, args.warmup)
    fp = ForceGraphs(model, [per])
    out["graph_periodic_ms"] = timed(fp.replay, args.steps, args.warmup)
    fm = ForceGraphs(model, [mol])
    out["graph_molecular_ms"] = timed(fm.replay, args.steps, args.warmup)
    for k in ("periodic", "molecular"):
        out[f"graph_{k}_ns_per_triplet"] = 1e6 * out[f"graph_{k}_ms"] / max(out[f"triplets_{k}"], 1)
    # the MD loop: positions walk, the list is rebuilt every step
    walk = random_walk(R, args.steps + args.warmup)
    state = {"i": 0}

    def nxt():
        state["i"] = (state["i"] + 1) % len(walk)
        return walk[state["i"]]

    def md_eager():
        Rs = nxt()
        ix = PeriodicGraphBuilder([A], args.cutoff, device="cuda")(Rs, celld, dtype=torch.int32)
        return model(dict(R=Rs, Z=Zd, N=Nd, cell=celld, **ix), stress=True)

    out["md_eager_ms"] = timed(md_eager, args.steps, args.warmup)
    ff = DynamicForceField(model, Zd, [A], args.cutoff, 10.0, cell=celld)
    ff(walk[0])
    state["i"] = 0
    out["md_graph_ms"] = timed(lambda: ff(nxt(), exact=False), args.steps, args.warmup)
    torch.cuda.synchronize()
    out["md_graph_exact_ms"] = timed(lambda: ff(nxt()), args.steps, args.warmup)
    out["recaptures"] = int(ff.recaptures)
    out["md_index_failed"] = bool(ff.index_failed())
    out["md_sizes"] = list(ff.runner.index_sizes())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
