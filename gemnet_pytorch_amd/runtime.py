"""Static-shape inference runtime: hipGraphs of forward+force, replayed concurrently on dedicated HIP streams.

At the headline batch (32 molecules x 32 atoms: 18 k edges) every kernel of the path is latency-bound — a
128x128 layer over 18 k rows is ~4 us of MFMA work behind ~4 us of launch/drain — so a single in-order
stream leaves the chip partly idle between kernels.  Molecules are independent (block-diagonal index
arrays), so the batch is cut into sub-batches, each captured ONCE into its own hipGraph
(`torch.cuda.CUDAGraph`, including the autograd pass that yields F = -dE/dR) on its own stream; a step
launches all graphs back-to-back and the hardware interleaves their kernels.  No nested capture, no
collective, no host synchronisation inside a step.

The graphs read the model parameters and the `R` tensors of the sub-batches in place: `set_positions`
copies new coordinates into the captured buffers (MD with a fixed neighbour list); a changed graph
(new neighbour list) needs a new runner.
"""
import os
import warnings

import torch


class RangeFlag:
    """The range check of REPLAYED graphs (include/gemnet_hip.h, gn_nonfinite_flag_f32).

    The default Dense arithmetic ("h3") keeps activations in two fp16 planes: beyond 65 504 they become inf, which propagates
    to the energies and forces; the reference's fp32 (base_layers.py:44-48) has no such cliff.  An eager forward reads its
    outputs back (GemNet.forward); a captured hipGraph — the MD loop, padded batches, the training step: the paths built for
    long unattended runs — cannot.  A graph captured with a RangeFlag ends with one tiny launch per output that ORs a bit
    into ONE device word when the output holds an inf / NaN, and with a copy of that word into pinned host memory; the host
    reads the pinned copy without synchronising (`tripped()`: what the COMPLETED replays left there — exact right after
    anything that waited for the replay, e.g. the `.cpu()` of `GemNet.predict`).  The word is sticky until `reset()`.
    Bits: OUTPUT = non-finite energies / forces of a forward; GRAD = a non-finite gradient norm (the fused optimizer skipped
    that step, csrc/optim.hip); bits 8+ of the word count the steps the fused optimizer skipped since the last reset.
    With several ranks (`snapshot` / `poll_lagged`) the word is OR-reduced over the ranks at a fixed point of every step and
    read from the mirror slot of the step BEFORE the previous one, behind that step's event: every rank then sees the same
    word at the same call, whatever its host is ahead of its GPU by."""
    OUTPUT, GRAD = 1, 2

    def __init__(self, device):
        self.word = torch.zeros(1, dtype=torch.int32, device=device)
        self.host = torch.zeros(1, dtype=torch.int32).pin_memory() if torch.device(device).type == "cuda" \
            else torch.zeros(1, dtype=torch.int32)
        self.trips = 0
        self._slots = None          # multi-rank polling: two pinned mirror slots + their events, by step parity
        self._step = 0

    def watch(self, *tensors, bit=OUTPUT):
        """Enqueue (or capture) the check of `tensors` (contiguous fp32) and the mirror copy on the current stream."""
        from . import kernels as K
        for t in tensors:
            K.nonfinite_flag(t, self.word, bit)
        self.mirror()

    def mirror(self):
        self.host.copy_(self.word, non_blocking=True)

    def tripped(self):
        return int(self.host[0]) & 0xff

    def skipped(self):
        """Steps the fused optimizer skipped on the device since the last reset (as of the last completed mirror copy)."""
        return int(self.host[0]) >> 8

    def reset(self):
        self.word.zero_()
        self.host.zero_()
        if self._slots is not None:
            for h, _ in self._slots:
                h.zero_()

    # ---- several ranks: one decision for all of them -------------------------------------------------------------------
    def snapshot(self, group=None):
        """End of a step (every rank, same point): OR the word over the ranks on the device (the collective is enqueued like the
        gradient all-reduce: no host synchronisation) and mirror it into the pinned slot of this step's parity, behind an event."""
        import torch.distributed as dist
        if self._slots is None:
            cuda = self.word.is_cuda
            self._slots = [((torch.zeros(1, dtype=torch.int32).pin_memory() if cuda else torch.zeros(1, dtype=torch.int32)),
                            torch.cuda.Event() if cuda else None) for _ in range(2)]
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.word, op=dist.ReduceOp.BOR, group=group)
        host, ev = self._slots[self._step & 1]
        host.copy_(self.word, non_blocking=True)
        if ev is not None:
            ev.record()
        self.host.copy_(self.word, non_blocking=True)
        self._step += 1

    def poll_lagged(self):
        """Start of a step: the word as the step before the previous one left it (waits for THAT step's event — free when the
        host runs at most one step ahead of the device).  The same value on every rank at the same call."""
        if self._slots is None or self._step < 2:
            return 0
        host, ev = self._slots[self._step & 1]          # parity of step - 2
        if ev is not None:
            ev.synchronize()
        return int(host[0])


def fall_back_to_bf16_planes(model, what, positions=None):
    """A replayed graph of `model` produced non-finite values in the fp16-plane arithmetic: warn, move THIS model to the
    bf16-plane form ("split6": fp32 exponent range) and drop everything derived from its weights in the old format.  The
    caller captures anew.  False when the model was not on the fp16 planes (the values are non-finite for another reason:
    nothing to fall back to)."""
    from . import kernels as K
    mode = getattr(model, "matmul_precision", None) or K.DEFAULT_CHAIN_MODE
    if positions is not None:
        bad = [p for p in (positions if isinstance(positions, (list, tuple)) else [positions])
               if torch.is_tensor(p) and not bool(torch.isfinite(p).all())]
        if bad:
            # NaN / inf handed in by the caller is not an overflow of the arithmetic: the model stays where it is
            warnings.warn(f"gemnet_pytorch_amd: non-finite values in {what}: the POSITIONS handed in are not finite "
                          "(the arithmetic is left unchanged)", RuntimeWarning)
            return False
    if mode != "h3":
        warnings.warn(f"gemnet_pytorch_amd: non-finite values in {what} (arithmetic {mode!r}: no fp16 range limit involved)",
                      RuntimeWarning)
        return False
    warnings.warn(f"gemnet_pytorch_amd: non-finite values in {what} — the fp16-plane Dense arithmetic ('h3') overflows beyond "
                  "65504 (are the scale factors fitted?); this model now uses matmul_precision = 'split6' (bf16 planes, fp32 "
                  "range) and the graph is captured again", RuntimeWarning)
    model.matmul_precision = "split6"
    model._wcache = {}
    if getattr(model, "_packs", None) is not None:
        model._packs.clear()
    return True


class ForceGraphs:
    def __init__(self, model, batches, warmup=2):
        """`batches`: list of input dicts (reference keys, already on the HIP device), one per sub-batch."""
        if not batches:
            raise ValueError("at least one sub-batch")
        self.model = model
        # Private position buffers: autograd ties a leaf's gradient accumulator to the stream of its first backward
        # and keeps it on the tensor; positions that already went through an eager forward on the DEFAULT stream make
        # the capture below crash inside hipStreamEndCapture (the engine synchronises the capturing stream with the
        # default stream).  Fresh leaves see their first backward on this runner's own streams.
        self.batches = [dict(b, R=b["R"].detach().clone()) for b in batches]
        for b in self.batches:
            b.pop("_plan", None)
            if b.get("cell") is not None:     # periodic batch (pbc.py): fixed neighbour list, private cell buffer
                b["cell"] = b["cell"].detach().float().clone()
        self.periodic = [b.get("cell") is not None for b in self.batches]
        # a direct-force model (GemNet.periodic_direct_forces) has no stress: it is never asked for one
        self.with_stress = [p and not getattr(model, "direct_forces", False) for p in self.periodic]
        dev = self.batches[0]["R"].device
        if dev.type != "cuda":
            raise RuntimeError("ForceGraphs needs a HIP device (no CPU fallback)")
        self.streams = [torch.cuda.Stream(device=dev) for _ in self.batches]
        self.graphs = []
        self.outputs = []
        self.flag = RangeFlag(dev)
        self._capture(warmup)

    def _capture(self, warmup=2):
        model, dev = self.model, self.batches[0]["R"].device
        self.graphs, self.outputs = [], []
        model.eval()
        cur = torch.cuda.current_stream(dev)
        for inputs, st, stress in zip(self.batches, self.streams, self.with_stress):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                for _ in range(warmup):
                    model(inputs, stress=stress)
            cur.wait_stream(st)
        torch.cuda.synchronize(dev)
        for inputs, st, stress in zip(self.batches, self.streams, self.with_stress):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                out = model(dict(inputs, _range_flag=self.flag), stress=stress)
            self.graphs.append(g)
            self.outputs.append(out)
        torch.cuda.synchronize(dev)

    def set_positions(self, i, R):
        self.batches[i]["R"].detach().copy_(R)

    def set_cell(self, i, cell):
        """New cell of periodic sub-batch i (in place; the neighbour list and its offsets stay as captured)."""
        if not self.periodic[i]:
            raise ValueError("sub-batch %d has no cell" % i)
        self.batches[i]["cell"].copy_(cell)

    def stress(self):
        """Concatenated stress (nStructures, 3, 3) of the last replay (periodic sub-batches only, sub-batch order)."""
        if not all(self.periodic):
            raise ValueError("stress needs every sub-batch to be periodic")
        if not all(self.with_stress):
            raise ValueError("a direct-force model has no stress (its forces are not the gradient of its energy)")
        return torch.cat([o[2] for o in self.outputs])

    def replay(self):
        """Enqueue one step (all sub-batches); the calling stream waits for all of them.  A non-finite result of an EARLIER
        replay (RangeFlag, polled without synchronising) makes the model fall back to the bf16 planes and the graphs are
        captured again before this step runs."""
        if self.flag.tripped():
            self.flag.trips += 1
            torch.cuda.synchronize()
            self.flag.reset()
            if fall_back_to_bf16_planes(self.model, "a replayed forward+force graph (ForceGraphs)",
                                        positions=[b["R"] for b in self.batches]):
                self._capture()
        cur = torch.cuda.current_stream()
        for g, st in zip(self.graphs, self.streams):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                g.replay()
        for st in self.streams:
            cur.wait_stream(st)
        return self.outputs

    __call__ = replay

    def energies_forces(self):
        """Concatenated (E (nMol, T), F (nAtoms, ...)) of the last replay, sub-batch order."""
        return (torch.cat([o[0] for o in self.outputs]), torch.cat([o[1] for o in self.outputs]))


# The index build inside the replayed graph (padded.PaddedGraphRunner.attach_builder: GemNet-T and GemNet-Q).
IN_GRAPH_INDEX = os.environ.get("GEMNET_INDEX_IN_GRAPH", "1") == "1"


class DynamicForceField:
    """Energies and forces of ONE system for positions that change from call to call — the loop of the reference's ASE
    calculator (ase_calculator.py:148-170: new neighbour list every step) — at hipGraph speed:

        ff = DynamicForceField(model, Z, N_host, cutoff=5.0, int_cutoff=10.0)
        E, F = ff(R)            # R (A, 3) float32 on the device

    Every call builds the index arrays on the device (index_device.DeviceGraphBuilder, on a stream of its own), pads them to
    the current capacities and replays the one captured graph (padded.PaddedGraphRunner: bit-identical to the eager run
    on the unpadded arrays).  The capacities start `margin` above the first call's sizes; a call that outgrows them
    captures a new graph with `margin` head room again (counted in `recaptures`).  Triplets-only AND quadruplet models (the
    latter since round 5: padded.py pads interaction edges, intermediate triplets and quadruplets as well — GemNet-Q is the
    model of the reference's MD example, ase_example.ipynb cell 13).

    Periodic structures (`cell=` (B,3,3), `pbc=`; GemNet-T, and a GemNet-Q with `model.periodic_quadruplets` and
    `model.periodic_quadruplets_dynamic` set — pbc.PeriodicQuadGraphBuilder / gn_pbc_qindex_padded, all five capacities): the image neighbour list of pbc.PeriodicGraphBuilder, built inside
    the replayed graph (gn_pbc_index_padded_t) for the positions AND the cell of the step:

        ff = DynamicForceField(model, Z, N_host, cutoff, int_cutoff, cell=cell, pbc=pbc)
        E, F = ff(R)  |  ff(R, cell=new_cell);   S = ff.stress()

    The first call also sizes the in-degree bound (images: not bounded by the structure's size) with `margin` head room; a step
    that outgrows a capacity or that bound is re-sized and repeated like a molecular one, a cell the builder rejects
    (degenerate, or more than pbc.MAX_IMAGES images per side) raises the builder's `ValueError` and the last accepted cell
    is put back: the next `ff(R)` computes on it."""

    def __init__(self, model, Z, N_host, cutoff, int_cutoff, margin=0.08, max_in_degree=None, cell=None, pbc=None):
        from .index_device import DeviceGraphBuilder
        import numpy as np
        self.model, self.Z = model, Z
        self.N_host = np.asarray(N_host, dtype=np.int64).reshape(-1)
        self.N = torch.as_tensor(self.N_host, device=Z.device)
        self.margin = float(margin)
        self.periodic = cell is not None
        if self.periodic:
            from .padded import periodic_quad_opted_in
            from .pbc import PeriodicGraphBuilder, PeriodicQuadGraphBuilder
            if model.triplets_only:
                self.builder = PeriodicGraphBuilder(self.N_host, cutoff, pbc=pbc, device=Z.device)
            elif periodic_quad_opted_in(model):     # (model.periodic_quadruplets and model.periodic_quadruplets_dynamic)
                self.builder = PeriodicQuadGraphBuilder(self.N_host, cutoff, int_cutoff, pbc=pbc, device=Z.device)
            else:
                raise NotImplementedError("periodic cells: GemNet-T (triplets_only=True) only, not GemNet-Q")
            # private cell buffer: the caller's tensor may change between the step and its repetition after a re-size
            self.cell = torch.as_tensor(cell).detach().to(device=Z.device, dtype=torch.float32).reshape(-1, 3, 3).clone()
            self._good_cell = self.cell.clone()      # the last cell a completed step accepted (restored after a rejected one)
            self.deg = int(max_in_degree) if max_in_degree is not None else 0       # grown from the observed lists
        else:
            self.builder = DeviceGraphBuilder(self.N_host, cutoff, int_cutoff, model.triplets_only, device=Z.device)
            self.deg = int(max_in_degree) if max_in_degree is not None else int(self.N_host.max()) - 1
        self.runner = None
        self.recaptures = 0
        self._bstream = None

    def _build(self, R):
        main = torch.cuda.current_stream(R.device)
        if self._bstream is None:
            self._bstream = torch.cuda.Stream(device=R.device)
        self._bstream.wait_stream(main)          # the new positions come from work on the calling stream (the integrator)
        with torch.cuda.stream(self._bstream):
            if self.periodic:                            # (check_cell raises the ValueErrors of a cell it cannot serve)
                idx = self.builder(R, self.cell, dtype=torch.int32)
                idx = {k: v for k, v in idx.items() if k not in ("batch_seg", "Kidx3", "Kidx4")}
            else:
                idx = self.builder(R, dtype=torch.int32)     # as built: the padded runner keeps its index buffers in int32
        main.wait_stream(self._bstream)
        for t in idx.values():
            t.record_stream(main)
        return idx

    def __call__(self, R, cell=None, exact=True):
        """`cell` (periodic force fields): the cells of this step (kept until the next one is given).
        `exact` (the graph builds its own neighbour list): wait for the step and look at the
        device-side report of its index build — a system that outgrew the capacities is re-sized and the step repeated, as
        on the host-sized path.  With exact=False nothing waits: such a step returns NaN energies / forces and the NEXT call
        re-sizes (for callers that keep everything on the device and check `index_failed()` themselves)."""
        from .padded import PaddedGraphRunner
        if cell is not None:
            if not self.periodic:
                raise ValueError("this force field was built without a cell")
            self.cell.copy_(torch.as_tensor(cell).reshape(-1, 3, 3))
        r = self.runner
        if r is not None and r.builder is not None:
            if not r.index_error():
                # the whole step — index build included — is one replay
                out = r.run_positions(R, cell=self.cell if cell is not None else None)
                if not exact:
                    return out
                torch.cuda.current_stream(R.device).synchronize()
                if not r.index_error():
                    if cell is not None:
                        self._good_cell.copy_(self.cell)
                    return out
            err = r.index_error()
            r.reset_index_state()                   # this / an earlier step outgrew the capacities: size them anew below
            # periodic builders: the cell itself, the builder's own check says what is wrong with it.  (The molecular GemNet-Q
            # build reports I > i_cap and Q > q_cap in these two bits: capacities, re-sized below like the others.)
            if self.periodic and err & (32 | 64):
                bad = self._restore_cell()
                self.builder.check_cell(bad)
                raise ValueError(f"the in-graph neighbour list rejected the cell (index error bits {err})")
        try:
            idx = self._build(R)
        except ValueError:                          # check_cell of the host-sized build: same promise as above
            if self.periodic:
                self._restore_cell()
            raise
        if self.periodic:
            self._good_cell.copy_(self.cell)
        sizes = PaddedGraphRunner.sizes_of(idx)
        r = self.runner
        m = self.margin
        deg_now = PaddedGraphRunner.in_degree_of(idx) if self.periodic else 0
        # pad triplets need a complete quad (unit) of pad edges; the pad edges must fit the dummy groups' in-degree bound
        if r is None or not r.fits(sizes) or deg_now > r.deg:
            E, T = sizes[:2]
            if self.periodic:
                self.deg = max(self.deg, int(deg_now * (1 + m)) + 1)
            e_cap = int(E * (1 + 1.5 * m)) // 12 * 12 + 24
            t_cap = int(T * (1 + m)) // 2 * 2 + 2
            # dummy groups for the largest padding this runner may see (a later call with fewer edges pads more)
            groups = max(1, -(-int(e_cap * min(1.0, 4 * m)) // (2 * max(self.deg, 2))))
            if self.periodic:
                # small cells: the fixed head room of e_cap outweighs the margin, and a dummy atom a takes BOTH pad edges of a
                # quad — groups for the padding left when the list shrinks by 4 x margin, two incoming edges per quad
                pad_max = e_cap - int(E * (1 - min(1.0, 4 * m)))
                groups = max(1, -(-(-(-pad_max // 4)) // max(self.deg // 2, 1)))
                if not self.model.triplets_only:    # units of six, two incoming edges per unit on atoms a and b of a group
                    groups = max(1, -(-(-(-pad_max // 6)) // max(self.deg // 2, 1)))
            quad_caps = None
            if not self.model.triplets_only:
                Eint, I, Q = sizes[2:5]
                quad_caps = (int(Eint * (1 + 1.5 * m)) + 4, int(I * (1 + m)) + 4, int(Q * (1 + m)) + 4)
            pk = dict(cell=self.cell, pbc=self.builder.pbc_host) if self.periodic else {}
            self.runner = PaddedGraphRunner(self.model, self.Z, self.N, e_cap, t_cap, max_in_degree=self.deg, n_groups=groups,
                                            quad_caps=quad_caps, **pk)
            self.recaptures += self.runner is not r and r is not None
        if IN_GRAPH_INDEX and R.dtype == torch.float32:
            # from here on the index build is part of the graph (padded.attach_builder): this call's
            # arrays validate the buffers, every later call is  positions in -> one replay -> results out
            self.runner._fill(R, idx, cell=self.cell if self.periodic else None)
            if self.runner.builder is None:
                self.runner.attach_builder(self.builder)
            return self.runner.run_positions(R)
        return self.runner(R, idx, cell=self.cell if self.periodic else None)

    def _restore_cell(self):
        """A cell was rejected: put the last accepted one back (here and in the graph's static buffer), so that the next
        `ff(R)` without a cell computes on it; -> the rejected cell on the host."""
        bad = self.cell.cpu().numpy()
        self.cell.copy_(self._good_cell)
        if self.runner is not None:
            self.runner._set_cell(self.cell)
        return bad

    def stress(self):
        """Stress (B,3,3) of the last step of a periodic force field (valid until the next call)."""
        if self.periodic and getattr(self.model, "direct_forces", False):
            raise ValueError("a direct-force model has no stress (its forces are not the gradient of its energy)")
        if not self.periodic or self.runner is None:
            raise ValueError("stress needs a periodic force field that has run a step")
        return self.runner.stress()

    def index_failed(self):
        """Did a completed step's in-graph index build outgrow the capacities (its outputs are NaN)?  Exact after the caller
        waited for that step."""
        return self.runner is not None and self.runner.builder is not None and bool(self.runner.index_error())

    def range_tripped(self):
        """RangeFlag of the current runner (exact after the caller waited for the last replay)."""
        return self.runner is not None and self.runner.flag.tripped()

    def recover(self, R):
        """After `range_tripped()`: fall back to the bf16 planes, capture anew, repeat the step."""
        self.runner.recover()
        return self(R)
