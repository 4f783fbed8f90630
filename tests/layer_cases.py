"""Shared by test_layers_cpu.py / test_gpu_layers.py: replay the per-layer fixtures recorded from the
REFERENCE modules by forward hooks (tests/golden/make_golden.py::run_model2 -> model2.npz, keys
`<case>.L.<module path>.in.<i>[.<j>] / .kw.<name> / .out[.<i>]`) through the same-named modules of this package.

The reference hands its layers zero-padded / transposed tensors; the adapters below restate them in this package's
CSR form: rbf_W1 (E,I,S) -> (E,S,I); padded sph (E,S,Kmax) -> per-triplet rows sph[id_reduce[t], :, Kidx[t]].

Second half (test_layer_grads_cpu.py / test_gpu_layer_grads.py, docs/LAYER_GRADS.md): the same layers differentiated once and
twice on inputs captured from the package's own model, and the row-relative comparator against the float64 emulation."""
import contextlib
import zlib

import numpy as np
import torch

from gemnet_pytorch_amd import ops
from gemnet_pytorch_amd.graph import GraphPlan, RowIndex, SegmentPlan

LAYER_CASES = [
    ("q1L", "mlp_cbf3"), ("q1L", "mlp_sbf4"), ("q1L", "int_blocks.0.trip_interaction.mlp_cbf"),
    ("q1L", "int_blocks.0.quad_interaction.mlp_sbf"), ("q1L", "int_blocks.0.trip_interaction"),
    ("q1L", "int_blocks.0.quad_interaction"), ("q1L", "int_blocks.0.atom_update"), ("q1L", "out_blocks.1"),
    ("q1L", "int_blocks.0"),
    ("t2s", "mlp_cbf3"), ("t2s", "int_blocks.1.trip_interaction.mlp_cbf"), ("t2s", "int_blocks.1.trip_interaction"),
    ("t2s", "int_blocks.1.atom_update"), ("t2s", "out_blocks.2"), ("t2s", "int_blocks.1"),
]


class Rec:
    """The recorded tensors of one module call."""

    def __init__(self, g, case, layer, device, dtype):
        self.pre = f"{case}.L.{layer}."
        self.g, self.device, self.dtype = g, device, dtype

    def __call__(self, key):
        v = torch.tensor(self.g[self.pre + key])
        return v.to(self.device, self.dtype) if v.is_floating_point() else v.to(self.device)

    def has(self, key):
        return self.pre + key in self.g


def per_entry_sph(sph_padded_T, id_reduce, Kidx):
    """(E,S,Kmax) transposed zero-padded harmonics of the reference -> (T,S) rows."""
    return sph_padded_T[id_reduce.long(), :, Kidx.long()].contiguous()


def run_layer(model, plan, inputs, rec, layer):
    """Call `model.<layer>` on the recorded reference inputs; returns (ours, reference) lists of tensors."""
    mod = model.get_submodule(layer)
    leaf = layer.split(".")[-1]
    if leaf in ("mlp_cbf3", "mlp_sbf4"):                       # P5 EfficientInteractionDownProjection
        rbf_env = rec("in.0.0")                                 # (S, E, R); tensor basis: rows repeated (2l+1)x
        rad = rbf_env.permute(1, 0, 2)
        if leaf == "mlp_sbf4":
            L = int(round(rad.shape[1] ** 0.5))
            rad = rad[:, [l * l for l in range(L)], :]
        out = mod(rad.contiguous())                             # (E, S, I)
        return [out], [rec("out.0").permute(0, 2, 1)]
    if leaf in ("mlp_cbf", "mlp_sbf") and "interaction" in layer:   # P4 EfficientInteractionBilinear
        rbf_W1, sphT, x_t, id_reduce, Kidx = rec("in.0.0"), rec("in.0.1"), rec("in.1"), rec("in.2"), rec("in.3")
        T = x_t.shape[0]
        sp = SegmentPlan(id_reduce, torch.arange(T, device=x_t.device), rbf_W1.shape[0], T)
        out = mod(rbf_W1.permute(0, 2, 1).contiguous(), per_entry_sph(sphT, id_reduce, Kidx), x_t.contiguous(), sp)
        return [out], [rec("out")]
    if leaf == "trip_interaction":                              # P2
        m, rbf3, rbf_W1, sphT = rec("in.0"), rec("in.1"), rec("in.2.0"), rec("in.2.1")
        sph = per_entry_sph(sphT, inputs["id3_reduce_ca"], inputs["Kidx3"])
        out = mod(m, rbf3, (rbf_W1.permute(0, 2, 1).contiguous(), sph), plan)
        return [out], [rec("out")]
    if leaf == "quad_interaction":                              # P3
        m, rbf, cbf, rbf_W1, sphT = rec("in.0"), rec("in.1"), rec("in.2"), rec("in.3.0"), rec("in.3.1")
        sph = per_entry_sph(sphT, inputs["id4_reduce_ca"], inputs["Kidx4"])
        out = mod(m, rbf, cbf, (rbf_W1.permute(0, 2, 1).contiguous(), sph), plan)
        return [out], [rec("out")]
    if leaf == "atom_update":                                   # P10
        out = mod(rec("in.0"), rec("in.1"), rec("in.2"), plan.id_a)
        return [out], [rec("out")]
    if layer.startswith("out_blocks."):                         # P10 + P13 head
        E, F = mod(rec("in.0"), rec("in.1"), rec("in.2"), plan.id_a)
        ours, ref = [E], [rec("out.0")]
        if rec.has("out.1"):
            ours.append(F), ref.append(rec("out.1"))
        return ours, ref
    if layer.startswith("int_blocks.") and layer.count(".") == 1:   # P1 whole InteractionBlock[TripletsOnly]
        kw = dict(h=rec("kw.h"), m=rec("kw.m"), rbf3=rec("kw.rbf3"), rbf_h=rec("kw.rbf_h"), plan=plan,
                  rbf4=None, cbf4=None, sbf4=None)
        sph3 = per_entry_sph(rec("kw.cbf3.1"), inputs["id3_reduce_ca"], inputs["Kidx3"])
        kw["cbf3"] = (rec("kw.cbf3.0").permute(0, 2, 1).contiguous(), sph3)
        if rec.has("kw.sbf4.0"):
            sph4 = per_entry_sph(rec("kw.sbf4.1"), inputs["id4_reduce_ca"], inputs["Kidx4"])
            kw.update(rbf4=rec("kw.rbf4"), cbf4=rec("kw.cbf4"),
                      sbf4=(rec("kw.sbf4.0").permute(0, 2, 1).contiguous(), sph4))
        h, m = mod(**kw)
        return [h, m], [rec("out.0"), rec("out.1")]
    raise KeyError(layer)


def replay(model, g, case, layer, inputs, device, dtype, fused):
    """Run one recorded layer call in the fused first-order mode (what eval / inference uses: single-launch Dense,
    LDS-resident stacks, fused bilinear) or the composite mode (what force training differentiates twice)."""
    plan = GraphPlan.from_inputs(inputs, model.triplets_only)
    rec = Rec(g, case, layer, device, dtype)
    with torch.no_grad(), ops.weight_cache({}), ops.fused_first_order(fused), ops.param_grads(not fused):
        ours, ref = run_layer(model, plan, inputs, rec, layer)
    return ours, ref


# ------------------------------------------------------------------------------------------------------------------------
# Layer ADJOINTS (test_layer_grads_cpu.py / test_gpu_layer_grads.py, docs/LAYER_GRADS.md): every hot-path layer differentiated
# once (the inference adjoint, first-order training) and twice (force training: the four sweeps of ops_train.py and the
# composite closure) stand-alone, on the inputs the package's own model hands it, against the float64 emulation of the same
# pass.  Nothing below reads the recorded `.L.` fixtures: the inputs come from one forward of the model (`capture`).
GRAD_CASES = {"t2s": (True, 2), "q1L": (False, 1), "q2s": (False, 2), "t4s": (True, 4)}     # case -> (triplets_only, num_blocks)


def grad_layers(case):
    """The layers of one case: embedding, interaction blocks with their members, output blocks, basis projections.  t4s (the
    published four-block GemNet-T on 630 edges = 7 x 80 + 70, 32 atoms = 2 x 16): block 0 and the last block only."""
    T, nb = GRAD_CASES[case]
    blocks = [0, nb - 1] if case == "t4s" else list(range(nb))
    outs = [0, nb] if case == "t4s" else list(range(nb + 1))
    layers = ["edge_emb"]
    for i in blocks:
        layers += [f"int_blocks.{i}", f"int_blocks.{i}.trip_interaction"]
        if not T:
            layers.append(f"int_blocks.{i}.quad_interaction")
        layers.append(f"int_blocks.{i}.atom_update")
    layers += [f"out_blocks.{i}" for i in outs]
    layers += ["mlp_rbf3", "mlp_cbf3", "mlp_rbf_h", "mlp_rbf_out"]
    if not T:
        layers += ["mlp_rbf4", "mlp_cbf4", "mlp_sbf4"]
    return layers


def is_whole_block(layer):
    return layer.startswith("int_blocks.") and layer.count(".") == 1


def grad_passes(layer):
    """A: inference adjoint; B: first-order training; C2 / C0: force training on the fused sweeps / the composite closure;
    `*s6`: the same on the bf16 planes a model falls back to after an fp16-plane overflow (whole interaction blocks)."""
    return ["A", "B", "C2", "C0"] + (["As6", "C2s6", "C0s6"] if is_whole_block(layer) else [])


GRAD_ITEMS = [(c, l, p) for c in GRAD_CASES for l in grad_layers(c) for p in grad_passes(l)]


def round_f32(t):
    """A floating tensor rounded to the nearest float32 value, in its own dtype: both runs of a comparison get these values."""
    return t.detach().float().to(t.dtype) if t.is_floating_point() else t.detach()


def round_model_(model):
    """Parameters and floating buffers of a float64 model rounded to float32 values in place (what `.float()` keeps)."""
    with torch.no_grad():
        for t in list(model.parameters()) + list(model.buffers()):
            if t.is_floating_point():
                t.copy_(round_f32(t))
    return model


def tree_map(fn, x):
    if isinstance(x, (tuple, list)):
        return type(x)(tree_map(fn, v) for v in x)
    if isinstance(x, dict):
        return {k: tree_map(fn, v) for k, v in x.items()}
    return fn(x)


def plan_paths(plan):
    """id(object) -> attribute path for the plan and the RowIndex / SegmentPlan objects it owns (two levels)."""
    paths = {id(plan): ()}
    for k, v in vars(plan).items():
        if isinstance(v, (RowIndex, SegmentPlan)):
            paths.setdefault(id(v), (k,))
            if isinstance(v, SegmentPlan):
                paths.setdefault(id(v.reduce), (k, "reduce"))
                paths.setdefault(id(v.expand), (k, "expand"))
        elif isinstance(v, dict):
            for kk, vv in v.items():
                if isinstance(vv, RowIndex):
                    paths.setdefault(id(vv), (k, kk))
    return paths


def plan_at(plan, path):
    obj = plan
    for p in path:
        obj = obj[p] if isinstance(obj, dict) else getattr(obj, p)
    return obj


class PlanRef:
    """Stands for `plan.<path>` in captured arguments."""

    def __init__(self, path):
        self.path = path


def capture(model, inputs, layers):
    """One no_grad forward of `model` (float64, launchers emulated, inference path); per named submodule the positional and
    keyword arguments of its FIRST call, as the model passed them: floating tensors detached and rounded to float32 values,
    plan objects replaced by `PlanRef`s, everything else as it is.  (The circular basis of GemNet-Q goes through the module
    `mlp_cbf4` for the capture: on the inference path a fused kernel replaces the module call.)"""
    plan = GraphPlan.from_inputs(inputs, model.triplets_only)
    paths = plan_paths(plan)
    got, hooks = {}, []

    def strip(v):
        if isinstance(v, torch.Tensor):
            return round_f32(v).clone()
        if isinstance(v, (GraphPlan, RowIndex, SegmentPlan)):
            return PlanRef(paths[id(v)])
        return v

    for name in layers:
        def pre(mod, args, kwargs, name=name):
            if name not in got:
                got[name] = (tree_map(strip, tuple(args)), tree_map(strip, dict(kwargs)))
        hooks.append(model.get_submodule(name).register_forward_pre_hook(pre, with_kwargs=True))
    old = ops.USE_CBF_PROJECT
    ops.USE_CBF_PROJECT = False
    try:
        with torch.no_grad():
            model(inputs)
    finally:
        ops.USE_CBF_PROJECT = old
        for h in hooks:
            h.remove()
    assert set(got) == set(layers), set(layers) - set(got)
    return got


def _angles_of(ang):
    """(Q,4) (sin, cos) pairs -> the two angles (Q,) each, float64 on the host."""
    a = ang.double().cpu()
    return torch.atan2(a[:, 0], a[:, 1]), torch.atan2(a[:, 2], a[:, 3])


class Problem:
    """One layer call on one device: the module, its arguments with every floating input a leaf, and how to read results."""

    def __init__(self, model, plan, layer, captured, device, dtype, composite=False, stacked=True):
        self.mod = model.get_submodule(layer)
        self.layer = layer
        self.device, self.dtype = device, dtype
        self.leaves, self.names = [], []
        self.ang = {}          # leaf index -> (Q,4) angle-form basis replaced by its two angles on the composite closure
        self.shared = []       # leaves the model marks with ops.share_gradient (the harmonics of a (radial, harmonics) pair)
        args, kwargs = captured
        if not stacked and "tails" in kwargs:
            # the tail projections of the atom stack (the concat-Dense's atom terms) ride on the LDS-resident stack only: the
            # training forms call the atom update without them (layers._InteractionBase._update_stacked / _update), and so
            # do their stand-alone passes — the tails in the sweeps S2 .. S4 are part of the whole-block cases
            kwargs = {k: v for k, v in kwargs.items() if k != "tails"}

        def place(v, name, in_pair=None):
            if isinstance(v, torch.Tensor):
                if not v.is_floating_point():
                    return v.to(device)
                if composite and v.dim() == 2 and v.shape[1] == 4 and in_pair == 1:
                    # the tensor basis in angle form only exists on the fused kernels: the composite closure gets the two
                    # angles as one (Q,2) leaf and builds Y_lm with its own differentiable op, as GemNet.forward does there
                    th, ph = _angles_of(v)
                    # (exact in float64; a float32 run rounds them like any other input it is handed)
                    t = torch.stack([th, ph], 1).to(device, dtype).requires_grad_(True)
                    self.ang[len(self.leaves)] = int(round(49 ** 0.5))
                else:
                    t = v.to(device, dtype).requires_grad_(True)
                if in_pair == 1:
                    self.shared.append(len(self.leaves))
                self.leaves.append(t)
                self.names.append(name)
                return t
            if isinstance(v, PlanRef):
                return plan_at(plan, v.path)
            if isinstance(v, (tuple, list)):
                pair = len(v) == 2 and all(isinstance(e, torch.Tensor) and e.is_floating_point() for e in v)
                return type(v)(place(e, f"{name}.{i}", i if pair else None) for i, e in enumerate(v))
            return v

        self.args = tuple(place(v, f"in.{i}") for i, v in enumerate(args))
        self.kwargs = {k: place(v, f"kw.{k}") for k, v in kwargs.items()}
        self.params = [(n, p) for n, p in self.mod.named_parameters() if p.requires_grad]

    def call(self):
        """-> (outputs that take a cotangent, their values as the reference layer defines them)."""
        leaf_of = {id(t): i for i, t in enumerate(self.leaves)}

        def live(v):
            if isinstance(v, torch.Tensor) and id(v) in leaf_of:
                i = leaf_of[id(v)]
                if i in self.ang:
                    return ops.ylm(v[:, 0], v[:, 1], self.ang[i])
                if i in self.shared:
                    return ops.share_gradient(v)
            return v
        out = self.mod(*tree_map(live, self.args), **tree_map(live, self.kwargs))
        if isinstance(out, ops.SwappedPair):
            # the tied pair IS x3 = y_ca + y_ac[id_swap]: one cotangent, on y_ca (ops._UpPair)
            return [out.y_ca], [out.y_ca.detach() + out.y_ac.detach()[out.swap.idx64]]
        outs = [o for o in (out if isinstance(out, (tuple, list)) else [out]) if isinstance(o, torch.Tensor) and o.requires_grad]
        return outs, [o.detach() for o in outs]

    def pack(self, i, g):
        """The gradient of leaf i in the layout of the captured argument (angle form: (d theta, d phi, 0, 0))."""
        if g is None or i not in self.ang:
            return g
        out = torch.zeros((g.shape[0], 4), device=g.device, dtype=g.dtype)
        out[:, :2] = g
        return out


def problem_kw(kind):
    return dict(composite=kind.startswith("C0"), stacked=kind.startswith("A"))


def cot_key(case, layer, kind):
    """Seed of the cotangents: one per (case, layer, pass family) — both forms of pass C and both arithmetics share theirs."""
    return f"{case}/{layer}/{kind[0]}"


class Cotangents:
    """Seeded tensors, drawn in float64 on the host and rounded to float32: the same for every run of one (case, layer, pass)."""

    def __init__(self, key, device, dtype):
        self.gen = torch.Generator().manual_seed(zlib.crc32(key.encode()) & 0x7FFFFFFF)
        self.device, self.dtype = device, dtype

    def like(self, t, packed_ang=False):
        shape = (t.shape[0], 4) if packed_ang else tuple(t.shape)
        c = round_f32(torch.randn(shape, generator=self.gen, dtype=torch.float64))
        if packed_ang:
            c = c[:, :2].contiguous()
        return c.to(self.device, self.dtype)


@contextlib.contextmanager
def _contexts(fused, pgrads, t2, mode):
    with ops.exclusive(), ops.weight_cache({}), ops.fused_first_order(fused), ops.param_grads(pgrads), \
            ops.train2(t2, None), ops.chain_mode(mode), ops.position_graph(False):
        yield


def run_pass(prob, kind, key, second_order=True):
    """One pass over `prob` -> {name: tensor or None}.  Names: `out.k` (values), `d.<leaf>` / `dW.<param>` (A, B: gradients of
    sum <out_k, c_k>), and for C: `g.<leaf>` (the create_graph gradient), `dL.<leaf>`, `dLc.k`, `dLW.<param>` (gradients of
    L = sum <out_k, w_k> + sum <g_i, u_i>).  `second_order=False` drops the u term (L = sum <out_k, w_k>)."""
    mode = "split6" if kind.endswith("s6") else None
    kind = kind[:-2] if kind.endswith("s6") else kind
    cot = Cotangents(key, prob.device, prob.dtype)
    leaves, res = prob.leaves, {}
    params = [p for _, p in prob.params]
    if kind in ("A", "B"):
        with _contexts(True, kind == "B", False, mode):
            outs, vals = prob.call()
            cs = [cot.like(o) for o in outs]
            wrt = leaves + (params if kind == "B" else [])
            grads = torch.autograd.grad(outs, wrt, grad_outputs=cs, allow_unused=True)
        for k, v in enumerate(vals):
            res[f"out.{k}"] = v
        for i, n in enumerate(prob.names):
            res[f"d.{n}"] = prob.pack(i, grads[i])
        if kind == "B":
            for (n, _), g in zip(prob.params, grads[len(leaves):]):
                res[f"dW.{n}"] = g
        return res
    assert kind in ("C2", "C0")
    old = ops.USE_TRAIN2
    ops.USE_TRAIN2 = kind == "C2"
    try:
        with ops.exclusive(), ops.weight_cache({}):
            with _contexts(False, True, kind == "C2", mode):
                outs, vals = prob.call()
                cs = [cot.like(o).requires_grad_(True) for o in outs]
                ws = [cot.like(o) for o in outs]
                us = [cot.like(t, packed_ang=i in prob.ang) for i, t in enumerate(leaves)]
                with ops.param_grads(False):
                    g = torch.autograd.grad(outs, leaves, grad_outputs=cs, create_graph=True, allow_unused=True)
                L = sum((o * w).sum() for o, w in zip(outs, ws))
                if second_order:
                    for gi, u in zip(g, us):
                        if gi is not None and gi.requires_grad:
                            L = L + (gi * u).sum()
            # (the final sweep runs where loss.backward() of a training step runs: after the forward's contexts have closed)
            wrt = params + leaves + cs
            grads = torch.autograd.grad(L, wrt, allow_unused=True)
    finally:
        ops.USE_TRAIN2 = old
    for k, v in enumerate(vals):
        res[f"out.{k}"] = v
    for i, n in enumerate(prob.names):
        res[f"g.{n}"] = prob.pack(i, None if g[i] is None else g[i].detach())
        res[f"dL.{n}"] = prob.pack(i, grads[len(params) + i])
    for k in range(len(cs)):
        res[f"dLc.{k}"] = grads[len(params) + len(leaves) + k]
    for (n, _), gr in zip(prob.params, grads):
        res[f"dLW.{n}"] = gr
    return res


def order_of(name):
    """Which factor guards a tensor of pass C: its values and the create_graph gradient are first order, the rest second."""
    return 1 if name.startswith(("out.", "g.", "d.", "dW.")) else 2


# ---------------------------------------------------------------------------------------------------------------- comparator
def row_error(got, ref):
    """max over rows r of max_j |got - ref| / max(max_j |ref_r|, 1e-3 max |ref|); a 1-D (or 0-D) tensor is one row."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    rows = ref.shape[0] if ref.dim() >= 2 else 1
    got, ref = got.reshape(rows, -1), ref.reshape(rows, -1)
    d = (got - ref).abs().max(1).values
    scale = torch.maximum(ref.abs().max(1).values, 1e-3 * ref.abs().max())
    if float(ref.abs().max()) == 0.0:
        return 0.0 if float(d.max()) == 0.0 else float("inf")
    e = float((d / scale).max())
    return e if e == e else float("inf")      # (nan -> inf)


E32_FLOOR = 1e-7


def compare(got, ref, ref32, factor):
    """-> (failures, rows).  `got`, `ref`, `ref32`: {name: tensor | None} of one pass on the code under test, the float64
    emulation and the float32 emulation; a tensor's bar is factor(name) * max(e32, 1e-7) with e32 = row_error(ref32, ref), the
    reference's own float32 noise.  The sets of undefined gradients must agree.  rows: (name, e, e32, e / e32)."""
    failures, rows = [], []
    if set(got) != set(ref):
        return [("names", sorted(set(got) ^ set(ref)))], rows
    for n in ref:
        if (got[n] is None) != (ref[n] is None):
            failures.append((n, "None" if got[n] is None else "defined", "None" if ref[n] is None else "defined"))
            continue
        if ref[n] is None:
            continue
        e32 = max(row_error(ref32[n], ref[n]), E32_FLOOR)
        e = row_error(got[n], ref[n])
        rows.append((n, e, e32, e / e32))
        if not e <= factor(n) * e32:
            failures.append((n, e, e32))
    return failures, rows


# ------------------------------------------------------------------------------------------------------------------ the cases
class GradCase:
    """Models (float64 and float32 on the emulated launchers), plan and captured layer inputs of one fixture; built once per
    session.  Reference results are cached per (layer, pass, dtype): several tests read them, nobody writes them."""
    _cache = {}

    @classmethod
    def get(cls, g, case):
        if case not in cls._cache:
            cls._cache[case] = cls(g, case)
        return cls._cache[case]

    def __init__(self, g, case):
        import cpu_kernels
        from test_model_cpu import build
        from test_oracle_model import load_case
        self.case = case
        self.cfg, self.params, self.inputs = load_case(g, case)
        self.inputs["R"] = self.inputs["R"].double()
        with cpu_kernels.emulate():
            self.model64 = round_model_(build(self.cfg, self.params)).eval()
            self.captured = capture(self.model64, self.inputs, grad_layers(case))
        self.model32 = build(self.cfg, self.params, dtype=torch.float32).eval()
        self.plan = GraphPlan.from_inputs(self.inputs, self.model64.triplets_only)
        self._ref = {}

    def problem(self, layer, kind, dtype=torch.float64):
        model = self.model64 if dtype == torch.float64 else self.model32
        return Problem(model, self.plan, layer, self.captured[layer], "cpu", dtype, **problem_kw(kind))

    def reference(self, layer, kind, dtype=torch.float64, second_order=True):
        """The pass on the emulated launchers (float64: the reference; float32: its own rounding noise)."""
        import cpu_kernels
        k = (layer, kind, dtype, second_order)
        if k not in self._ref:
            with cpu_kernels.emulate():
                self._ref[k] = run_pass(self.problem(layer, kind, dtype), kind, cot_key(self.case, layer, kind), second_order)
        return self._ref[k]
