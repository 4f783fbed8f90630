"""-m gpu: the adjoints of every hot-path layer on the HIP kernels against float64 (tests/layer_cases.py, docs/LAYER_GRADS.md).

Per (case, layer, pass) one stand-alone call of the layer on the inputs the package's own model hands it (captured from one
forward, rounded to float32, the same values on both sides), differentiated
  A   once on the inference path (LDS-resident stacks, fused bilinear / up-projection pair / aggregation, constant weights),
  B   once with parameter gradients (direct-force and energy-only training),
  C2  twice on the four-sweep force-training form (ops_train.py: S2, S3, S4 with the f'' source terms),
  C0  twice on the composite closure,
and, for whole interaction blocks, A / C2 / C0 on the bf16 planes ("split6") a model falls back to after an fp16-plane overflow.
Every result tensor is compared row by row (layer_cases.row_error) with the float64 emulation of the same pass; its bar is
FACTOR x the error of the float32 emulation of that pass against the float64 one (floored at 1e-7) — the reference's own
float32 noise, measured inside the test.  The factors were fixed after the first run on an MI355X at twice the worst measured
ratio, rounded up to a power of two (docs/LAYER_GRADS.md holds the table)."""
from collections import Counter

import pytest
import torch

import cpu_kernels
import layer_cases as LC
from layer_cases import GRAD_CASES, GRAD_ITEMS, GradCase, Problem, compare, cot_key, order_of, problem_kw, run_pass
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd import ops
from gemnet_pytorch_amd.graph import GraphPlan

pytestmark = pytest.mark.gpu
DEV = "cuda"
# one number per pass kind: A / B, pass C first order (values and the create_graph gradient), pass C second order.
# Worst measured e / e32 on an MI355X: 4.23 (B, t4s int_blocks.3.atom_update dW.dense_rbf.weight), 3.24 (C2, q1L out_blocks.1
# out.0), 10.02 (C0, t4s int_blocks.3.trip_interaction dLW.mlp_rbf.weight) -> twice that, rounded up to a power of two
FACTOR = {"AB": 16.0, "C1": 8.0, "C2": 32.0}
WIDE = ("t2s", "q2s", "t4s")            # the published widths (128 / 64 / 16): the shapes the fused kernels are built for
COUNTED = cpu_kernels._NAMES


def factor_of(kind):
    if kind[0] in "AB":
        return lambda name: FACTOR["AB"]
    return lambda name: FACTOR["C1"] if order_of(name) == 1 else FACTOR["C2"]


class DeviceCase:
    _cache = {}

    @classmethod
    def get(cls, g, case):
        if case not in cls._cache:
            cls._cache[case] = cls(g, case)
        return cls._cache[case]

    def __init__(self, g, case):
        from test_gpu_model import build, to_dev
        self.host = GradCase.get(g, case)
        self.model = build(self.host.cfg, self.host.params).eval()
        inputs = to_dev({k: v for k, v in self.host.inputs.items() if k != "_plan"})
        inputs["R"] = inputs["R"].float()
        self.plan = GraphPlan.from_inputs(inputs, self.model.triplets_only).warm()
        self.inputs = inputs

    def run(self, layer, kind, count=None):
        prob = Problem(self.model, self.plan, layer, self.host.captured[layer], DEV, torch.float32, **problem_kw(kind))
        saved = {}
        if count is not None:
            for n in COUNTED:
                f = getattr(K, n)
                saved[n] = f
                setattr(K, n, (lambda *a, _f=f, _n=n, **k: (count.update([_n]), _f(*a, **k))[1]))
        try:
            res = run_pass(prob, kind, cot_key(self.host.case, layer, kind))
            torch.cuda.synchronize()
        finally:
            for n, f in saved.items():
                setattr(K, n, f)
        return res


def _report(tag, rows):
    for name, e, e32, ratio in rows:
        print(f"LAYER_GRADS {tag} {name} e={e:.3e} e32={e32:.3e} ratio={ratio:.2f}")


def _has_stack(layer):
    return layer.startswith(("int_blocks.", "out_blocks."))


@pytest.mark.parametrize("case,layer,kind", GRAD_ITEMS)
def test_layer_pass_against_float64(golden_model2, case, layer, kind):
    dc = DeviceCase.get(golden_model2, case)
    host = dc.host
    ref, r32 = host.reference(layer, kind), host.reference(layer, kind, torch.float32)
    cnt = Counter()
    up0 = ops.BIL_UP_CALLS
    got = dc.run(layer, kind, cnt)
    failures, rows = compare(got, ref, r32, factor_of(kind))
    _report(f"{case} {layer} {kind}", rows)
    assert rows and not failures, failures
    # the pass ran what it is named for
    base = kind[:2] if kind.startswith("C") else kind[0]
    leaf = layer.split(".")[-1]
    if base == "C0":
        assert cnt["chain"] == 0, cnt
    elif _has_stack(layer) and base in ("A", "C2"):
        assert cnt["chain"] > 0, cnt
    if base == "A" and case in WIDE:
        if leaf == "trip_interaction" or LC.is_whole_block(layer):
            if GRAD_CASES[case][0] and kind == "A":
                # GemNet-T on the fp16 planes: the bilinear layer and the up-projection pair are ONE launch each way
                assert ops.BIL_UP_CALLS == up0 + 1, (ops.BIL_UP_CALLS, up0)
            assert cnt["bil_fused_fwd"] >= 1 and cnt["bil_fused_bwd"] >= 1, cnt
        if leaf == "atom_update" or layer.startswith("out_blocks."):
            assert cnt["rbf_aggregate_fwd"] >= 1 and cnt["rbf_aggregate_bwd"] >= 1, cnt
    # no atomics anywhere: the same pass again gives the same bits
    again = dc.run(layer, kind)
    for name, t in got.items():
        assert (t is None) == (again[name] is None) and (t is None or torch.equal(t, again[name])), name


# ------------------------------------------------------------------------------------------------------------ output group
@pytest.mark.parametrize("case", ["t2s", "t4s"])
def test_output_group_adjoint_against_float64(golden_model2, case):
    """ops.output_group — all output blocks of a GemNet-T force pass as one grouped launch per stage, the default inference
    path, reached by no module hook — on the captured inputs of ALL output blocks: the sum of the blocks' energies and its
    gradients w.r.t. every block's m and the shared radial projection, against the per-block float64 emulation."""
    dc = DeviceCase.get(golden_model2, case)
    host = dc.host
    nb = GRAD_CASES[case][1]
    CK = cpu_kernels
    # (t4s captures two of its five output blocks for the per-layer items: the group needs all of them)
    names = [f"out_blocks.{i}" for i in range(nb + 1)]
    with CK.emulate():
        cap = LC.capture(host.model64, host.inputs, names)
    hs, ms = [cap[n][0][0] for n in names], [cap[n][0][1] for n in names]
    rbf = cap[names[0]][0][2]
    assert all(torch.equal(cap[n][0][2], rbf) for n in names)
    cot = LC.Cotangents(f"{case}/output_group", "cpu", torch.float64).like(torch.empty(host.plan.n_atoms, 1))

    def host_pass(model, dtype):
        with CK.emulate(), LC._contexts(True, False, False, None):
            m_l = [m.to(dtype).requires_grad_(True) for m in ms]
            r_l = rbf.to(dtype).requires_grad_(True)
            E = None
            for i, m in enumerate(m_l):
                E = model.out_blocks[i](hs[i].to(dtype), m, r_l, host.plan.id_a, E_sum=E)[0]
            grads = torch.autograd.grad(E, m_l + [r_l], grad_outputs=cot.to(dtype))
        return dict(E=E.detach(), rbf=grads[-1], **{f"m{i}": g for i, g in enumerate(grads[:-1])})

    ref, r32 = host_pass(host.model64, torch.float64), host_pass(host.model32, torch.float32)

    def device_pass():
        with LC._contexts(True, False, False, None):
            m_l = [m.to(DEV, torch.float32).requires_grad_(True) for m in ms]
            r_l = rbf.to(DEV, torch.float32).requires_grad_(True)
            blocks = dc.model._out_group_blocks(dc.inputs["R"], m_l[0], r_l)
            assert blocks is not None and ops.output_group_supported(blocks, m_l, r_l)
            n0 = ops.OUT_GROUP_CALLS
            E = ops.output_group(blocks, m_l, r_l, dc.plan.id_a, s=2.0 ** -0.5)
            assert ops.OUT_GROUP_CALLS == n0 + 1
            grads = torch.autograd.grad(E, m_l + [r_l], grad_outputs=cot.to(DEV, torch.float32))
            torch.cuda.synchronize()
        return dict(E=E.detach(), rbf=grads[-1], **{f"m{i}": g for i, g in enumerate(grads[:-1])})

    got = device_pass()
    failures, rows = compare(got, ref, r32, lambda n: FACTOR["AB"])
    _report(f"{case} output_group A", rows)
    assert rows and not failures, failures
    again = device_pass()
    assert all(torch.equal(got[n], again[n]) for n in got)


# ------------------------------------------------------------------------------------------------- padded quadruplet batch
def test_quad_interaction_adjoint_on_a_padded_batch(golden_model2):
    """The quadruplet x-adjoint reads graph.SegmentPlan.row_grid; on a padded batch (padded.py, `max_in_degree` given) the grid
    is built with static capacities from index arrays whose pad quadruplets collide on cells and pair edges and rows of
    different dummy atoms (tests/test_padded_cpu.py::test_row_grid_of_padded_quadruplet_batches).  Pass A of the quadruplet
    interaction on q2s padded with two dummy groups: the rows of the real molecules meet the comparator, and two runs — each
    on an index plan of its own — agree bit for bit INCLUDING the pad rows."""
    from test_gpu_model import to_dev
    from test_padded_cpu import _padded_quad_inputs
    layer, kind = "int_blocks.0.quad_interaction", "A"
    dc = DeviceCase.get(golden_model2, "q2s")
    host = dc.host
    extra = (40, 50, 6, 30, 400)
    padded, A, n_mol = _padded_quad_inputs({k: v for k, v in host.inputs.items() if k != "_plan"}, 2, extra)
    real = {int(padded[k].shape[0]): int(host.inputs[k].shape[0])
            for k in ("id_c", "id4_expand_intm_db", "id4_reduce_ca")}          # padded rows -> real rows (edges, intm, quads)
    assert len(real) == 3
    with cpu_kernels.emulate():
        cap = LC.capture(host.model64, padded, [layer])[layer]
    plan = GraphPlan.from_inputs(padded, False)
    assert plan.quad._ab_max_rows == 64
    key = cot_key("q2s-padded", layer, kind)

    def host_pass(model, dtype):
        with cpu_kernels.emulate():
            return run_pass(Problem(model, plan, layer, cap, "cpu", dtype, **problem_kw(kind)), kind, key)

    def device_pass():
        inputs = to_dev({k: v for k, v in padded.items() if k not in ("_plan", "max_in_degree")})
        inputs.update(R=inputs["R"].float(), max_in_degree=64)
        dplan = GraphPlan.from_inputs(inputs, False).warm()
        assert dplan.quad.row_grid is not None
        res = run_pass(Problem(dc.model, dplan, layer, cap, DEV, torch.float32, **problem_kw(kind)), kind, key)
        torch.cuda.synchronize()
        return res

    def real_rows(res):
        return {n: (t if t is None or t.dim() < 2 or t.shape[0] not in real else t[:real[t.shape[0]]]) for n, t in res.items()}

    ref, r32 = real_rows(host_pass(host.model64, torch.float64)), real_rows(host_pass(host.model32, torch.float32))
    got = device_pass()
    failures, rows = compare(real_rows(got), ref, r32, factor_of(kind))
    _report(f"q2s-padded {layer} {kind}", rows)
    assert rows and not failures, failures
    assert any(t is not None and t.dim() == 2 and t.shape[0] in real for t in got.values())
    again = device_pass()
    for name, t in got.items():
        assert (t is None) == (again[name] is None) and (t is None or torch.equal(t, again[name])), name
