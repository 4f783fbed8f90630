"""Layer adjoints on the CPU emulation (tests/layer_cases.py, docs/LAYER_GRADS.md): every hot-path layer of t2s, q1L, q2s and
t4s differentiated twice stand-alone on the inputs the package's own model hands it —
  * the four-sweep force-training form (ops_train.py) equals the composite closure in float64, for the create_graph gradient
    and every gradient of L = sum <out, w> + sum <g, u>;
  * the comparator of test_gpu_layer_grads.py passes on the float32 emulation at factor 2 and FAILS on the float64 reference
    with each of the errors it is there to find planted into it."""
import pytest
import torch

import layer_cases as LC
from layer_cases import GRAD_CASES, GradCase, compare, grad_layers, order_of

LAYERS = [(c, l) for c in GRAD_CASES for l in grad_layers(c)]


def _is_angle_leaf(gc, layer, name):
    """Is `name` a gradient of the tensor basis in angle form (the (Q,4) harmonics argument of a GemNet-Q layer)?"""
    prob = gc.problem(layer, "C0")
    return any(name.endswith("." + prob.names[i]) for i in prob.ang)


@pytest.mark.parametrize("case,layer", LAYERS)
def test_train2_equals_composite_closure(golden_model2, case, layer):
    gc = GradCase.get(golden_model2, case)
    a, b = gc.reference(layer, "C2"), gc.reference(layer, "C0")
    assert set(a) == set(b)
    worst, n = 0.0, 0
    for name in b:
        if a[name] is None and b[name] is not None and name.startswith("dL.") and _is_angle_leaf(gc, layer, name):
            # the angle-form twins of the quadruplet layer carry no Hessian of the two angles (ops.position_graph): nothing
            # that training asks for depends on it, and the fused form returns no gradient there
            continue
        assert (a[name] is None) == (b[name] is None), name
        if b[name] is None:
            continue
        scale = float(b[name].abs().max())
        err = float((a[name] - b[name]).abs().max())
        worst, n = max(worst, err / max(scale, 1e-300)), n + 1
        assert err <= 1e-11 * scale, (name, err, scale)
    assert n >= 5
    print(f"{case} {layer}: train2 vs composite, {n} tensors, worst {worst:.1e} of max")


@pytest.mark.parametrize("kind", ["A", "B", "C2", "C0"])
@pytest.mark.parametrize("case,layer", LAYERS)
def test_comparator_passes_on_the_float32_emulation(golden_model2, case, layer, kind):
    gc = GradCase.get(golden_model2, case)
    ref, r32 = gc.reference(layer, kind), gc.reference(layer, kind, torch.float32)
    failures, rows = compare(r32, ref, r32, lambda n: 2.0)
    assert not failures and rows


# ---------------------------------------------------------------------------------------------------- planted errors
PLANT = [("t2s", "int_blocks.1"), ("t2s", "int_blocks.1.trip_interaction"), ("t2s", "int_blocks.1.atom_update"),
         ("t2s", "out_blocks.2"), ("q2s", "int_blocks.0.quad_interaction"), ("q1L", "int_blocks.0"), ("t4s", "int_blocks.3")]
FACTOR = 32.0           # the largest factor the GPU test may use: what fails here fails there


def _tile_tail(t, case):
    """First row of the last partial row tile of a gradient with edge rows (80-row tiles) or atom rows (16-row tiles)."""
    A = {"t2s": 21, "q1L": 12, "q2s": 21, "t4s": 32}[case]
    E = {"t2s": 168, "q1L": 96, "q2s": 168, "t4s": 630}[case]
    if t.dim() == 2 and t.shape[0] == E and E % 80:
        return 80 * (E // 80)
    if t.dim() == 2 and t.shape[0] == A and A % 16:
        return 16 * (A // 16)
    return None


def _planted(gc, layer, kind):
    ref, r32 = gc.reference(layer, kind), gc.reference(layer, kind, torch.float32)
    return ref, r32, {n: (None if v is None else v.clone()) for n, v in ref.items()}


@pytest.mark.parametrize("kind", ["A", "C2"])
@pytest.mark.parametrize("case,layer", PLANT)
def test_comparator_sees_a_zeroed_last_row_tile(golden_model2, case, layer, kind):
    """(i) rows >= 80 floor(M / 80) (edge rows) resp. 16 floor(A / 16) (atom rows) of ONE gradient zeroed."""
    gc = GradCase.get(golden_model2, case)
    ref, r32, _ = _planted(gc, layer, kind)
    hit = 0
    for name, t in ref.items():
        if t is None or name.startswith("out.") or _tile_tail(t, case) is None:
            continue
        r0 = _tile_tail(t, case)
        if float(t[r0:].abs().max()) == 0.0:
            continue
        bad = dict(ref)
        bad[name] = t.clone()
        bad[name][r0:] = 0
        failures, _ = compare(bad, ref, r32, lambda n: FACTOR)
        assert [f[0] for f in failures] == [name], (name, failures)
        hit += 1
    assert hit >= 1


@pytest.mark.parametrize("kind", ["A", "B", "C2"])
@pytest.mark.parametrize("case,layer", PLANT)
def test_comparator_sees_one_scaled_row(golden_model2, case, layer, kind):
    """(ii) one single row of one tensor scaled by 1 + 64 * bar — every tensor in turn, the row with the smallest maximum
    that is still above the comparator's floor (the hardest one to see)."""
    gc = GradCase.get(golden_model2, case)
    ref, r32, _ = _planted(gc, layer, kind)
    hit = 0
    for name, t in ref.items():
        if t is None or float(t.abs().max()) == 0.0:
            continue
        e32 = max(LC.row_error(r32[name], t), LC.E32_FLOOR)
        rows = t.reshape(t.shape[0] if t.dim() >= 2 else 1, -1)
        mx = rows.abs().max(1).values
        ok = torch.nonzero(mx >= 1e-3 * mx.max())[:, 0]
        r = int(ok[torch.argmin(mx[ok])])
        bad = dict(ref)
        b = rows.clone()
        b[r] *= 1.0 + 64.0 * FACTOR * e32
        bad[name] = b.reshape(t.shape)
        failures, _ = compare(bad, ref, r32, lambda n: FACTOR)
        assert [f[0] for f in failures] == [name], (name, failures)
        hit += 1
    assert hit >= 3


@pytest.mark.parametrize("kind", ["C2", "C0"])
@pytest.mark.parametrize("case,layer", PLANT)
def test_comparator_sees_missing_second_order_terms(golden_model2, case, layer, kind):
    """(iii) pass C with u = 0: every contribution that reaches L through the create_graph gradient is missing."""
    gc = GradCase.get(golden_model2, case)
    ref, r32 = gc.reference(layer, kind), gc.reference(layer, kind, torch.float32)
    bad = gc.reference(layer, kind, second_order=False)
    # (a gradient that exists only through the u term is undefined without it: its missing value is zero)
    bad = {n: (torch.zeros_like(ref[n]) if bad[n] is None and ref[n] is not None else bad[n]) for n in ref}
    failures, _ = compare(bad, ref, r32, lambda n: FACTOR)
    failed = {f[0] for f in failures}
    # first-order quantities do not depend on u; every parameter gradient and the gradient w.r.t. the cotangents do
    assert not any(order_of(n) == 1 for n in failed), failed
    second = [n for n in ref if ref[n] is not None and n.startswith(("dLW.", "dLc."))]
    assert second and all(n in failed for n in second), sorted(set(second) - failed)


@pytest.mark.parametrize("case,layer", PLANT)
def test_comparator_sees_a_first_order_parameter_gradient(golden_model2, case, layer):
    """(iv) one parameter's gradient of pass C replaced by that of pass B with the cotangent w (L without the u term): the
    mu_z^T da term is missing."""
    gc = GradCase.get(golden_model2, case)
    ref, r32 = gc.reference(layer, "C2"), gc.reference(layer, "C2", torch.float32)
    first = gc.reference(layer, "C2", second_order=False)
    names = [n for n in ref if n.startswith("dLW.") and ref[n] is not None and first[n] is not None]
    assert len(names) >= 3
    for name in names:
        bad = dict(ref)
        bad[name] = first[name]
        failures, _ = compare(bad, ref, r32, lambda n: FACTOR)
        assert [f[0] for f in failures] == [name], (name, failures)
