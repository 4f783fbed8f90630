"""-m gpu: scale-factor fitting on periodic batches (GemNet.periodic_scale_fitting, training.periodic.fit_scale_factors).
Kernel (red zone): gn_col_var_f32 against torch.var of the gathered rows in float64 — every width, row counts around the trip and
block sizes, with and without an index, one source row, an ill-conditioned column, accumulation, repeatability, refusals.
Model: the direct-force golden fit of the REFERENCE classes (tests/golden/scaling_fit.json) reproduced through cells without an
image inside the cutoff; autograd-force GemNet-T / -Q in such cells against the float64 host molecular fit; cells WITH images
against the float64 host emulation of the same periodic fit (recorded in tests/golden/pbc_fit_host.json); invariance under moves
by lattice vectors; GEMNET_FIT_STAT=0 against 1; what raises; the fitted model against a fresh one built from the written json;
the launches of a fit-mode pass."""
import json
import os

import numpy as np
import pytest
import torch

import pbc_fit_common as FC
import pbc_q_common as Q
from conftest import GOLDEN
from gemnet_pytorch_amd import _lib
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd.model import scaling
from gemnet_pytorch_amd.model.scaling import AutomaticFit
from oracle import gemnet_oracle as GO
from redzone import put, redzone_on_request  # noqa: F401  (the kernel-level tests below ask for `redzone`: they run under the red-zone harness)

pytestmark = pytest.mark.gpu
DEV = FC.DEV
REL = 1e-6          # float64 shifted sums of exact float32 inputs are good to ~1e-12; a float32 / naive sum misses by 1e-3
NS = (2, 3, 63, 64, 65, 255, 257, 4097)


# ----------------------------------------------------------------------------------------------------------------- kernel
def _stat(x, idx, w=1.0, acc=None, slot=0):
    acc = torch.zeros(3, device=DEV, dtype=torch.float64) if acc is None else acc
    K.col_var(x, idx, acc, slot, w)
    return acc


@pytest.mark.parametrize("C", K.COL_VAR_WIDTHS)
def test_col_var_matches_float64_var_of_the_gathered_rows(C, redzone):      # noqa: F811
    rs = np.random.RandomState(100 + C)
    worst = 0.0
    for n in NS:
        n_src = max(5, n // 3 + 7)
        xh = torch.tensor(rs.standard_normal((n_src, C)) * rs.uniform(0.5, 2.0, C) + rs.uniform(-3, 3, C), dtype=torch.float32)
        ih = torch.tensor(rs.randint(0, n_src - 3, n), dtype=torch.int32)            # unsorted, repeats; the last rows never named
        x, idx = put(xh), put(ih)
        xn = put(xh[:n].contiguous()) if n <= n_src else put(torch.tensor(rs.standard_normal((n, C)), dtype=torch.float32))
        for xx, ix in ((x, idx), (xn, None)):
            acc = _stat(xx, ix, slot=1)
            ref = FC.col_var_reference(xx, ix)
            got = acc.cpu().tolist()
            assert got[0] == 0.0 and got[2] == 0.0                                  # the other slots are not touched
            if ref == 0.0:
                assert got[1] == 0.0
            else:
                worst = max(worst, abs(got[1] - ref) / ref)
                assert abs(got[1] - ref) <= REL * ref, (n, C, ix is not None, got[1], ref)
            assert torch.equal(_stat(xx, ix, slot=1), acc)                          # two runs: the same bits
    print(f"gn_col_var_f32, C = {C}: worst relative error against float64 torch.var {worst:.2e}")


@pytest.mark.parametrize("C", (8, 128))
def test_col_var_of_one_source_row_is_exactly_zero(C, redzone):      # noqa: F811
    x = put(torch.tensor(np.random.RandomState(1).standard_normal((1, C)) * 1e3, dtype=torch.float32))
    for n in (2, 65, 4097):
        acc = _stat(x, put(torch.zeros(n, dtype=torch.int32)), w=7.0)
        assert acc.cpu().tolist() == [0.0, 0.0, 0.0]


def test_col_var_survives_a_mean_far_above_the_spread(redzone):      # noqa: F811
    """1e5 rows, C = 32, column means ~ 1e3, spread ~ 1e-2 (variance 1e-4 under squares of 1e6): relative error <= 1e-6, with
    the rows as they are and gathered."""
    rs = np.random.RandomState(7)
    xh = torch.tensor(1e3 * rs.uniform(0.5, 1.5, 32) + 1e-2 * rs.standard_normal((100000, 32)), dtype=torch.float32)
    x = put(xh)
    idx = put(torch.tensor(rs.randint(0, 100000, 100000), dtype=torch.int32))
    for ix in (None, idx):
        got, ref = float(_stat(x, ix)[0]), FC.col_var_reference(x, ix)
        print(f"ill-conditioned column variance ({'gathered' if ix is not None else 'plain'}): relative error "
              f"{abs(got - ref) / ref:.2e} (float32 torch.var: {abs(float(torch.var(x if ix is None else x[ix.long()], dim=0).mean()) - ref) / ref:.2e})")
        assert abs(got - ref) <= REL * ref


def test_col_var_accumulates_weighted_terms(redzone):      # noqa: F811
    rs = np.random.RandomState(3)
    x1 = put(torch.tensor(rs.standard_normal((300, 64)), dtype=torch.float32))
    x2 = put(torch.tensor(rs.standard_normal((77, 64)) * 3, dtype=torch.float32))
    i2 = put(torch.tensor(rs.randint(0, 77, 500), dtype=torch.int32))
    w1, w2 = 300.0, 0.125
    acc = _stat(x1, None, w=w1, slot=2)
    _stat(x2, i2, w=w2, acc=acc, slot=2)
    v1, v2 = float(_stat(x1, None)[0]), float(_stat(x2, i2)[0])
    assert acc.cpu().tolist()[:2] == [0.0, 0.0] and float(acc[2]) == w1 * v1 + w2 * v2
    ref = w1 * FC.col_var_reference(x1) + w2 * FC.col_var_reference(x2, i2)
    assert abs(float(acc[2]) - ref) <= REL * ref


def test_col_var_launcher_rejects_without_launching(redzone):      # noqa: F811
    acc = torch.zeros(1, device=DEV, dtype=torch.float64)
    x = put(torch.ones(4, 32))
    n0 = redzone.n_launches
    with pytest.raises(ValueError, match="two rows"):
        K.col_var(x, put(torch.zeros(1, dtype=torch.int32)), acc, 0, 1.0)                    # n = 1
    with pytest.raises(ValueError, match="two rows"):
        K.col_var(put(torch.ones(1, 32)), None, acc, 0, 1.0)
    with pytest.raises(ValueError, match="width 24"):
        K.col_var(put(torch.ones(4, 24)), None, acc, 0, 1.0)                                # an unlisted C
    with pytest.raises(TypeError, match="contiguous float32"):
        K.col_var(put(torch.ones(4, 64))[:, ::2], None, acc, 0, 1.0)                        # not contiguous
    with pytest.raises(TypeError, match="contiguous float32"):
        K.col_var(put(torch.ones(4, 32, dtype=torch.float64)), None, acc, 0, 1.0)           # not float32
    with pytest.raises(ValueError, match="slot"):
        K.col_var(x, None, acc, 1, 1.0)
    assert redzone.n_launches == n0 and float(acc[0]) == 0.0
    # the C entry point itself: hipErrorInvalidValue (1) before any launch
    ws = torch.empty(_lib.GN_COL_VAR_MAX_BLOCKS * 2 * 32, device=DEV, dtype=torch.float64)
    lib = _lib.load()
    for n_src, n, C in ((4, 1, 32), (4, 4, 24), (4, 5, 32)):
        assert lib.gn_col_var_f32(_lib.ptr(x), None, _lib.ptr(ws), _lib.ptr(acc), n_src, n, C, 0, 1.0, _lib.stream()) == 1
    torch.cuda.synchronize()
    assert float(acc[0]) == 0.0


# ---------------------------------------------------------------------------------- cells without an image inside the cutoff
def _golden(tag):
    with open(os.path.join(GOLDEN, "scaling_fit.json")) as f:
        return json.load(f)[tag]


def _container(g, cfg):
    from gemnet_pytorch_amd.training.data_container import DataContainer
    data = dict(N=np.array(g["N"], np.int32), Z=np.array(g["Z"], np.int32), R=np.array(g["R"], np.float32),
                E=np.zeros(len(g["N"]), np.float32), F=np.zeros((len(g["Z"]), 3), np.float32))
    return DataContainer.from_arrays(data, 5.0, 10.0, triplets_only=cfg["triplets_only"])


def _boxed_structs(g, margin):
    """The golden's molecules, each in a cubic all-periodic cell of edge extent + margin."""
    R, Z, off, out = np.array(g["R"], np.float32).astype(np.float64), np.array(g["Z"]), 0, []
    for n in g["N"]:
        cell, pbc = FC.boxed(R[off:off + n], margin)
        out.append((R[off:off + n], Z[off:off + n], cell, pbc))
        off += n
    return out


def _boxed_batches(g, family, cfg, margin):
    """Periodic device batches [[0, 1], [2]] of the boxed molecules; their index arrays are the molecular ones, array for array."""
    structs, dc = _boxed_structs(g, margin), _container(g, cfg)
    batches = []
    for ids in g["batches"]:
        b = FC.device_batch(family, [structs[i] for i in ids], cutoff=5.0, int_cutoff=10.0)
        mol = dc[ids]
        shared = [k for k in mol if k in b and k not in ("R", "Z", "N", "E", "F")]
        assert {"id_a", "id_c", "id_swap", "id3_reduce_ca", "id3_expand_ba", "batch_seg"} <= set(shared)
        assert family != "Q" or {"id4_reduce_ca", "id4_expand_db", "id4_expand_abd", "id4_int_a"} <= set(shared)
        for k in shared:
            assert torch.equal(b[k].cpu().long().reshape(-1), mol[k].cpu().long().reshape(-1)), k
        assert int(b["cell_offsets"].abs().max()) == 0 and (family != "Q" or int(b["int_cell_offsets"].abs().max()) == 0)
        batches.append(b)
    return batches, dc


def test_direct_force_fit_reproduces_the_reference_fit_through_cells(tmp_path):
    """GemNet-dT: tests/golden/scaling_fit.json["T"] was fitted by the reference's own classes in float64 on molecules; the
    same molecules in cells of edge extent + 2 cutoff + 1 A have the molecular index arrays, so the periodic fit must give the
    reference's factors: same order, 2e-3 relative (the bar of tests/test_gpu_scaling_fit.py on the same golden)."""
    g = _golden("T")
    cfg = g["cfg"]
    assert cfg["direct_forces"] and cfg["triplets_only"]
    batches, _ = _boxed_batches(g, "dT", cfg, 2 * 5.0 + 1.0)
    params = GO.make_params(cfg, g["seed"], None, torch.float64)
    _, order, fitted = FC.fit_periodic("dT", cfg, params, batches, FC.new_scale_file(tmp_path / "s.json"), DEV)
    assert order == g["order"]
    w = FC.worst(fitted, g["fitted"])
    print(f"periodic GemNet-dT fit against the reference's float64 fit: {len(fitted)} factors, worst relative deviation {w:.2e}")
    for k, v in g["fitted"].items():
        assert abs(fitted[k] - v) <= 2e-3 * abs(v), (k, fitted[k], v)


@pytest.mark.parametrize("tag", ["T", "Q"])
def test_autograd_force_fit_in_cells_matches_the_host_molecular_fit(tag, tmp_path):
    """The golden configuration with direct_forces=False (Q: cell edge extent + 2 int_cutoff + 1 A) against the float64
    host-emulated MOLECULAR fit of the same parameters on the same batches: equal order, 2e-3 relative.  (The oracle is computed
    here, on the host: it is most of this test's time — about 8 s for GemNet-Q's 2 x 8 float64 passes over 26 atoms.)"""
    g = _golden(tag)
    cfg = dict(g["cfg"], direct_forces=False)
    margin = 2 * (5.0 if tag == "T" else 10.0) + 1.0
    batches, dc = _boxed_batches(g, tag, cfg, margin)
    params = GO.make_params(cfg, g["seed"], None, torch.float64)
    mol = []
    for ids in g["batches"]:
        b = {k: v for k, v in dc[ids].items() if k not in ("E", "F")}
        b["R"] = b["R"].double()
        mol.append(b)
    order_ref, ref = FC.fit_molecular_host(cfg, params, mol, FC.new_scale_file(tmp_path / "ref.json"))
    _, order, fitted = FC.fit_periodic(tag, cfg, params, batches, FC.new_scale_file(tmp_path / "s.json"), DEV)
    assert order == order_ref and len(order) == len(g["order"]) - 2          # (no `_had` factors of the direct force heads)
    w = FC.worst(fitted, ref)
    print(f"periodic GemNet-{tag} fit in image-free cells against the float64 host molecular fit: {len(fitted)} factors, worst "
          f"relative deviation {w:.2e}")
    assert w <= 2e-3


# --------------------------------------------------------------------------------------------------------------- real images
def _device_fit(family, split, tmp_path, structs=None, name="dev"):
    structs = structs or FC.structures()
    params = GO.make_params(FC.CFGS[family], FC.SEED, None, torch.float64)
    batches = [FC.device_batch(family, [structs[i] for i in ids]) for ids in FC.SPLITS[split]]
    model, order, fitted = FC.fit_periodic(family, FC.CFGS[family], params, batches,
                                           FC.new_scale_file(tmp_path / f"{name}.json"), DEV)
    return model, order, fitted, batches, params


@pytest.mark.parametrize("split", list(FC.SPLITS))
@pytest.mark.parametrize("family", FC.FAMILIES)
def test_fit_with_images_matches_the_float64_host_fit(family, split, tmp_path):
    """small, triclinic, slab, cubic1 as one batch and as two: the float32 device fit against the float64 host emulation of the
    same periodic fit — equal order, 2e-3 relative.  Afterwards fit mode is off and the fitted model's eval call equals, bit for
    bit, that of a fresh model built from the written json (no cached weight form carries a factor of 1)."""
    order_ref, ref = FC.host_golden(family, split)       # (recorded; recomputed and checked by tests/test_pbc_fit_cpu.py)
    model, order, fitted, batches, params = _device_fit(family, split, tmp_path)
    assert not AutomaticFit.fitting_mode and AutomaticFit.fitting_completed()
    w = FC.worst(fitted, ref)
    print(f"periodic GemNet-{family} fit, {split} batch(es): {len(fitted)} factors, worst relative deviation from the float64 host "
          f"fit {w:.2e}")
    assert order == order_ref and w <= 2e-3
    fresh = FC.build(FC.CFGS[family], params, str(tmp_path / "dev.json"), DEV, family, factors_from_file=True)
    assert all(float(m.scale_factor) == fitted[m.autofit.name] for m in fresh.modules() if hasattr(m, "autofit"))
    for a, b in zip(model(batches[0]), fresh(batches[0])):
        assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("family", FC.FAMILIES)
def test_lattice_invariance_on_the_device(family, tmp_path):
    base, moved = FC.invariance_pair()
    FC.SPLITS["inv"] = [[0, 1, 2]]
    try:
        _, o0, f0, _, _ = _device_fit(family, "inv", tmp_path, structs=base, name="base")
        _, o1, f1, _, _ = _device_fit(family, "inv", tmp_path, structs=moved, name="moved")
    finally:
        del FC.SPLITS["inv"]
    w = FC.worst(f1, f0)
    print(f"GemNet-{family}: lattice invariance of the fitted factors on the device, worst relative difference {w:.2e}")
    assert o0 == o1 and w <= 2e-3


@pytest.mark.parametrize("family", FC.FAMILIES)
def test_aten_statistic_switch_agrees_with_the_kernel(family, tmp_path, monkeypatch):
    """GEMNET_FIT_STAT=0 (materialised gather + torch.var, float32 sums) against 1: same order, factors within 2e-3."""
    _, o1, f1, _, _ = _device_fit(family, "two", tmp_path, name="k")
    monkeypatch.setattr(scaling, "USE_FIT_STAT", False)
    _, o0, f0, _, _ = _device_fit(family, "two", tmp_path, name="a")
    w = FC.worst(f0, f1)
    print(f"GemNet-{family}: GEMNET_FIT_STAT=0 against 1, worst relative difference {w:.2e}")
    assert o0 == o1 and w <= 2e-3


# ----------------------------------------------------------------------------------------------------------------- behaviour
def _fit_mode_model(family, tmp_path, switch=True, have=None, **cfg_kw):
    cfg = dict(FC.CFGS[family], **cfg_kw)
    path = FC.new_scale_file(tmp_path / "s.json")
    if have:
        from gemnet_pytorch_amd.model.utils import update_json
        update_json(path, have)
    AutomaticFit.set2fitmode()
    model = FC.build(cfg, GO.make_params(cfg, FC.SEED, None, torch.float64), path, DEV, family)
    model.periodic_scale_fitting = switch
    return model


@pytest.mark.parametrize("family", FC.FAMILIES)
def test_refusals(family, tmp_path, monkeypatch):
    who = "periodic cells (GemNet-Q)" if family == "Q" else "periodic cells"
    batch = FC.device_batch(family, FC.structures()[:2])
    try:
        model = _fit_mode_model(family, tmp_path, switch=False)
        with pytest.raises(NotImplementedError) as e:
            model(batch)
        assert str(e.value) == f"{who}: no scale-factor fitting with a cell"               # switch off: word for word
        model.periodic_scale_fitting = True
        model.train()
        with pytest.raises(NotImplementedError, match="scale-factor fitting with a cell runs in eval mode"):
            model(batch)
        model.eval()
        with pytest.raises(NotImplementedError, match=r"fixed index arrays only.*padded batch"):
            model(dict(batch, _guard_rows=(2, 6)))
        with monkeypatch.context() as m:
            m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)            # (what a capturing stream answers)
            with pytest.raises(NotImplementedError, match="cannot run inside a stream capture"):
                model(batch)
        AutomaticFit.reset()
        two = _fit_mode_model(family, tmp_path, num_targets=2)
        with pytest.raises(NotImplementedError, match="one target only"):
            two(batch)
        if family == "Q":
            AutomaticFit.reset()
            dq = _fit_mode_model("Q", tmp_path, direct_forces=True)
            dq.periodic_direct_forces = True
            with pytest.raises(NotImplementedError, match="direct-force GemNet-Q is not served with a cell"):
                dq(batch)
    finally:
        AutomaticFit.fitting_mode = False
        AutomaticFit.reset()


def _traced(model, batch, redzone):      # noqa: F811
    """One call under a tracer that keeps every C-ABI call -> (calls, byte sizes of the guarded buffers that were allocated
    inside the forward of the quadruplet interaction — the layer that would form the gathered rows)."""
    calls, sizes = FC.Calls(), []
    qi = model.int_blocks[0].quad_interaction
    inner = qi.forward

    def forward(*args, **kw):
        before = {id(a) for a in redzone.arenas}
        out = inner(*args, **kw)
        sizes.extend(a.n for a in redzone.arenas if id(a) not in before)
        return out

    qi.forward = forward
    with redzone.untraced():
        _lib.TRACE = calls
        try:
            model(batch)
            torch.cuda.synchronize()
        finally:
            _lib.TRACE = None
            del qi.forward
    assert sizes
    return calls, sizes


@pytest.mark.parametrize("stat", [True, False])
def test_launches_of_a_fit_mode_pass_of_gemnet_q(stat, tmp_path, monkeypatch, redzone):      # noqa: F811
    """The (Q, C) gather and the statistic of `*_sum_sbf` exist only while that factor is the active one — and with the kernel
    statistic the gather does not exist at all: no gn_gather_rows_f32 over Q rows, no (Q, C) float32 allocation."""
    monkeypatch.setattr(scaling, "USE_FIT_STAT", stat)
    batch = FC.device_batch("Q", FC.structures())
    Qn, C = int(batch["id4_expand_abd"].shape[0]), Q.CFG_Q["emb_size_quad"]
    assert Qn > 1000
    names = ["QuadInteraction_1_had_rbf", "QuadInteraction_1_had_cbf", "QuadInteraction_1_sum_sbf", "TripInteraction_1_had_rbf",
             "TripInteraction_1_sum_cbf", "AtomUpdate_1_sum", "OutBlock_0_sum", "OutBlock_1_sum"]

    def q_gathers(calls):
        return [a for a in calls.of("gn_gather_rows_f32") if a[3] == Qn and a[4] == C]

    def q_buffers(sizes):
        return [n for n in sizes if n == Qn * C * 4]

    try:
        # the active factor is elsewhere (the last one): nothing is done for `_sum_sbf`
        model = _fit_mode_model("Q", tmp_path, have={k: 1.0 for k in names[:-1]})
        assert AutomaticFit.activeVar._name == names[-1]
        calls, sizes = _traced(model, batch, redzone)
        stats = calls.of("gn_col_var_f32")
        assert len(stats) == (2 if stat else 0) and all(a[5] != Qn for a in stats)
        assert not q_gathers(calls) and not q_buffers(sizes)
        AutomaticFit.reset()
        # `_sum_sbf` is the active one
        model = _fit_mode_model("Q", tmp_path, have={k: 1.0 for k in names if k != names[2]})
        assert AutomaticFit.activeVar._name == names[2]
        calls, sizes = _traced(model, batch, redzone)
        stats = calls.of("gn_col_var_f32")
        if stat:
            assert len(stats) == 2 and stats[0][5] == Qn and stats[0][1] is not None and stats[0][6] == C
            assert not q_gathers(calls) and not q_buffers(sizes)
        else:
            assert not stats and len(q_gathers(calls)) == 1 and len(q_buffers(sizes)) >= 1     # (the detector sees the gather)
    finally:
        AutomaticFit.fitting_mode = False
        AutomaticFit.reset()
