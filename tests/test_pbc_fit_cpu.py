"""CPU, float64: scale-factor fitting on periodic batches (GemNet.periodic_scale_fitting, GemNet._forward_periodic_fit,
training.periodic.fit_scale_factors) on the emulated launchers — the statistic read through the expand index against the
materialised gather, the switch GEMNET_FIT_STAT, invariance of the fitted factors under moves by lattice vectors, the binding of
gn_col_var_f32, and what raises with the opt-in switch off and on."""
import os
import re

import numpy as np
import pytest
import torch

import pbc_common as P
import pbc_fit_common as FC
from conftest import ROOT, SCALE_FILE
from gemnet_pytorch_amd import _lib, hbcheck
from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd.model import scaling
from gemnet_pytorch_amd.model.scaling import AutomaticFit
from oracle import gemnet_oracle as GO


def _params(family):
    return GO.make_params(FC.CFGS[family], FC.SEED, None, torch.float64)


# -------------------------------------------------------------------------------------------------------------- statistic
@pytest.mark.parametrize("C", K.COL_VAR_WIDTHS)
def test_host_restatement_equals_var_of_the_gathered_rows(C):
    rs = np.random.RandomState(C)
    x = torch.tensor(rs.standard_normal((37, C)) * 3.0 + 50.0)
    for n in (2, 3, 65, 400):
        idx = torch.tensor(rs.randint(0, 30, n), dtype=torch.int32)           # unsorted, repeats, rows 30.. never named
        for ix in (idx, None):
            acc = torch.zeros(2, dtype=torch.float64)
            FC.col_var(x, ix, acc, 1, 2.5)
            ref = 2.5 * FC.col_var_reference(x, ix)
            assert float(acc[0]) == 0.0 and abs(float(acc[1]) - ref) <= 1e-12 * abs(ref)
    acc = torch.zeros(1, dtype=torch.float64)
    FC.col_var(x[:1].contiguous(), torch.zeros(9, dtype=torch.int32), acc, 0, 1.0)
    assert float(acc[0]) == 0.0
    with pytest.raises(ValueError, match="two rows"):
        FC.col_var(x, torch.zeros(1, dtype=torch.int32), acc, 0, 1.0)


def test_header_declares_and_lib_binds_the_statistic():
    with open(os.path.join(ROOT, "include", "gemnet_hip.h")) as f:
        text = f.read()
    assert all(str(c) in re.search(r"C is one of ([\d, ]+)", text).group(1) for c in K.COL_VAR_WIDTHS)
    assert len(_lib.SIGNATURES["gn_col_var_f32"]) == 10 and _lib.GN_COL_VAR_MAX_BLOCKS == 2048
    funcs, _ = hbcheck.parse_header()
    modes = dict(funcs["gn_col_var_f32"])
    assert [modes[n] for n in ("x", "idx", "ws", "acc")] == ["r", "r", "w", "w"] and modes["stream"] == "stream"
    with pytest.raises(RuntimeError, match="HIP device"):
        K.col_var(torch.zeros(4, 8), None, torch.zeros(1, dtype=torch.float64), 0, 1.0)


def test_switch_defaults(monkeypatch):
    assert scaling.USE_FIT_STAT is True and not scaling.periodic_statistic_active()
    from gemnet_pytorch_amd.model.gemnet import GemNet
    assert GemNet(**P.CFG, scale_file=SCALE_FILE).periodic_scale_fitting is False


# -------------------------------------------------------------------------------------------------------------------- fit
_FITS = {}


def _fit(family, split, tmp_path, stat=True, structs=None, key=None):
    """The float64 host fit of `family` on the batches of `split` (computed once per key, shared, never modified)."""
    key = key or (family, split, stat)
    if key not in _FITS:
        structs = structs or FC.structures()
        old = scaling.USE_FIT_STAT
        scaling.USE_FIT_STAT = stat
        try:
            with FC.emulate(family):
                batches = [FC.host_batch(family, [structs[i] for i in ids]) for ids in FC.SPLITS[split]]
                _, order, fitted = FC.fit_periodic(family, FC.CFGS[family], _params(family), batches,
                                                   FC.new_scale_file(tmp_path / f"{'_'.join(map(str, key))}.json"), "cpu")
        finally:
            scaling.USE_FIT_STAT = old
        _FITS[key] = (order, fitted)
    return _FITS[key]


@pytest.mark.parametrize("split", list(FC.SPLITS))
@pytest.mark.parametrize("family", FC.FAMILIES)
def test_index_statistic_equals_materialised_gather(family, split, tmp_path):
    """GEMNET_FIT_STAT=1 (rows read through the expand index, float64 device-style accumulator) against =0 (ops.gather_rows +
    torch.var): same order, every factor to 1e-12 (both float64 here).  The fit leaves fit mode off."""
    order1, fit1 = _fit(family, split, tmp_path, True)
    order0, fit0 = _fit(family, split, tmp_path, False)
    assert not AutomaticFit.fitting_mode and AutomaticFit.fitting_completed()
    n = {"T": 5, "dT": 7, "Q": 8}[family]          # 1 block: 2 + 1 atom update, 2 outputs (+ 2 direct), (+ 3 quadruplet)
    assert order1 == order0 and len(order1) == n, order1
    assert any(k.endswith("_sum_cbf") for k in order1) and (family != "Q" or any(k.endswith("_sum_sbf") for k in order1))
    w = FC.worst(fit1, fit0)
    print(f"{family}/{split}: worst relative difference index statistic vs materialised gather {w:.2e}")
    assert w <= 1e-12
    assert all(np.isfinite(v) and v > 0 for v in fit1.values())
    # the recorded copy that tests/test_gpu_pbc_fit.py compares the device fit with (factors are float32-rounded: a last-bit
    # difference of the float64 sums between two hosts can move one by 2^-24 at the most)
    order_g, fit_g = FC.host_golden(family, split)
    assert order_g == order1 and FC.worst(fit_g, fit1) <= 2.0 ** -23


@pytest.mark.parametrize("family", FC.FAMILIES)
def test_lattice_invariance(family, tmp_path):
    """small, triclinic and slab with atoms moved by integer lattice vectors: every local environment is unchanged (the rows of
    every observed array are the same rows, permuted), so every factor agrees to 1e-9."""
    base, moved = FC.invariance_pair()
    assert any(np.abs(m[0] - b[0]).max() > 1.0 for m, b in zip(moved, base))
    b0, b1 = FC.host_batch(family, base), FC.host_batch(family, moved)
    assert all(b0[k].shape == b1[k].shape for k in b0)                         # the same lists up to the order of their rows
    FC.SPLITS["inv"] = [[0, 1, 2]]
    try:
        o0, f0 = _fit(family, "inv", tmp_path, structs=base, key=(family, "inv", "base"))
        o1, f1 = _fit(family, "inv", tmp_path, structs=moved, key=(family, "inv", "moved"))
    finally:
        del FC.SPLITS["inv"]
    w = FC.worst(f1, f0)
    print(f"{family}: lattice invariance of the fitted factors (float64 host), worst relative difference {w:.2e}")
    assert o0 == o1 and w <= 1e-9


# -------------------------------------------------------------------------------------------------------------- behaviour
def _fit_mode_model(family, tmp_path, switch=True, **cfg_kw):
    cfg = dict(FC.CFGS[family], **cfg_kw)
    AutomaticFit.set2fitmode()
    model = FC.build(cfg, GO.make_params(cfg, FC.SEED, None, torch.float64), FC.new_scale_file(tmp_path / "s.json"), "cpu",
                     family)
    model.periodic_scale_fitting = switch
    return model


@pytest.mark.parametrize("family", FC.FAMILIES)
def test_switch_off_keeps_the_refusal_word_for_word(family, tmp_path):
    who = "periodic cells (GemNet-Q)" if family == "Q" else "periodic cells"
    try:
        with FC.emulate(family):
            model = _fit_mode_model(family, tmp_path, switch=False)
            with pytest.raises(NotImplementedError) as e:
                model(FC.host_batch(family, FC.structures()[:2]))
            assert str(e.value) == f"{who}: no scale-factor fitting with a cell"
    finally:
        AutomaticFit.fitting_mode = False
        AutomaticFit.reset()


def test_switch_on_refusals_name_their_reason(tmp_path):
    structs = FC.structures()[:2]
    try:
        with FC.emulate("T"):
            model = _fit_mode_model("T", tmp_path)
            batch = FC.host_batch("T", structs)
            model.train()
            with pytest.raises(NotImplementedError, match=r"scale-factor fitting with a cell runs in eval mode"):
                model(batch)
            model.eval()
            with pytest.raises(NotImplementedError, match=r"fixed index arrays only.*padded batch"):
                model(dict(batch, _guard_rows=(2, 6)))
            E, F, S = model(batch, stress=True)             # ... and the plain eval call is served: (E, F, S)
            assert E.shape == (2, 1) and F.shape == (6, 3) and S.shape == (2, 3, 3)
        AutomaticFit.fitting_mode = False
        AutomaticFit.reset()
        with FC.emulate("T"):
            two = _fit_mode_model("T", tmp_path, num_targets=2)
            with pytest.raises(NotImplementedError, match="one target only"):
                two(FC.host_batch("T", structs))
        AutomaticFit.fitting_mode = False
        AutomaticFit.reset()
        with FC.emulate("Q"):
            dq = _fit_mode_model("Q", tmp_path, direct_forces=True)
            dq.periodic_direct_forces = True
            with pytest.raises(NotImplementedError, match="direct-force GemNet-Q is not served with a cell"):
                dq(FC.host_batch("Q", structs))
        AutomaticFit.fitting_mode = False
        AutomaticFit.reset()
        with FC.emulate("dT"):
            dt = _fit_mode_model("dT", tmp_path)
            E, F = dt(FC.host_batch("dT", structs))           # a direct-force model: (E, F (A,1,3)) as in eval mode
            assert E.shape == (2, 1) and F.shape == (6, 1, 3)
            dt.periodic_direct_forces = False
            with pytest.raises(NotImplementedError, match="not direct_forces"):
                dt(FC.host_batch("dT", structs))
    finally:
        AutomaticFit.fitting_mode = False
        AutomaticFit.reset()


def test_driver_refuses_a_model_that_is_not_in_fit_mode_or_not_opted_in(tmp_path):
    from gemnet_pytorch_amd.training.periodic import fit_scale_factors
    cfg = FC.CFGS["T"]
    model = FC.build(cfg, _params("T"), SCALE_FILE, "cpu")
    with pytest.raises(RuntimeError, match="set2fitmode"):
        fit_scale_factors(model, [{}])
    try:
        AutomaticFit.set2fitmode()
        with pytest.raises(RuntimeError, match="periodic_scale_fitting"):
            fit_scale_factors(model, [{}])
    finally:
        AutomaticFit.fitting_mode = False
        AutomaticFit.reset()


def test_fit_mode_outputs_equal_the_eval_outputs_with_the_same_factors(tmp_path):
    """The fit-mode pass returns (E, F, S) of the batch: with every factor already in the scale file (nothing enrols) it agrees
    with the periodic training path's outputs to 1e-9."""
    structs = FC.structures()
    with FC.emulate("T"):
        batch = FC.host_batch("T", structs)
        params = GO.make_params(P.CFG, 3, GO.load_scale_factors(SCALE_FILE))
        model = FC.build(P.CFG, params, SCALE_FILE, "cpu", "T")
        # (the reference on these launchers: the training path's composite closure, whose outputs the tests of
        #  test_pbc_train_cpu.py hold to the oracle)
        model.force_graph, model.periodic_training = True, True
        ref = [t.detach() for t in model(batch, stress=True)]
        model.force_graph = None
        try:
            AutomaticFit.fitting_mode = True
            out = model(batch, stress=True)
        finally:
            AutomaticFit.fitting_mode = False
            AutomaticFit.reset()
    for a, b in zip(out, ref):
        assert float((a - b).abs().max()) <= 1e-9 * max(1.0, float(b.abs().max()))
