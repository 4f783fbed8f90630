"""Helpers of the tests of scale-factor fitting on periodic batches (GemNet.periodic_scale_fitting,
training.periodic.fit_scale_factors): a float64 host restatement of the statistic launcher (kernels.col_var) that never forms the
gathered rows either, the context manager that swaps it in beside the emulated launchers of the three model families, the
model / batch builders of both devices and the fit drivers (periodic, and the molecular one that serves as an oracle where a cell
holds no image inside the cutoff)."""
import contextlib
import json
import os

import numpy as np
import torch

import cpu_kernels
import pbc_common as P
import pbc_direct_train_common as DT
import pbc_q_common as Q
import pbc_q_train_common as QT
import pbc_train_common as PT
from oracle import gemnet_oracle as GO

DEV = "cuda"
KINDS = ["small", "triclinic", "slab", "cubic1"]
SPLITS = {"one": [[0, 1, 2, 3]], "two": [[0, 1], [2, 3]]}
FAMILIES = ("T", "dT", "Q")
CFGS = {"T": P.CFG, "dT": dict(P.CFG, direct_forces=True), "Q": Q.CFG_Q}
SWITCH = {"T": (), "dT": ("periodic_direct_forces",), "Q": ("periodic_quadruplets",)}
SEED = 11


# ---------------------------------------------------------------------------------------------- the statistic on the host
def col_var(x, idx32, acc, slot, w):
    """kernels.col_var in float64 WITHOUT the gathered rows: shifted sums weighted by how often the index names a row."""
    if x.dim() != 2 or not x.is_contiguous():
        raise TypeError("col_var: a contiguous (n_src, C) array expected")
    xd = x.detach().double()
    if idx32 is None:
        n, cnt, first = xd.shape[0], torch.ones(xd.shape[0], dtype=torch.float64), 0
    else:
        n, first = int(idx32.shape[0]), int(idx32[0]) if idx32.shape[0] else 0
        cnt = torch.bincount(idx32.long(), minlength=xd.shape[0]).double()
    if n < 2:
        raise ValueError(f"col_var: a variance needs at least two rows; got {n}")
    d = xd - xd[first]
    s1, s2 = (cnt[:, None] * d).sum(0), (cnt[:, None] * d * d).sum(0)
    acc[slot] += float(w) * float(((s2 - s1 * s1 / n) / (n - 1)).clamp(min=0).mean())


def col_var_reference(x, idx=None):
    """torch.var(x.double()[idx], dim=0).mean(): the materialised form, as a float."""
    xd = x.detach().double().cpu()
    rows = xd if idx is None else xd[idx.cpu().long()]
    return float(torch.var(rows, dim=0).mean())


_EMULATE = {"T": PT.emulate, "dT": DT.emulate, "Q": QT.emulate}


@contextlib.contextmanager
def emulate(family):
    """The emulated launchers of the family's periodic path + the statistic: observations go through `col_var` above (the
    kernel path of AutoScaleFit.observe, bookkeeping included) whenever the switch GEMNET_FIT_STAT is on."""
    import gemnet_pytorch_amd.kernels as K
    from gemnet_pytorch_amd.model import scaling
    saved = (K.col_var, scaling._kernel_statistic)
    with _EMULATE[family]():
        try:
            K.col_var = col_var
            scaling._kernel_statistic = lambda t: scaling.USE_FIT_STAT and scaling.periodic_statistic_active()
            yield
        finally:
            K.col_var, scaling._kernel_statistic = saved


# ------------------------------------------------------------------------------------------------------ structures, batches
def structures():
    return [P.structure(k, seed=i) for i, k in enumerate(KINDS)]


def shifted(struct, seed):
    """The structure with some atoms moved by integer lattice vectors along its periodic axes (unwrapped positions): every
    local environment is unchanged."""
    R, Z, cell, pbc = struct
    rs = np.random.RandomState(seed)
    n = rs.randint(-2, 3, size=(len(R), 3)) * np.asarray(pbc, int)[None, :]
    n[0] = 0
    assert np.abs(n).sum() > 0
    return R + n @ np.asarray(cell, np.float64), Z, cell, pbc


def invariance_pair():
    """-> (base, moved): small, triclinic, slab and the same with atoms moved by lattice vectors.  The base positions are rounded
    through float32: the slab's lattice vector b has length 3.0 = pbc_q_common.INT_CUTOFF exactly, and with 24-bit positions
    R_y + 3 k is exact in float64, so that self-image pair sits AT the cutoff (and inside the list) in both structures instead
    of on either side of it by a rounding error."""
    base = [P.f32_round(s) for s in structures()[:3]]
    return base, [shifted(s, seed=3 + i) for i, s in enumerate(base)]


def host_batch(family, structs):
    return (QT.batch if family == "Q" else PT.batch)(structs)


def device_batch(family, structs, cutoff=P.CUTOFF, int_cutoff=Q.INT_CUTOFF):
    """A periodic batch on the device from pbc.PeriodicGraphBuilder / PeriodicQuadGraphBuilder (float64 positions for the list)."""
    from gemnet_pytorch_amd.pbc import PeriodicGraphBuilder, PeriodicQuadGraphBuilder
    R, Z, N, cell, pbc = P.arrays(structs)
    if family == "Q":
        b = PeriodicQuadGraphBuilder(N, cutoff, int_cutoff, pbc=pbc, device=DEV)
    else:
        b = PeriodicGraphBuilder(N, cutoff, pbc=pbc, device=DEV)
    inputs = dict(b(torch.tensor(R, dtype=torch.float64, device=DEV), torch.tensor(cell, dtype=torch.float64, device=DEV)))
    inputs.update(R=torch.tensor(R, dtype=torch.float32, device=DEV), Z=torch.tensor(Z, device=DEV).long(),
                  N=torch.tensor(N, device=DEV), cell=torch.tensor(cell, dtype=torch.float32, device=DEV))
    return inputs


def boxed(R, extent_margin):
    """A molecule in a cubic cell of edge extent + margin, all axes periodic."""
    R = np.asarray(R, np.float64)
    edge = float((R.max(0) - R.min(0)).max()) + extent_margin
    return np.eye(3) * edge, np.array([True, True, True])


# ------------------------------------------------------------------------------------------------------------------- models
def new_scale_file(path):
    from gemnet_pytorch_amd.model.utils import write_json
    write_json(str(path), {"comment": "test"})
    return str(path)


def build(cfg, params, scale_file, device, family=None, factors_from_file=False):
    """The model of `cfg` with the oracle's weights on `device` ("cpu": float64, input check off), in eval mode, opted in.
    `factors_from_file`: the scale factors stay what the constructor read from `scale_file` (the state dict of the oracle's
    parameters carries factors of its own: 1.0)."""
    from gemnet_pytorch_amd.model.gemnet import GemNet
    model = GemNet(**cfg, scale_file=scale_file)
    state = GO.expand_to_reference_state_dict(params if device == "cpu" else {k: v.float() for k, v in params.items()})
    if factors_from_file:
        state = {k: v for k, v in state.items() if not k.endswith(".scale_factor")}
    if device == "cpu":
        model = model.double()
    missing = model.load_state_dict(state, strict=not factors_from_file)
    assert not missing.unexpected_keys and all(k.endswith(".scale_factor") for k in missing.missing_keys)
    if device == "cpu":
        model._check_inputs = lambda R: None
    else:
        model = model.to(device)
    model.eval()
    if family is not None:
        model.periodic_scale_fitting = True
        for s in SWITCH[family]:
            setattr(model, s, True)
    return model


def read_fitted(scale_file):
    with open(scale_file) as f:
        out = json.load(f)
    out.pop("comment", None)
    return out


def fit_periodic(family, cfg, params, batches, scale_file, device, num_batches=None):
    """fit_scale_factors on a fresh model -> (model, order, fitted).  Call inside `emulate(family)` for device == "cpu"."""
    from gemnet_pytorch_amd.model.scaling import AutomaticFit
    from gemnet_pytorch_amd.training.periodic import fit_scale_factors
    AutomaticFit.set2fitmode()
    try:
        model = build(cfg, params, scale_file, device, family)
        fitted = fit_scale_factors(model, batches, num_batches=num_batches or len(batches))
    finally:
        AutomaticFit.fitting_mode = False
        AutomaticFit.reset()
    assert fitted == read_fitted(scale_file)
    return model, list(fitted), fitted


def fit_molecular_host(cfg, params, batches, scale_file):
    """The molecular fit of the same parameters in float64 on the emulated launchers (eval-mode calls, the loop of
    fit_scaling.py): -> (order, fitted).  `batches`: molecular input dicts (float64 R)."""
    from gemnet_pytorch_amd.model.scaling import AutomaticFit
    order = []
    with cpu_kernels.emulate():
        AutomaticFit.set2fitmode()
        try:
            model = build(cfg, params, scale_file, "cpu")
            while not AutomaticFit.fitting_completed():
                for b in batches:
                    model(dict(b))
                order.append(AutomaticFit.activeVar._name)
                AutomaticFit.activeVar.fit()
        finally:
            AutomaticFit.fitting_mode = False
            AutomaticFit.reset()
    return order, read_fitted(scale_file)


def host_golden(family, split):
    """(order, fitted) of the float64 host emulation of the periodic fit of `family` on the batches of `split`, as recorded in
    tests/golden/pbc_fit_host.json (tests/test_pbc_fit_cpu.py recomputes every entry and holds the file to it)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pbc_fit_host.json")) as f:
        g = json.load(f)["fits"][family][split]
    return g["order"], g["fitted"]


def worst(fitted, ref):
    assert sorted(fitted) == sorted(ref)
    return max(abs(fitted[k] - v) / abs(v) for k, v in ref.items())


# ------------------------------------------------------------------------------------------------------------ launch trace
class Calls:
    """A tracer for `_lib.TRACE` that keeps (name, plain-int arguments) of every C-ABI call."""

    def __init__(self):
        self.calls = []

    def touch(self, t):
        pass

    def note(self, reads=(), writes=()):
        pass

    def proxy(self, lib):
        outer = self

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(lib, name)

                def call(*args):
                    outer.calls.append((name, args))
                    return fn(*args)
                return call
        return Proxy()

    def of(self, name):
        return [a for n, a in self.calls if n == name]
