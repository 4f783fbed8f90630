"""Molecular-dynamics entry point: the reference's `ase_calculator.Molecule` surface over the device-resident path.

The reference's MD loop (ase_calculator.py:148-170, `GNNCalculator.calculate`) does, every step,

    self.molecule.update(R=atoms.positions)        # new positions
    inputs = self.molecule.get()                   # index construction on the host (data_container.py:244-489) + H2D copies
    energy, forces = self.model.predict(inputs)    # forward + force, D2H

`Molecule` builds the neighbour lists / triplets / quadruplets in numpy and scipy on the CPU each time.  `DeviceMolecule`
has the same constructor and the same three methods the calculator uses (`update`, `get`, `to`) but `get()` hands back
only positions, atomic numbers and the molecule layout, tagged as `MoleculeInputs`; `GemNet.predict` recognises the tag
and serves the call from `runtime.DynamicForceField`: index construction on the device, padded to fixed capacities, ONE
captured hipGraph replayed per step (bit-identical to the eager run on the unpadded arrays).  The calculator class itself
is used unchanged:

    from gemnet_pytorch_amd.md import DeviceMolecule as Molecule          # the only edited line of an MD script
    calc = GNNCalculator(Molecule(R, Z, cutoff, int_cutoff, triplets_only), model=model, atoms=atoms)

A periodic `DeviceMolecule(..., cell=, pbc=)` (GemNet-T) is served the same way: `predict_periodic`, a cached
`DynamicForceField(cell=)` whose graph builds the image neighbour list itself; `predict(..., stress=True)` adds the stress.

Triplets-only and quadruplet models alike (GemNet-Q — the model of the reference's MD example — since round 5: the padding
scheme covers interaction edges, intermediate triplets and quadruplets, padded.py)."""
import numpy as np
import torch


class MoleculeInputs(dict):
    """What `DeviceMolecule.get()` returns: {"R", "Z", "N"} (no index arrays) + the cutoffs that define the graph."""

    def __init__(self, data, cutoff, int_cutoff, triplets_only, layout_key=None):
        super().__init__(data)
        self.cutoff, self.int_cutoff, self.triplets_only = float(cutoff), float(int_cutoff), bool(triplets_only)
        # (atomic numbers, molecule sizes) as a hashable HOST value — the key of the per-system force field; given by
        # DeviceMolecule (which holds both on the host), else derived from the tensors once per call (a device read-back)
        self.layout_key = layout_key


class DeviceMolecule:
    """Drop-in for the reference's `Molecule(R, Z, cutoff, int_cutoff, triplets_only)` (ase_calculator.py:23-104)."""

    def __init__(self, R, Z, cutoff, int_cutoff, triplets_only=False, cell=None, pbc=None, periodic_quadruplets=False):
        """cell (3,3) rows = lattice vectors, pbc (3,) bool (default all periodic): a periodic structure (pbc.py; GemNet-T).
        `periodic_quadruplets=True`: a periodic structure for a GemNet-Q (`triplets_only=False`) that opts in with
        `model.periodic_quadruplets` and `model.periodic_quadruplets_dynamic`; without it such a molecule raises."""
        R = np.asarray(R)
        Z = np.asarray(Z)
        assert R.shape == (len(Z), 3)
        self.cutoff, self.int_cutoff, self.triplets_only = cutoff, int_cutoff, triplets_only
        self.cell = None if cell is None else np.asarray(cell, dtype=np.float64).reshape(3, 3)
        self.pbc = np.ones(3, dtype=bool) if pbc is None else np.asarray(pbc, dtype=bool).reshape(3)
        if self.cell is not None and not triplets_only and not periodic_quadruplets:
            raise NotImplementedError("periodic cells: GemNet-T (triplets_only=True) only, not GemNet-Q")
        self.R = R
        self.Z = Z
        self.N = np.array([len(Z)], dtype=np.int32)
        self.device = "cpu"
        self._Z_dev = self._N_dev = None
        self._key = (np.asarray(Z, dtype=np.int64).tobytes(), (int(len(Z)),))

    def update(self, R):
        """New positions (ase_calculator.py:86-97)."""
        R = np.asarray(R) if not torch.is_tensor(R) else R
        assert tuple(self.R.shape) == tuple(R.shape)
        self.R = R

    def to(self, device):
        """Device of the tensors `get()` returns (ase_calculator.py:99-103)."""
        self.device = device
        self._Z_dev = self._N_dev = None

    def get(self):
        if self._Z_dev is None:   # constant over the trajectory: uploaded once
            self._Z_dev = torch.as_tensor(np.asarray(self.Z), dtype=torch.int64).to(self.device)
            self._N_dev = torch.as_tensor(self.N, dtype=torch.int64).to(self.device)
        R = self.R if torch.is_tensor(self.R) else torch.as_tensor(np.asarray(self.R, dtype=np.float32))
        data = dict(R=R.to(self.device, dtype=torch.float32), Z=self._Z_dev, N=self._N_dev)
        if self.cell is not None:
            data["cell"] = torch.as_tensor(self.cell, dtype=torch.float32).reshape(1, 3, 3).to(self.device)
            data["pbc"] = torch.as_tensor(self.pbc).reshape(1, 3)
        return MoleculeInputs(data, self.cutoff, self.int_cutoff, self.triplets_only, layout_key=self._key)


def predict_periodic(model, inputs, stress=False, to_host=False):
    """A periodic `MoleculeInputs` -> (E, F) or (E, F, S).  Served like a molecule (predict_molecule) from a cached
    `runtime.DynamicForceField(cell=, pbc=)`: the image neighbour list is built INSIDE the replayed graph for the positions and
    the cell of the call, so an MD step is one replay.  A GemNet-Q is served the same way when it opts in
    (`model.periodic_quadruplets` and `model.periodic_quadruplets_dynamic`; gn_pbc_qindex_padded), otherwise it raises.  The cache
    key is the layout, both cutoffs, the periodic axes and the
    device — the cell is data.  GEMNET_INDEX_IN_GRAPH=0: the host-sized path (device list per call, padded, one replay)."""
    R, Z, N, cell = inputs["R"], inputs["Z"], inputs["N"], inputs["cell"]
    if not R.is_cuda:
        raise RuntimeError("periodic structures run on a HIP device only (no CPU fallback); DeviceMolecule.to('cuda')")
    from .padded import periodic_quad_opted_in
    if not model.triplets_only and not periodic_quad_opted_in(model):
        raise NotImplementedError("periodic cells: GemNet-T (triplets_only=True) only, not GemNet-Q")
    if stress and getattr(model, "direct_forces", False):
        raise ValueError("a direct-force model has no stress (its forces are not the gradient of its energy)")
    pbc = np.asarray(inputs["pbc"].cpu().numpy(), dtype=bool).reshape(-1, 3)
    lk = inputs.layout_key
    if lk is None:
        lk = (Z.detach().cpu().numpy().astype(np.int64).tobytes(), tuple(int(n) for n in N.tolist()))
    key = (lk, inputs.cutoff, inputs.int_cutoff, pbc.tobytes(), R.device.index)
    cache = model.__dict__.setdefault("_md_fields", {})
    ff = cache.get(key)
    was_training = model.training
    try:
        model.eval()
        if ff is None:
            from .runtime import DynamicForceField
            ff = DynamicForceField(model, Z, N.cpu().numpy(), inputs.cutoff, inputs.int_cutoff, cell=cell, pbc=pbc)
            if len(cache) >= 8:
                cache.pop(next(iter(cache)))
            cache[key] = ff
        E, F = ff(R, cell=cell)
        out = (E, F, ff.stress()) if stress else (E, F)
        if to_host:
            host = tuple(t.detach().cpu() for t in out)      # (after this copy the replay's device-side range check is exact)
            if ff.range_tripped():
                E, F = ff.recover(R)
                out = (E, F, ff.stress()) if stress else (E, F)
                host = tuple(t.detach().cpu() for t in out)
            return host
        return out
    finally:
        model.train(was_training)


def predict_molecule(model, inputs, to_host=False):
    """`GemNet.predict` for `MoleculeInputs`: -> (E, F) on the device (inference only); `to_host`: detached host copies, the
    replayed step's range flag checked after the copy (what `GemNet.predict` returns)."""
    R, Z, N = inputs["R"], inputs["Z"], inputs["N"]
    if inputs.triplets_only != model.triplets_only:
        raise ValueError("DeviceMolecule(triplets_only=...) does not match the model")
    if inputs.get("cell") is not None:
        return predict_periodic(model, inputs, to_host=to_host)
    if not R.is_cuda:
        # host tensors: the host index builder (include/gemnet_index.h) + the ordinary forward (raises without a device,
        # like every other entry point: there is no CPU compute path)
        from .training.data_container import DataContainer
        dc = DataContainer.from_arrays(dict(R=R.numpy(), Z=Z.numpy(), N=N.numpy(), E=np.zeros((1, 1), np.float32),
                                            F=np.zeros((R.shape[0], 3), np.float32)),
                                       inputs.cutoff, inputs.int_cutoff, triplets_only=model.triplets_only)
        b = dc[[0]]
        E, F = model({k: v for k, v in b.items() if k not in ("E", "F")})
        return (E.detach().cpu(), F.detach().cpu()) if to_host else (E, F)
    lk = inputs.layout_key
    if lk is None:
        lk = (Z.detach().cpu().numpy().astype(np.int64).tobytes(), tuple(int(n) for n in N.tolist()))
    key = (lk, inputs.cutoff, inputs.int_cutoff, R.device.index)
    cache = model.__dict__.setdefault("_md_fields", {})
    ff = cache.get(key)
    was_training = model.training
    if ff is None:
        model.eval()
        # (the caller's parameters are left as they are — `requires_grad` included: an eval-mode forward with forces by autograd
        #  treats the weights as constants anyway (ops.constant_weights), and a force field built in the middle of a training
        #  script must not freeze the model; the reference's predict() does not touch it either, gemnet.py:780-784)
        from .runtime import DynamicForceField
        ff = DynamicForceField(model, Z, N.cpu().numpy(), inputs.cutoff, inputs.int_cutoff)
        if len(cache) >= 8:
            cache.pop(next(iter(cache)))
        cache[key] = ff
    try:
        model.eval()
        E, F = ff(R)
        if to_host:
            # the MD loop reads its results on the host (ase_calculator.py:166-170): after this copy the replay has completed
            # and its device-side range check (runtime.RangeFlag) is exact — an overflow of the fp16-plane arithmetic in a
            # REPLAYED step warns, moves the model to the bf16 planes, captures anew and repeats the step
            Eh, Fh = E.detach().cpu(), F.detach().cpu()
            if hasattr(ff, "range_tripped") and ff.range_tripped():
                E, F = ff.recover(R)
                Eh, Fh = E.detach().cpu(), F.detach().cpu()
            return Eh, Fh
        return E, F
    finally:
        model.train(was_training)
