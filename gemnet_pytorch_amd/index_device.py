"""Index construction on the device: `build_indices_device` returns the same dict of index
tensors as `DataContainer.__getitem__` (gemnet/training/data_container.py:156-408; canonical within-segment
order, see include/gemnet_hip.h), built by csrc/index_gpu.hip from positions that already live in HBM — the
MD loop of ase_calculator.py:155-158 rebuilds the graph every step.

    idx = build_indices_device(R, N, cutoff, int_cutoff, triplets_only)      # R (A,3) cuda float32|float64
    inputs = dict(Z=Z, R=R.float(), N=N_dev, **idx)                            # -> GemNet.forward

`DeviceGraphBuilder` keeps the molecule layout (offsets, workspace) for repeated calls on the same system.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, require_device, stream

KEYS_T = ["batch_seg", "id_undir", "id_swap", "id_c", "id_a", "id3_expand_ba", "id3_reduce_ca", "Kidx3"]
KEYS_Q = ["id4_int_b", "id4_int_a", "id4_reduce_ca", "id4_expand_db", "id4_reduce_cab", "id4_expand_abd", "Kidx4",
          "id4_reduce_intm_ca", "id4_expand_intm_db", "id4_reduce_intm_ab", "id4_expand_intm_ab"]


class DeviceGraphBuilder:
    def __init__(self, N, cutoff, int_cutoff, triplets_only=False, device="cuda"):
        N = np.asarray(N, dtype=np.int64).reshape(-1)
        self.B, self.A = int(len(N)), int(N.sum())
        self.nmax = int(N.max()) if len(N) else 0
        self.sum_n2 = int((N * N).sum())
        if self.sum_n2 >= 2 ** 31:
            raise ValueError("sum of squared molecule sizes exceeds int32")
        self.cutoff, self.int_cutoff, self.triplets_only = float(cutoff), float(int_cutoff), bool(triplets_only)
        self.device = torch.device(device)
        self.mol_off = torch.tensor(np.concatenate([[0], np.cumsum(N)]), dtype=torch.int32, device=self.device)
        self.sq_off = torch.tensor(np.concatenate([[0], np.cumsum(N * N)]), dtype=torch.int32, device=self.device)
        self.lib = _lib.load()
        nbytes = int(self.lib.gn_index_gpu_ws_bytes(self.A, self.sum_n2, int(self.triplets_only)))
        self.ws = torch.empty(max(nbytes, 64), dtype=torch.uint8, device=self.device)
        self.cap = max(self.sum_n2 - self.A, 0)  # upper bound of E and of Eint

    def __call__(self, R, dtype=torch.int64):
        """R (A,3) device float32 | float64 -> {key: tensor(dtype)}; dtype int64 (reference) or int32 (no copy)."""
        require_device(R)
        if R.dtype not in (torch.float32, torch.float64):
            raise TypeError("positions must be float32 or float64")
        R = R.contiguous()
        assert R.shape == (self.A, 3)
        dev, i32 = R.device, torch.int32
        quad = not self.triplets_only
        new = lambda n: torch.empty(int(n), dtype=i32, device=dev)
        batch_seg = new(self.A)
        e_arr = {k: new(self.cap) for k in ("id_a", "id_c", "id_undir", "id_swap")}
        i_arr = {k: new(self.cap if quad else 0) for k in ("id4_int_a", "id4_int_b")}
        sizes = (ctypes.c_int64 * 6)()
        check(_lib.load().gn_index_gpu_stage1(
            ptr(R), int(R.dtype == torch.float64), ptr(self.mol_off), ptr(self.sq_off), self.B, self.A, self.nmax,
            self.sum_n2, self.cutoff, self.int_cutoff, int(self.triplets_only), ptr(self.ws), ptr(batch_seg),
            ptr(e_arr["id_a"]), ptr(e_arr["id_c"]), ptr(e_arr["id_undir"]), ptr(e_arr["id_swap"]),
            ptr(i_arr["id4_int_a"]), ptr(i_arr["id4_int_b"]), sizes, stream()), "gn_index_gpu_stage1")
        E, T, Eint, Ica, Idb, Q = (int(v) for v in sizes)
        out = {"batch_seg": batch_seg}
        for k, v in e_arr.items():
            out[k] = v[:E]
        t_arr = {k: new(T) for k in ("id3_reduce_ca", "id3_expand_ba", "Kidx3")}
        q_arr = {}
        if quad:
            for k, v in i_arr.items():
                out[k] = v[:Eint]
            q_arr = {k: new(Q) for k in ("id4_reduce_ca", "id4_expand_db", "id4_reduce_cab", "id4_expand_abd", "Kidx4")}
            q_arr.update(id4_reduce_intm_ca=new(Ica), id4_reduce_intm_ab=new(Ica),
                         id4_expand_intm_db=new(Idb), id4_expand_intm_ab=new(Idb))
        g = lambda d, k: ptr(d[k]) if k in d else None
        check(_lib.load().gn_index_gpu_stage2(
            ptr(self.mol_off), ptr(self.sq_off), self.B, self.A, self.sum_n2, int(self.triplets_only), ptr(self.ws),
            ptr(out["id_a"]), ptr(out["id_c"]), g(out, "id4_int_a"), g(out, "id4_int_b"), E, Eint,
            ptr(t_arr["id3_reduce_ca"]), ptr(t_arr["id3_expand_ba"]), ptr(t_arr["Kidx3"]),
            g(q_arr, "id4_reduce_ca"), g(q_arr, "id4_expand_db"), g(q_arr, "id4_reduce_cab"), g(q_arr, "id4_expand_abd"),
            g(q_arr, "Kidx4"), g(q_arr, "id4_reduce_intm_ca"), g(q_arr, "id4_expand_intm_db"),
            g(q_arr, "id4_reduce_intm_ab"), g(q_arr, "id4_expand_intm_ab"), stream()), "gn_index_gpu_stage2")
        out.update(t_arr)
        out.update(q_arr)
        keys = KEYS_T + ([] if self.triplets_only else KEYS_Q)
        return {k: (out[k] if dtype == torch.int32 else out[k].to(dtype)) for k in keys}


class DeviceCapacityGraphBuilder(DeviceGraphBuilder):
    """`DeviceGraphBuilder` whose layout can change: `n_mol` molecules per batch inside an atom capacity `a_cap`, none larger
    than `n_max` atoms, their sizes N set per batch — the molecular sibling of pbc.PeriodicCapacityGraphBuilder.  It owns
    `mol_off` (n_mol + 2), `sq_off` (n_mol + 1), `atom_mol` (a_cap) and the workspace as device buffers of the capacity shapes
    (the filler atoms between the batch and a_cap form "molecule" n_mol: padded.capacity_layout), and the sizes as the
    in-graph layout reads them: `N32` (n_mol) int32, `n_atoms` (1) int32.

        builder = DeviceCapacityGraphBuilder(n_mol, a_cap, n_max, cutoff, device=dev)
        builder.set_layout(N)                          # host or device array
        idx = builder(R)                               # = DeviceGraphBuilder(N, cutoff, cutoff, triplets_only=True)(R)

    Attached to a molecular `padded.PaddedGraphRunner` with `a_cap` the layout (gn_index_gpu_layout) and the lists
    (gn_index_gpu_padded_tv) are built inside the replay from these buffers.  Triplets-only models (GemNet-T); GemNet-Q takes
    `DeviceCapacityQuadGraphBuilder` below."""

    def __init__(self, n_mol, a_cap, n_max, cutoff, triplets_only=True, device="cuda"):
        if not triplets_only:
            raise NotImplementedError("DeviceCapacityGraphBuilder: triplets-only models (GemNet-T) only, not GemNet-Q "
                                      "(quadruplet lists with an atom capacity are not built inside the graph)")
        self._init_capacity(n_mol, a_cap, n_max, cutoff, cutoff, True, device)

    def _init_capacity(self, n_mol, a_cap, n_max, cutoff, int_cutoff, triplets_only, device):
        self.B, self.a_cap, self.n_max = int(n_mol), int(a_cap), int(n_max)
        if not 0 < self.B <= self.a_cap:
            raise ValueError(f"need 0 < n_mol <= a_cap; got n_mol = {self.B}, a_cap = {self.a_cap}")
        if not 0 < self.n_max <= self.a_cap:
            raise ValueError(f"need 0 < n_max <= a_cap; got n_max = {self.n_max}, a_cap = {self.a_cap}")
        if self.a_cap * self.n_max >= 2 ** 31:
            raise ValueError(f"a_cap * n_max = {self.a_cap * self.n_max} exceeds int32 (the adjacency blocks of the batch)")
        self.A = None                       # atoms of the current layout (known on the host once a batch came by)
        self.cutoff, self.int_cutoff, self.triplets_only = float(cutoff), float(int_cutoff), bool(triplets_only)
        self.device = torch.device(device)
        dev = self.device
        self.mol_off = torch.zeros(self.B + 2, dtype=torch.int32, device=dev)
        self.sq_off = torch.zeros(self.B + 1, dtype=torch.int32, device=dev)
        self.atom_mol = torch.full((self.a_cap,), self.B, dtype=torch.int32, device=dev)
        self.N32 = torch.ones(self.B, dtype=torch.int32, device=dev)
        self.n_atoms = torch.zeros(1, dtype=torch.int32, device=dev)
        self._N_host = None                 # the sizes as the host knows them (None: handed in on the device)
        self._arrays = False                # do mol_off / sq_off / atom_mol hold the layout of N32?
        self._ws = None

    @property
    def ws(self):
        """The workspace of the capacity shapes (kernels.index_cap_ws_bytes), allocated on first use."""
        if self._ws is None:
            from . import kernels as K
            nbytes = K.index_cap_ws_bytes(self.a_cap, self.n_max, quad=not self.triplets_only)
            self._ws = torch.empty(max(nbytes, 64), dtype=torch.uint8, device=self.device)
        return self._ws

    def check_sizes(self, N, n_atoms=None):
        """ValueError unless the host sizes N fit this builder: n_mol of them, each in [1, n_max], a_cap atoms at the most (and
        `n_atoms` of them when given) — what gn_index_gpu_layout checks on the device (error bit 128)."""
        N = np.asarray(N, dtype=np.int64).reshape(-1)
        if len(N) != self.B:
            raise ValueError(f"N must hold {self.B} molecule sizes; got {len(N)}")
        if N.min() < 1 or N.max() > self.n_max or N.sum() > self.a_cap or (n_atoms is not None and N.sum() != int(n_atoms)):
            raise ValueError(f"molecule sizes (min {int(N.min())}, max {int(N.max())}, sum {int(N.sum())}) do not fit n_max = "
                             f"{self.n_max} / a_cap = {self.a_cap}" + ("" if n_atoms is None else f" / n_atoms = {int(n_atoms)}"))
        return N

    def set_layout(self, N=None, n_atoms=None, arrays=True):
        """Sizes N (n_mol,) of the next batch, a host or a device array (None: as they are).  No host sync.  `n_atoms`: the atom
        count the in-graph layout checks sum(N) against (default: sum of a host N); `arrays=False` leaves `mol_off` / `sq_off` /
        `atom_mol` to the in-graph layout kernel, which refuses sizes that do not fit (bit 128).  With `arrays=True` host sizes
        that do not fit raise `ValueError`; device sizes that do not fit leave the three arrays as they were."""
        if N is not None:
            on_dev = torch.is_tensor(N) and N.device.type != "cpu"
            Nt = (N if torch.is_tensor(N) else torch.as_tensor(np.asarray(N, dtype=np.int64))).reshape(-1)
            if int(Nt.shape[0]) != self.B:
                raise ValueError(f"N must hold {self.B} molecule sizes; got {int(Nt.shape[0])}")
            host = None if on_dev else Nt.detach().numpy().astype(np.int64)
            if host is not None:
                if arrays:
                    self.check_sizes(host, n_atoms)
                if n_atoms is None:
                    n_atoms = int(host.sum())
            self._N_host = host
            self.N32.copy_(Nt)
            self.A = None if n_atoms is None else int(n_atoms)
            self._arrays = False
        if n_atoms is not None:
            self.A = int(n_atoms)
            self.n_atoms.fill_(int(n_atoms))
        if arrays and not self._arrays:
            self._write_arrays(check_atoms=n_atoms is not None)
        return self

    def _write_arrays(self, check_atoms=True):
        """mol_off / sq_off / atom_mol of N32 (padded.capacity_layout and the prefix sums of N^2) in PyTorch, without a host
        sync: sizes that gn_index_gpu_layout would refuse leave the arrays as they were."""
        from .padded import capacity_layout
        N = self.N32.to(torch.int64)
        lay = capacity_layout(N, self.B, self.a_cap, self.a_cap)
        sq = torch.cat([torch.zeros(1, dtype=torch.int64, device=N.device), torch.cumsum(N * N, 0)])
        ok = ((N >= 1) & (N <= self.n_max)).all() & (N.sum() <= self.a_cap)
        if check_atoms:
            ok = ok & (N.sum() == self.n_atoms[0])
        self.mol_off.copy_(torch.where(ok, lay["mol_off"], self.mol_off))
        self.sq_off.copy_(torch.where(ok, sq.clamp(max=2 ** 31 - 1).to(torch.int32), self.sq_off))
        self.atom_mol.copy_(torch.where(ok, lay["atom_mol"], self.atom_mol))
        self._arrays = True

    def __call__(self, R, dtype=torch.int64):
        """The host-sized build for the current layout: the kernels of `DeviceGraphBuilder` on the capacity buffers (their first
        n_mol + 1 entries are that builder's arrays).  Reads the sizes back when they were handed in on the device."""
        N = self.check_sizes(self._N_host if self._N_host is not None else self.N32.cpu().numpy())
        A = int(R.shape[0])
        if A != int(N.sum()) or (self.A is not None and A != self.A):
            raise ValueError(f"positions of {A} atoms for a layout of {int(N.sum())} (a_cap = {self.a_cap}): set_layout(N) first")
        if not self._arrays:
            self._write_arrays(check_atoms=False)
        self.A, self.nmax, self.sum_n2 = A, int(N.max()), int((N * N).sum())
        self.cap = max(self.sum_n2 - self.A, 0)
        self.ws                             # (allocated)
        return super().__call__(R, dtype=dtype)


class DeviceCapacityQuadGraphBuilder(DeviceCapacityGraphBuilder):
    """`DeviceCapacityGraphBuilder` for quadruplet models (GemNet-Q): the same layout buffers, its own interaction cutoff and the
    workspace of the quadruplet capacity shapes (kernels.index_cap_ws_bytes(a_cap, n_max, quad=True)).  `n_max >= 2`: a batch
    of single atoms has no pair.

        builder = DeviceCapacityQuadGraphBuilder(n_mol, a_cap, n_max, cutoff, int_cutoff, device=dev)
        builder.set_layout(N)
        idx = builder(R)                               # = DeviceGraphBuilder(N, cutoff, int_cutoff, triplets_only=False)(R)

    Attached to a molecular `padded.PaddedGraphRunner` with `a_cap` and `quad_caps` the layout (gn_index_gpu_layout) and all
    sixteen lists (gn_index_gpu_padded_qv) are built inside the replay."""

    def __init__(self, n_mol, a_cap, n_max, cutoff, int_cutoff, device="cuda"):
        if int(n_max) < 2:
            raise ValueError(f"need n_max >= 2 (a batch of single atoms has no pair); got n_max = {int(n_max)}")
        self._init_capacity(n_mol, a_cap, n_max, cutoff, int_cutoff, False, device)


def build_indices_device(R, N, cutoff, int_cutoff, triplets_only=False, dtype=torch.int64):
    return DeviceGraphBuilder(N, cutoff, int_cutoff, triplets_only, device=R.device)(R, dtype=dtype)


def ensure_indices(inputs, cutoff, int_cutoff, triplets_only):
    """`inputs` as `GemNet.forward` takes them; when the index arrays are missing (a `DataContainer(indices="device")` batch:
    Z, R, N only) they are built here from the device-resident positions — the same arrays, in the same canonical order, as the
    host builder's (tests/test_gpu_index.py).  One small read-back (the molecule sizes) + the builder's own size read-backs."""
    if "id_c" in inputs:
        return inputs
    R = inputs["R"]
    require_device(R)      # (no CPU fallback: on the host the arrays come from training.data_container.build_indices)
    N_host = inputs["N"].detach().cpu().numpy()
    idx = build_indices_device(R.detach(), N_host, cutoff, int_cutoff, triplets_only, dtype=torch.int32)
    return dict(inputs, **idx)
