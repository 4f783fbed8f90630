"""Periodic cells for GemNet-T (triplets_only=True, forces by autograd): the image neighbour list, the shifted edge geometry
and the stress (csrc/pbc.hip; conventions in include/gemnet_hip.h).  The Functions of the first-order (eval) path are
once-differentiable; training (GemNet.periodic_training) differentiates the energy through ops_train._DistVec2 / _AngleVec2
instead and takes forces and stress from `force_stress` below (csrc/pbc_train.hip).

    builder = PeriodicGraphBuilder(N, cutoff, pbc=[[True, True, True]])          # N: atoms per structure (host)
    idx = builder(R, cell)                                                       # R (A,3), cell (B,3,3) on the device
    E, F, S = model(dict(Z=Z, R=R, N=N, cell=cell, **idx), stress=True)

Input keys of a periodic batch: `cell` (B,3,3), rows = lattice vectors; `cell_offsets` (E,3) integer: edge e = (c -> a) has
V_e = R[a] - (R[c] + cell_offsets[e] @ cell[b(e)]).  The stress is dE/d(strain) / |det cell| (ASE's sign convention, eV/A^3).

A direct-force model (`GemNet(direct_forces=True)` with `model.periodic_direct_forces = True`) runs the same geometry without
autograd and ends in `direct_forces` below (csrc/direct_force.hip): E, F (A,1,3), no stress.  In training mode (with
`model.periodic_training = True` as well) the same pass keeps its graph to the parameters and ends in `direct_forces_train`,
whose backward is the adjoint kernel of the head: one first-order `loss.backward()` (training.periodic.PeriodicTrainStep).

The builder reads two sizes back per call.  For MD — a new list every step — the same list is built without a read-back inside a
captured graph (csrc/pbc_index.hip, kernels.pbc_index_padded_t): padded.PaddedGraphRunner(cell=...).attach_builder(builder),
runtime.DynamicForceField(cell=...), md.predict_periodic.  The same holds for PeriodicQuadGraphBuilder (four read-backs per call)
and a GemNet-Q that opts in with `model.periodic_quadruplets_dynamic`: csrc/pbc_index_qp.hip, kernels.pbc_index_padded_q.
Batches whose structure SIZES change (a dataset) use `PeriodicCapacityGraphBuilder(n_mol, a_cap, cutoff)`: `set_layout(N, pbc)` per
batch, the same dict from `builder(R, cell)`, and — attached to a PaddedGraphRunner(a_cap=, cell=) of a model that sets
`periodic_atom_capacity` — layout and list inside the replay (kernels.pbc_layout, kernels.pbc_index_padded_tv).

Training GemNet-Q with a cell (`model.periodic_quadruplets_training`, set by training.periodic.PeriodicTrainStep) differentiates
the energy through ops_train._DistVec2 / _AngleVec2 / _AngleVec2Q / _QuadAnglesVec2 on the two leaves V and Vint
(csrc/pbc_quad_train.hip) and takes forces and stress from `force_stress_q` below.
"""
import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check, ptr, require_device, stream
from .graph import RowIndex

KEYS = ["batch_seg", "id_undir", "id_swap", "id_c", "id_a", "id3_expand_ba", "id3_reduce_ca", "Kidx3", "cell_offsets"]
# PeriodicQuadGraphBuilder adds the reference's quadruplet keys and the images of the interaction edges
KEYS_Q = ["id4_int_b", "id4_int_a", "id4_reduce_ca", "id4_expand_db", "id4_reduce_cab", "id4_expand_abd", "Kidx4",
          "id4_reduce_intm_ca", "id4_expand_intm_db", "id4_reduce_intm_ab", "id4_expand_intm_ab", "int_cell_offsets"]
MAX_IMAGES = 64      # images per axis and side the builder accepts (cutoff / perpendicular height)


def image_extent(cell, pbc, cutoff):
    """(B,3) number of images per side that a WRAPPED atom needs: ceil(cutoff / h_k) on periodic axes, 0 elsewhere."""
    cell = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    pbc = np.asarray(pbc, dtype=bool).reshape(-1, 3)
    vol = np.abs(np.linalg.det(cell))
    out = np.zeros(pbc.shape, dtype=np.int64)
    for k in range(3):
        cr = np.cross(cell[:, (k + 1) % 3], cell[:, (k + 2) % 3])
        h = vol / np.linalg.norm(cr, axis=1)
        out[:, k] = np.where(pbc[:, k], np.ceil(cutoff / h), 0)
    return out


class PeriodicGraphBuilder:
    """Device neighbour list of periodic structures: the reference's index dict (GemNet-T keys) + `cell_offsets`."""

    def __init__(self, N, cutoff, int_cutoff=None, triplets_only=True, pbc=None, device="cuda"):
        if not triplets_only:
            raise NotImplementedError("periodic cells: this class builds the GemNet-T (triplets_only=True) arrays only; the "
                                      "GemNet-Q index arrays of a periodic batch come from PeriodicQuadGraphBuilder")
        N = np.asarray(N, dtype=np.int64).reshape(-1)
        self.B, self.A = int(len(N)), int(N.sum())
        self.cutoff = float(cutoff)
        self.device = torch.device(device)
        self.pbc_host = np.ones((self.B, 3), dtype=bool) if pbc is None else np.broadcast_to(
            np.asarray(pbc, dtype=bool).reshape(-1, 3), (self.B, 3)).copy()
        self.pbc = torch.tensor(self.pbc_host.astype(np.uint8), device=self.device)
        self.mol_off = torch.tensor(np.concatenate([[0], np.cumsum(N)]), dtype=torch.int32, device=self.device)
        self.atom_mol = torch.tensor(np.repeat(np.arange(self.B), N), dtype=torch.int32, device=self.device)

    def check_cell(self, cell_host):
        if cell_host.shape != (self.B, 3, 3):
            raise ValueError(f"cell must have shape ({self.B}, 3, 3); got {tuple(cell_host.shape)}")
        det = np.linalg.det(cell_host.astype(np.float64))
        if not np.all(np.isfinite(cell_host)) or np.any(np.abs(det) < 1e-12):
            raise ValueError("degenerate or non-finite cell")
        ext = image_extent(cell_host, self.pbc_host, self.cutoff)
        if ext.max(initial=0) > MAX_IMAGES:
            raise ValueError(f"cutoff / cell height needs {int(ext.max())} images per side (limit {MAX_IMAGES})")

    def __call__(self, R, cell, dtype=torch.int64):
        """R (A,3) device float32 | float64, cell (B,3,3) -> {key: tensor(dtype)} (distances rounded in R's dtype)."""
        out, _ = self._build(R, cell)
        return {k: (out[k] if dtype == torch.int32 else out[k].to(dtype)) for k in KEYS}

    def _build(self, R, cell):
        """-> (the int32 arrays of KEYS, workspace of the build: R, cell as the kernels read them, H, off, in_ptr)."""
        require_device(R)
        if R.dtype not in (torch.float32, torch.float64):
            raise TypeError("positions must be float32 or float64")
        R = R.detach().contiguous()
        assert R.shape == (self.A, 3)
        cell = torch.as_tensor(cell).detach().to(device=R.device, dtype=R.dtype).reshape(-1, 3, 3).contiguous()
        self.check_cell(cell.cpu().numpy())
        dev, i32, i64 = R.device, torch.int32, torch.int64
        f64 = int(R.dtype == torch.float64)
        lib = _lib.load()
        A = self.A
        cnt = torch.empty(max(A, 1), dtype=i64, device=dev)
        off = torch.zeros(A + 1, dtype=i64, device=dev)
        check(lib.gn_pbc_index_count(ptr(R), f64, ptr(cell), ptr(self.pbc), ptr(self.mol_off), ptr(self.atom_mol), self.B, A,
                                     self.cutoff, ptr(cnt), ptr(off), stream()), "gn_pbc_index_count")
        H = int(off[A].item())
        E = 2 * H
        if E >= 2 ** 31:
            raise ValueError("number of periodic edges exceeds int32")
        new = lambda *s, t=i32: torch.empty(s, dtype=t, device=dev)
        out = {"batch_seg": new(A)}
        for k in ("id_a", "id_c", "id_undir", "id_swap"):
            out[k] = new(E)
        out["cell_offsets"] = new(E, 3)
        deg, in_ptr, in_edge = new(max(A, 1), t=i64), new(A + 1, t=i64), new(max(E, 1))
        cnt3, off3 = new(max(E, 1), t=i64), torch.zeros(E + 1, dtype=i64, device=dev)
        check(lib.gn_pbc_index_fill(ptr(R), f64, ptr(cell), ptr(self.pbc), ptr(self.mol_off), ptr(self.atom_mol), A, self.cutoff,
                                    ptr(off), H, ptr(out["batch_seg"]), ptr(out["id_a"]), ptr(out["id_c"]), ptr(out["id_undir"]),
                                    ptr(out["id_swap"]), ptr(out["cell_offsets"]), ptr(deg), ptr(in_ptr), ptr(in_edge),
                                    ptr(cnt3), ptr(off3), stream()), "gn_pbc_index_fill")
        T = int(off3[E].item()) if E else 0
        if T >= 2 ** 31:
            raise ValueError("number of periodic triplets exceeds int32")
        for k in ("id3_reduce_ca", "id3_expand_ba", "Kidx3"):
            out[k] = new(T)
        check(lib.gn_pbc_index_trip(ptr(out["id_a"]), E, ptr(in_ptr), ptr(in_edge), ptr(off3), ptr(out["id3_reduce_ca"]),
                                    ptr(out["id3_expand_ba"]), ptr(out["Kidx3"]), stream()), "gn_pbc_index_trip")
        return out, dict(R=R, cell=cell, H=H, off=off, in_ptr=in_ptr)


class PeriodicQuadGraphBuilder(PeriodicGraphBuilder):
    """Device index build of periodic structures for GemNet-Q: the dict of `PeriodicGraphBuilder` (the same arrays, bit for
    bit) + the reference's quadruplet keys (data_container.py:428-489) with every node identified by (atom, image) +
    `int_cell_offsets` (n_int,3): interaction edge k = (id4_int_b -> id4_int_a) has b in the image int_cell_offsets[k] of a.
    Order and image rule: include/gemnet_hip.h (gn_pbc_qindex_*); without images the arrays are `DeviceGraphBuilder`'s.

        idx = PeriodicQuadGraphBuilder(N, cutoff, int_cutoff, pbc=pbc)(R, cell)

    Four size read-backs per call (edges, triplets, interaction edges, intermediate triplets + quadruplets)."""

    def __init__(self, N, cutoff, int_cutoff, pbc=None, device="cuda"):
        super().__init__(N, cutoff, pbc=pbc, device=device)
        self.int_cutoff = float(int_cutoff)

    def check_cell(self, cell_host):
        super().check_cell(cell_host)
        ext = image_extent(cell_host, self.pbc_host, max(self.cutoff, self.int_cutoff))
        if ext.max(initial=0) > MAX_IMAGES:
            raise ValueError(f"int_cutoff / cell height needs {int(ext.max())} images per side (limit {MAX_IMAGES})")

    def __call__(self, R, cell, dtype=torch.int64):
        out, ws = self._build(R, cell)
        R, cell, H, off, in_ptr = ws["R"], ws["cell"], ws["H"], ws["off"], ws["in_ptr"]
        dev, i32, i64 = R.device, torch.int32, torch.int64
        f64 = int(R.dtype == torch.float64)
        lib = _lib.load()
        A, E = self.A, 2 * H
        new = lambda *s, t=i32: torch.empty(s, dtype=t, device=dev)
        if H == 0:
            in_ptr = torch.zeros(A + 1, dtype=i64, device=dev)      # (gn_pbc_index_fill leaves it unwritten without edges)
        cnt = new(max(A, 1), t=i64)
        off_int = torch.zeros(A + 1, dtype=i64, device=dev)
        check(lib.gn_pbc_qindex_count(ptr(R), f64, ptr(cell), ptr(self.pbc), ptr(self.mol_off), ptr(self.atom_mol), self.B, A,
                                      self.int_cutoff, ptr(cnt), ptr(off_int), stream()), "gn_pbc_qindex_count")
        n_int = int(off_int[A].item())
        if n_int >= 2 ** 31:
            raise ValueError("number of periodic interaction edges exceeds int32")
        out["id4_int_a"], out["id4_int_b"], out["int_cell_offsets"] = new(n_int), new(n_int), new(n_int, 3)
        in_src, pos_src = new(max(E, 1)), new(max(E, 1))
        cnt_ca, cnt_db = new(max(n_int, 1), t=i64), new(max(n_int, 1), t=i64)
        off_ca, off_db = torch.zeros(n_int + 1, dtype=i64, device=dev), torch.zeros(n_int + 1, dtype=i64, device=dev)
        cnt4, off4 = new(max(E, 1), t=i64), torch.zeros(E + 1, dtype=i64, device=dev)
        check(lib.gn_pbc_qindex_int(ptr(R), f64, ptr(cell), ptr(self.pbc), ptr(self.mol_off), ptr(self.atom_mol), A,
                                    self.int_cutoff, ptr(off_int), n_int, ptr(off), H, ptr(out["id_a"]), ptr(out["id_c"]),
                                    ptr(out["cell_offsets"]), ptr(in_ptr), ptr(out["id4_int_a"]), ptr(out["id4_int_b"]),
                                    ptr(out["int_cell_offsets"]), ptr(in_src), ptr(pos_src), ptr(cnt_ca), ptr(off_ca),
                                    ptr(cnt_db), ptr(off_db), ptr(cnt4), ptr(off4), stream()), "gn_pbc_qindex_int")
        n_ca, n_db, Q = (int(v) for v in torch.stack([off_ca[n_int], off_db[n_int], off4[E]]).tolist())
        if max(n_ca, n_db) >= 2 ** 31:
            raise ValueError("number of periodic intermediate triplets exceeds int32")
        if Q >= 2 ** 31:
            raise ValueError("number of periodic quadruplets exceeds int32")
        out.update(id4_reduce_intm_ca=new(n_ca), id4_reduce_intm_ab=new(n_ca), id4_expand_intm_db=new(n_db),
                   id4_expand_intm_ab=new(n_db))
        for k in ("id4_reduce_ca", "id4_expand_db", "id4_reduce_cab", "id4_expand_abd", "Kidx4"):
            out[k] = new(Q)
        check(lib.gn_pbc_qindex_quad(ptr(self.mol_off), ptr(self.atom_mol), A, ptr(off), H, ptr(out["id_a"]), ptr(out["id_c"]),
                                     ptr(out["cell_offsets"]), ptr(in_ptr), ptr(in_src), ptr(pos_src), ptr(off_int), n_int,
                                     ptr(out["id4_int_a"]), ptr(out["id4_int_b"]), ptr(out["int_cell_offsets"]), ptr(off_ca),
                                     ptr(off_db), n_ca, n_db, ptr(off4), Q, ptr(out["id4_reduce_intm_ca"]),
                                     ptr(out["id4_reduce_intm_ab"]), ptr(out["id4_expand_intm_db"]),
                                     ptr(out["id4_expand_intm_ab"]), ptr(out["id4_reduce_ca"]), ptr(out["id4_expand_db"]),
                                     ptr(out["id4_reduce_cab"]), ptr(out["id4_expand_abd"]), ptr(out["Kidx4"]), stream()),
              "gn_pbc_qindex_quad")
        return {k: (out[k] if dtype == torch.int32 else out[k].to(dtype)) for k in KEYS + KEYS_Q}


class PeriodicCapacityGraphBuilder(PeriodicGraphBuilder):
    """`PeriodicGraphBuilder` whose layout can change: `n_mol` structures per batch inside an atom capacity `a_cap`, their sizes
    N and periodic axes set per batch.  It owns `mol_off` (n_mol + 2), `atom_mol` (a_cap) and `pbc` (n_mol + 1,3) as device
    buffers of the capacity shapes (the filler atoms between the batch and a_cap form "structure" n_mol:
    padded.capacity_layout), and the sizes as the in-graph layout reads them: `N32` (n_mol) int32, `n_atoms` (1) int32.

        builder = PeriodicCapacityGraphBuilder(n_mol, a_cap, cutoff, device=dev)
        builder.set_layout(N, pbc)                     # host or device arrays
        idx = builder(R, cell)                         # = PeriodicGraphBuilder(N, cutoff, pbc=pbc)(R, cell), array for array

    Attached to a periodic `padded.PaddedGraphRunner` with `a_cap` the layout (gn_pbc_layout) and the list
    (gn_pbc_index_padded_tv) are built inside the replay from these buffers."""

    def __init__(self, n_mol, a_cap, cutoff, device="cuda"):
        self.B, self.a_cap = int(n_mol), int(a_cap)
        if not 0 < self.B <= self.a_cap:
            raise ValueError(f"need 0 < n_mol <= a_cap; got n_mol = {self.B}, a_cap = {self.a_cap}")
        self.A = None                       # atoms of the current layout (known on the host once a batch came by)
        self.cutoff = float(cutoff)
        self.device = torch.device(device)
        dev = self.device
        self.pbc = torch.ones(self.B + 1, 3, dtype=torch.uint8, device=dev)
        self.mol_off = torch.zeros(self.B + 2, dtype=torch.int32, device=dev)
        self.atom_mol = torch.full((self.a_cap,), self.B, dtype=torch.int32, device=dev)
        self.N32 = torch.ones(self.B, dtype=torch.int32, device=dev)
        self.n_atoms = torch.zeros(1, dtype=torch.int32, device=dev)
        self._pbc_host = np.ones((self.B, 3), dtype=bool)

    @property
    def pbc_host(self):
        if self._pbc_host is None:          # (axes handed in on the device: read back when a host check asks)
            self._pbc_host = self.pbc[:self.B].cpu().numpy().astype(bool)
        return self._pbc_host

    def set_layout(self, N=None, pbc=None, n_atoms=None, arrays=True):
        """Sizes N (n_mol,) and periodic axes pbc (n_mol,3) or (3,) of the next batch, host or device arrays (None: as they
        are).  No host sync.  `n_atoms`: the atom count the in-graph layout checks sum(N) against (default: sum of a host N);
        `arrays=False` leaves `mol_off` / `atom_mol` to the in-graph layout kernel."""
        if N is not None:
            on_dev = torch.is_tensor(N) and N.device.type != "cpu"
            Nt = N if torch.is_tensor(N) else torch.as_tensor(np.asarray(N, dtype=np.int64))
            Nt = Nt.reshape(-1)
            if int(Nt.shape[0]) != self.B:
                raise ValueError(f"N must hold {self.B} structure sizes; got {int(Nt.shape[0])}")
            if not on_dev and n_atoms is None:
                n_atoms = int(Nt.sum())
            self.N32.copy_(Nt)
            self.A = None if n_atoms is None else int(n_atoms)
            if arrays:
                from .padded import capacity_layout
                lay = capacity_layout(self.N32, self.B, self.a_cap, self.a_cap)
                self.mol_off.copy_(lay["mol_off"])
                self.atom_mol.copy_(lay["atom_mol"])
        if n_atoms is not None:
            self.A = int(n_atoms)
            self.n_atoms.fill_(int(n_atoms))
        if pbc is not None:
            if torch.is_tensor(pbc) and pbc.device.type != "cpu":
                p = pbc.reshape(-1, 3)
                if p.shape[0] not in (1, self.B):
                    raise ValueError(f"pbc must have shape ({self.B}, 3) or (3,); got {tuple(pbc.shape)}")
                self.pbc[:self.B].copy_(p.expand(self.B, 3) != 0)
                self._pbc_host = None
            else:
                p = np.asarray(pbc.numpy() if torch.is_tensor(pbc) else pbc, dtype=bool).reshape(-1, 3)
                if p.shape[0] not in (1, self.B):
                    raise ValueError(f"pbc must have shape ({self.B}, 3) or (3,); got {p.shape}")
                self._pbc_host = np.broadcast_to(p, (self.B, 3)).copy()
                self.pbc[:self.B].copy_(torch.from_numpy(self._pbc_host.astype(np.uint8)))
        return self

    def _build(self, R, cell):
        """The host-sized build for the current layout: the kernels of `PeriodicGraphBuilder` on the capacity buffers (their
        first n_mol + 1 / A entries are that builder's arrays)."""
        A = int(R.shape[0])
        if self.A is None:
            self.A = int(self.N32.sum().item())
        if A != self.A or A > self.a_cap:
            raise ValueError(f"positions of {A} atoms for a layout of {self.A} (a_cap = {self.a_cap}): set_layout(N, pbc) first")
        return super()._build(R, cell)


def build_indices_periodic(R, N, cell, cutoff, pbc=None, dtype=torch.int64):
    return PeriodicGraphBuilder(N, cutoff, pbc=pbc, device=R.device)(R, cell, dtype=dtype)


# ------------------------------------------------------------------------------------------------ kernels
def edge_vectors(R, plan, cell):
    """V (E,3) = R[id_a] - (R[id_c] + cell_offsets @ cell[b]) (gn_pbc_edge_vec_f32), no autograd history."""
    require_device(R, cell)
    R = R.detach().float().contiguous()
    cell = cell.detach().float().contiguous()
    V = torch.empty((plan.n_edges, 3), device=R.device, dtype=torch.float32)
    check(_lib.load().gn_pbc_edge_vec_f32(ptr(R), ptr(plan.id_c.idx32), ptr(plan.id_a.idx32), ptr(plan.batch_seg.idx32),
                                          ptr(cell), ptr(plan.cell_offsets), ptr(V), plan.n_edges, stream()),
          "gn_pbc_edge_vec_f32")
    return V


class _EdgeBasisVec(torch.autograd.Function):
    """V -> D, rbf, rad (one launch); adjoint: dE/dV per edge (first order), and — while parameter gradients are on
    (ops.param_grads: direct-force training) — the gradient of the Bessel frequencies, as ops._EdgeBasis forms it."""

    @staticmethod
    def forward(ctx, V, freq, z, nrm, cutoff, p):
        E = V.shape[0]
        S, NR = z.shape
        D = torch.empty(E, device=V.device, dtype=torch.float32)
        rbf = torch.empty((E, NR), device=V.device, dtype=torch.float32)
        rad = torch.empty((E, S, NR), device=V.device, dtype=torch.float32)
        fr = freq.detach().float().contiguous()
        check(_lib.load().gn_edge_basis_vec_fwd_f32(ptr(V), ptr(fr), ptr(z), ptr(nrm), ptr(D), ptr(rbf), ptr(rad), E, NR, S,
                                                    cutoff, p, stream()), "gn_edge_basis_vec_fwd_f32")
        ctx.save_for_backward(V, fr, z, nrm, D)
        ctx.cfg = (cutoff, p)
        return D, rbf, rad

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gD, g_rbf, g_rad):
        from . import ops
        V, fr, z, nrm, D = ctx.saved_tensors
        cutoff, p = ctx.cfg
        S, NR = z.shape
        E = V.shape[0]
        c = lambda t: None if t is None else t.float().contiguous()
        W = gf = None
        if ctx.needs_input_grad[0]:
            W = torch.empty((E, 3), device=V.device, dtype=torch.float32)
            check(_lib.load().gn_edge_basis_vec_bwd_f32(ptr(c(gD)), ptr(c(g_rbf)), ptr(c(g_rad)), ptr(V), ptr(fr), ptr(z), ptr(nrm),
                                                        ptr(W), E, NR, S, cutoff, p, stream()), "gn_edge_basis_vec_bwd_f32")
        if ctx.needs_input_grad[1] and ops._PARAM_GRADS and g_rbf is not None:
            gf = (g_rbf * K.bessel_rbf(D, fr, cutoff, p, 0, 1)).sum(dim=0)
        return W, gf, None, None, None, None


def edge_basis(V, freq, z, nrm, cutoff, p):
    return _EdgeBasisVec.apply(V, freq, z, nrm, float(cutoff), int(p))


class _TripBasisVec(torch.autograd.Function):
    """V -> Y_l0 of the angle between the reduce and the expand edge of every triplet; adjoint: dE/dV summed per edge over the
    contiguous reduce segments and the expand-edge CSR (one gn_segsum_multi_f32)."""

    @staticmethod
    def forward(ctx, V, trip, S):
        red, exp = trip.reduce.idx32, trip.expand.idx32
        T = red.shape[0]
        Y = torch.empty((T, S), device=V.device, dtype=torch.float32)
        check(_lib.load().gn_trip_basis_vec_fwd_f32(ptr(V), ptr(red), ptr(exp), ptr(Y), None, T, S, stream()),
              "gn_trip_basis_vec_fwd_f32")
        ctx.save_for_backward(V)
        ctx.trip = trip
        return Y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gY):
        (V,) = ctx.saved_tensors
        trip = ctx.trip
        red, exp = trip.reduce.idx32, trip.expand.idx32
        T, S = gY.shape
        gY = gY.float().contiguous()
        Gu = torch.empty((T, 3), device=V.device, dtype=torch.float32)
        Gv = torch.empty((T, 3), device=V.device, dtype=torch.float32)
        check(_lib.load().gn_trip_basis_vec_bwd_f32(ptr(gY), ptr(V), ptr(red), ptr(exp), ptr(Gu), ptr(Gv), T, S, stream()),
              "gn_trip_basis_vec_bwd_f32")
        gV = K.segsum_multi([(Gu, *trip.reduce.csr, -1.0), (Gv, *trip.expand.csr, -1.0)], V.shape[0])
        return gV, None, None


def trip_basis(V, trip, S):
    return _TripBasisVec.apply(V, trip, int(S))


# ------------------------------------------------------------------------------------------------ GemNet-Q on vectors
def int_edge_vectors(R, plan, cell):
    """Vint (n_int,3) = R[id4_int_a] - (R[id4_int_b] + int_cell_offsets @ cell[b]): `edge_vectors` of the interaction edges."""
    require_device(R, cell)
    R = R.detach().float().contiguous()
    cell = cell.detach().float().contiguous()
    V = torch.empty((plan.n_int, 3), device=R.device, dtype=torch.float32)
    check(_lib.load().gn_pbc_edge_vec_f32(ptr(R), ptr(plan.int_b.idx32), ptr(plan.int_a.idx32), ptr(plan.batch_seg.idx32),
                                          ptr(cell), ptr(plan.int_cell_offsets), ptr(V), plan.n_int, stream()),
          "gn_pbc_edge_vec_f32")
    return V


class _RadBasisVec(torch.autograd.Function):
    """Vint -> rad (n_int,S,NR), the spherical-Bessel radial basis of the interaction edges (no Bessel rbf, no distance
    output: gn_edge_basis_vec_fwd_f32 / _bwd_f32 with those operands absent, as ops.edge_basis(want_rbf=False))."""

    @staticmethod
    def forward(ctx, V, z, nrm, cutoff, p):
        E = V.shape[0]
        S, NR = z.shape
        D = torch.empty(E, device=V.device, dtype=torch.float32)
        rad = torch.empty((E, S, NR), device=V.device, dtype=torch.float32)
        check(_lib.load().gn_edge_basis_vec_fwd_f32(ptr(V), None, ptr(z), ptr(nrm), ptr(D), None, ptr(rad), E, NR, S, cutoff, p,
                                                    stream()), "gn_edge_basis_vec_fwd_f32")
        ctx.save_for_backward(V, z, nrm)
        ctx.cfg = (cutoff, p)
        return rad

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rad):
        V, z, nrm = ctx.saved_tensors
        cutoff, p = ctx.cfg
        S, NR = z.shape
        E = V.shape[0]
        W = torch.empty((E, 3), device=V.device, dtype=torch.float32)
        check(_lib.load().gn_edge_basis_vec_bwd_f32(None, None, ptr(g_rad.float().contiguous()), ptr(V), None, ptr(z), ptr(nrm),
                                                    ptr(W), E, NR, S, cutoff, p, stream()), "gn_edge_basis_vec_bwd_f32")
        return W, None, None, None, None


def radial_basis(V, z, nrm, cutoff, p):
    return _RadBasisVec.apply(V, z, nrm, float(cutoff), int(p))


class _TripBasisVec2(torch.autograd.Function):
    """Vint, V -> Y_l0 of the a - b <- d angle of every intermediate triplet (u = Vint[intm_ab], v = -V[intm_db]); adjoint:
    dE/dVint summed over the contiguous triplets of an interaction edge, dE/dV over the intm_db CSR."""

    @staticmethod
    def forward(ctx, Vint, V, plan, S):
        T = plan.n_intm
        Y = torch.empty((T, S), device=V.device, dtype=torch.float32)
        check(_lib.load().gn_trip_basis_vec2_fwd_f32(ptr(Vint), ptr(plan.intm_ab.idx32), ptr(V), ptr(plan.intm_db.idx32), ptr(Y),
                                                     T, S, stream()), "gn_trip_basis_vec2_fwd_f32")
        ctx.save_for_backward(Vint, V)
        ctx.plan = plan
        return Y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gY):
        Vint, V = ctx.saved_tensors
        plan = ctx.plan
        T, S = gY.shape
        gY = gY.float().contiguous()
        GU = torch.empty((T, 3), device=V.device, dtype=torch.float32)
        GW = torch.empty((T, 3), device=V.device, dtype=torch.float32)
        check(_lib.load().gn_trip_basis_vec2_bwd_f32(ptr(gY), ptr(Vint), ptr(plan.intm_ab.idx32), ptr(V),
                                                     ptr(plan.intm_db.idx32), ptr(GU), ptr(GW), T, S, stream()),
              "gn_trip_basis_vec2_bwd_f32")
        return (K.segsum(GU, *plan.intm_ab.csr, plan.n_int), K.segsum(GW, *plan.intm_db.csr, plan.n_edges), None, None)


def trip_basis2(Vint, V, plan, S):
    return _TripBasisVec2.apply(Vint, V, plan, int(S))


class _QuadBasisVec(torch.autograd.Function):
    """V, Vint -> the tensor basis of every quadruplet from uac = -V[id4_reduce_ca], uab = -Vint[k], ubd = -V[id4_expand_db]:
    Y_lm rows (Q,S^2), or in angle form (Q,4) (sin, cos) of the two angles for the *_ang bilinear kernels.  Adjoint, reduced
    as ops._quad_adjoint does: per reduce edge over the contiguous quadruplet segments (-> dE/dV rows), per intermediate
    triplet through the CSR of id4_expand_abd ([dE/dVint | dE/dV[db]] rows of 32 B), then onto the V rows through the intm_db
    CSR and onto the Vint rows over the contiguous intermediate triplets of an interaction edge.  No atomics, fixed order."""

    @staticmethod
    def forward(ctx, V, Vint, plan, S, angle_form):
        Q = plan.quad.size
        lib, q = _lib.load(), plan.quad
        idx = (ptr(q.reduce.idx32), ptr(quad_expand_db(plan)), ptr(q.expand.idx32), ptr(plan.intm_ab.idx32))
        if angle_form:
            Y = torch.empty((Q, 4), device=V.device, dtype=torch.float32)
            check(lib.gn_quad_angles_vec_fwd_f32(ptr(V), ptr(Vint), *idx, ptr(Y), Q, stream()), "gn_quad_angles_vec_fwd_f32")
        else:
            Y = torch.empty((Q, S * S), device=V.device, dtype=torch.float32)
            check(lib.gn_quad_basis_vec_fwd_f32(ptr(V), ptr(Vint), *idx, ptr(Y), Q, S, stream()), "gn_quad_basis_vec_fwd_f32")
        ctx.save_for_backward(V, Vint)
        ctx.cfg = (plan, S, angle_form)
        return Y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gY):
        V, Vint = ctx.saved_tensors
        plan, S, angle_form = ctx.cfg
        Q = plan.quad.size
        lib, q = _lib.load(), plan.quad
        idx = (ptr(q.reduce.idx32), ptr(quad_expand_db(plan)), ptr(q.expand.idx32), ptr(plan.intm_ab.idx32))
        gY = gY.float().contiguous()
        Gc = torch.empty((Q, 3), device=V.device, dtype=torch.float32)
        Gbd = torch.empty((Q, 8), device=V.device, dtype=torch.float32)       # (the kernels write the two pad lanes themselves)
        if angle_form:
            check(lib.gn_quad_angles_vec_bwd_f32(ptr(gY), ptr(V), ptr(Vint), *idx, ptr(Gc), ptr(Gbd), Q, stream()),
                  "gn_quad_angles_vec_bwd_f32")
        else:
            check(lib.gn_quad_basis_vec_bwd_f32(ptr(gY), ptr(V), ptr(Vint), *idx, ptr(Gc), ptr(Gbd), Q, S, stream()),
                  "gn_quad_basis_vec_bwd_f32")
        return quad_reduce(Gc, Gbd, plan) + (None, None, None)


def quad_reduce(Gc, Gbd, plan):
    """The per-quadruplet adjoint rows Gc (Q,3) = dE/dV[ca], Gbd (Q,8) = [dE/dVint[k] | dE/dV[db]] -> (gV (E,3), gVint (n_int,3)):
    the three-level reduction of `_QuadBasisVec` (shared with the training twin, ops_train._QuadAnglesVec2)."""
    q = plan.quad
    Ec = K.segsum(Gc, None, q.seg_off, plan.n_edges)
    Ibd = K.segsum(Gbd, *q.expand.csr, q.n_expand)
    gV = Ec + K.segsum(Ibd[:, 4:7].contiguous(), *plan.intm_db.csr, plan.n_edges)
    gVint = K.segsum(Ibd[:, 0:3].contiguous(), *plan.intm_ab.csr, plan.n_int)
    return gV, gVint


def quad_index(plan):
    """The four int32 index arrays of the quadruplet kernels on vectors: q_ca, q_db, q_abd, intm_ab."""
    q = plan.quad
    return q.reduce.idx32, quad_expand_db(plan), q.expand.idx32, plan.intm_ab.idx32


def quad_angles_vec_fwd(V, Vint, plan):
    """ang (Q,4) = (sin, cos) of Phi_cab and Theta_cabd from (V, Vint) (gn_quad_angles_vec_fwd_f32), no autograd history."""
    Q = plan.quad.size
    ang = torch.empty((Q, 4), device=V.device, dtype=torch.float32)
    check(_lib.load().gn_quad_angles_vec_fwd_f32(ptr(V), ptr(Vint), *(ptr(i) for i in quad_index(plan)), ptr(ang), Q, stream()),
          "gn_quad_angles_vec_fwd_f32")
    return ang


def quad_angles_vec_adjoint(g_ang, V, Vint, plan):
    """First adjoint of the angle form on vectors: g_ang (Q,4) = (dE/dPhi, dE/dTheta, -, -) -> (gV, gVint)
    (gn_quad_angles_vec_bwd_f32 + `quad_reduce`)."""
    Q = plan.quad.size
    g_ang = g_ang.float().contiguous()
    Gc = torch.empty((Q, 3), device=V.device, dtype=torch.float32)
    Gbd = torch.empty((Q, 8), device=V.device, dtype=torch.float32)       # (the kernel writes the two pad lanes itself)
    check(_lib.load().gn_quad_angles_vec_bwd_f32(ptr(g_ang), ptr(V), ptr(Vint), *(ptr(i) for i in quad_index(plan)), ptr(Gc),
                                                 ptr(Gbd), Q, stream()), "gn_quad_angles_vec_bwd_f32")
    return quad_reduce(Gc, Gbd, plan)


def quad_expand_db(plan):
    """id4_expand_db as int32 (a periodic GemNet-Q plan keeps it: graph.GraphPlan)."""
    return plan.q_db32


def quad_basis(V, Vint, plan, S, angle_form=False):
    from . import ops
    return _QuadBasisVec.apply(V, Vint, plan, int(S), bool(angle_form and ops.USE_QUAD_ANGLES and S == 7))


def forces(G, plan):
    """F (A,3) from G = -dE/dV: F = segsum(G, id_a) - segsum(G, id_c)."""
    return K.segsum_multi([(G, *plan.id_a.csr, 1.0), (G, *plan.id_c.csr, -1.0)], plan.n_atoms)


def forces_q(G, Gint, plan):
    """F (A,3) of a periodic GemNet-Q batch from G = -dE/dV and Gint = -dE/dVint: the four edge -> atom sums in one launch."""
    return K.segsum_multi([(G, *plan.id_a.csr, 1.0), (G, *plan.id_c.csr, -1.0), (Gint, *plan.int_a.csr, 1.0),
                           (Gint, *plan.int_b.csr, -1.0)], plan.n_atoms)


def direct_forces(terms, V, plan, coupled):
    """F (A,T,3) of a direct-force model (gemnet.py:580-596) in one launch (gn_direct_force_f32): terms (K,E,T), the per-edge
    force magnitudes of the K output blocks; V (E,3) = `edge_vectors`; `coupled`: average the two directions of every
    undirected edge first (`plan.id_swap` pairs an edge with its negated-offset partner).  Inference only: no autograd."""
    perm, seg = plan.id_a.csr
    return K.direct_force(terms.detach(), V.detach(), plan.id_swap.idx32 if coupled else None, perm, seg, plan.n_atoms)


class _DirectForces(torch.autograd.Function):
    """The K (E,T) force terms of the output blocks -> F (A,T,3): `direct_forces` with a graph to the terms.  V, the coupling and
    the CSR are constants (positions and cell never join an autograd graph).  Backward: ONE launch of the head's adjoint
    (gn_direct_force_bwd_f32); d/dterms[k] is the same (E,T) array for every k and the SAME tensor is returned K times.  That is
    safe here: term k has exactly one consumer (this Function), so the engine hands the tensor straight to the backward of the
    Dense that produced the term (ops._FusedDense / ops._MM) without accumulating into it, and those only read their cotangent —
    the running sums of ops.accumulate_gradient are written into buffers of their own (GradSink.target), the weight-gradient
    queue reads, and AccumulateGrad adds into the flat gradient buffer."""

    @staticmethod
    def forward(ctx, V, plan, coupled, *terms):
        ctx.set_materialize_grads(False)
        perm, seg = plan.id_a.csr
        ctx.swap = plan.id_swap.idx32 if coupled else None
        ctx.plan, ctx.n_terms = plan, len(terms)
        ctx.save_for_backward(V)
        return K.direct_force(torch.stack([t.detach() for t in terms]), V.detach(), ctx.swap, perm, seg, plan.n_atoms)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gF):
        if gF is None:
            return (None,) * (3 + ctx.n_terms)
        (V,) = ctx.saved_tensors
        g = K.direct_force_bwd(gF, V, ctx.swap, ctx.plan.id_a.idx32, ctx.plan.n_atoms)
        return (None, None, None) + (g,) * ctx.n_terms


def direct_forces_train(terms_list, V, plan, coupled):
    """F (A,T,3) of a direct-force model with an autograd graph to the K (E,T) tensors of `terms_list` (the force terms of the
    output blocks): the forward is `direct_forces` on their stack, the backward one launch of its adjoint.  V gets no gradient."""
    return _DirectForces.apply(V, plan, bool(coupled), *terms_list)


def edge_structure(plan):
    """Edges grouped by structure (CSR of batch_seg[id_a], gn_csr_build_i32), built once per plan."""
    if getattr(plan, "_edge_mol", None) is None:
        key = plan.batch_seg.idx32.index_select(0, plan.id_a.idx32.long()).to(torch.int32)
        plan._edge_mol = RowIndex(key, plan.n_mol)
    return plan._edge_mol


def stress(V, G, plan, cell):
    """S (B,3,3) = -1/|det cell_b| sum_e V_e (x) G_e = dE/d(strain) / volume  (gn_pbc_stress_f32)."""
    perm, seg = edge_structure(plan).csr
    cell = cell.detach().float().contiguous()
    S = torch.empty((plan.n_mol, 3, 3), device=V.device, dtype=torch.float32)
    check(_lib.load().gn_pbc_stress_f32(ptr(V), ptr(G.contiguous()), ptr(perm), ptr(seg), ptr(cell), plan.n_mol, -1.0, ptr(S),
                                        stream()), "gn_pbc_stress_f32")
    return S


def stress_q(V, G, Vint, Gint, plan, cell):
    """S (B,3,3) of a periodic GemNet-Q batch: -1/|det cell_b| (sum_e V_e (x) G_e + sum_k Vint_k (x) Gint_k) over the edges and
    interaction edges of structure b (two launches of gn_pbc_stress_f32; the interaction edges are grouped by `plan.int_mol`)."""
    _, seg = plan.int_mol.csr
    cell_f = cell.detach().float().contiguous()
    Si = torch.empty((plan.n_mol, 3, 3), device=V.device, dtype=torch.float32)
    check(_lib.load().gn_pbc_stress_f32(ptr(Vint), ptr(Gint.contiguous()), None, ptr(seg), ptr(cell_f), plan.n_mol, -1.0, ptr(Si),
                                        stream()), "gn_pbc_stress_f32")
    return stress(V, G, plan, cell) + Si


class _ForceStress(torch.autograd.Function):
    """G = -dE/dV (E,3) -> F (A,3), S (B,3,3): `forces` + `stress`, differentiable in G for the training step (V and the cell are
    constants: positions and cell never join an autograd graph).  Backward: one launch of the exact adjoint,
    gG_e = gF[a(e)] - gF[c(e)] - 1/|det cell_b| V_e . gS_b (gn_pbc_force_stress_adj_f32)."""

    @staticmethod
    def forward(ctx, G, V, plan, cell):
        ctx.set_materialize_grads(False)
        G = G.contiguous()
        ctx.save_for_backward(V, cell)
        ctx.plan = plan
        return forces(G, plan), stress(V, G, plan, cell)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gF, gS):
        V, cell = ctx.saved_tensors
        plan = ctx.plan
        if gF is None and gS is None:
            return None, None, None, None
        if gF is None:
            gF = torch.zeros((plan.n_atoms, 3), device=V.device, dtype=V.dtype)
        gG = K.pbc_force_stress_adj(gF, gS, V, plan.id_c.idx32, plan.id_a.idx32, plan.batch_seg.idx32, cell.detach(), -1.0)
        return gG, None, None, None


def force_stress(G, V, plan, cell):
    """(F, S) from G = -dE/dV with an autograd graph through G (force training on periodic batches)."""
    return _ForceStress.apply(G, V, plan, cell)


class _ForceStressQ(torch.autograd.Function):
    """G = -dE/dV (E,3), Gint = -dE/dVint (n_int,3) -> F (A,3), S (B,3,3): `forces_q` + `stress_q`, differentiable in G and Gint
    (`_ForceStress` for a periodic GemNet-Q batch).  Backward: the adjoint kernel once per edge family — over the edges, and
    over the interaction edges with int_b, int_a in the roles of id_c, id_a (both arrays are of edge size)."""

    @staticmethod
    def forward(ctx, G, V, Gint, Vint, plan, cell):
        ctx.set_materialize_grads(False)
        G, Gint = G.contiguous(), Gint.contiguous()
        ctx.save_for_backward(V, Vint, cell)
        ctx.plan = plan
        return forces_q(G, Gint, plan), stress_q(V, G, Vint, Gint, plan, cell)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gF, gS):
        V, Vint, cell = ctx.saved_tensors
        plan = ctx.plan
        if gF is None and gS is None:
            return (None,) * 6
        if gF is None:
            gF = torch.zeros((plan.n_atoms, 3), device=V.device, dtype=V.dtype)
        bs, cell = plan.batch_seg.idx32, cell.detach()
        gG = K.pbc_force_stress_adj(gF, gS, V, plan.id_c.idx32, plan.id_a.idx32, bs, cell, -1.0)
        gGint = K.pbc_force_stress_adj(gF, gS, Vint, plan.int_b.idx32, plan.int_a.idx32, bs, cell, -1.0)
        return gG, None, gGint, None, None, None


def force_stress_q(G, V, Gint, Vint, plan, cell):
    """(F, S) of a periodic GemNet-Q batch from G = -dE/dV and Gint = -dE/dVint with an autograd graph through both (force
    training; the stress cotangent may be None)."""
    return _ForceStressQ.apply(G, V, Gint, Vint, plan, cell)
