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
runtime.DynamicForceField(cell=...), md.predict_periodic.
"""
import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check, ptr, require_device, stream
from .graph import RowIndex

KEYS = ["batch_seg", "id_undir", "id_swap", "id_c", "id_a", "id3_expand_ba", "id3_reduce_ca", "Kidx3", "cell_offsets"]
MAX_IMAGES = 64       # images per axis and side the builder accepts (cutoff / perpendicular height)


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
            raise NotImplementedError("periodic cells: GemNet-T (triplets_only=True) only; GemNet-Q has no periodic index build")
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
        return {k: (out[k] if dtype == torch.int32 else out[k].to(dtype)) for k in KEYS}


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


def forces(G, plan):
    """F (A,3) from G = -dE/dV: F = segsum(G, id_a) - segsum(G, id_c)."""
    return K.segsum_multi([(G, *plan.id_a.csr, 1.0), (G, *plan.id_c.csr, -1.0)], plan.n_atoms)


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
