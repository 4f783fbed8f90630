"""Helpers of the tests of direct-force TRAINING on periodic batches: the fp64 closed form of the force head's adjoint
(gn_direct_force_bwd_f32) with its derived error bound, a torch restatement of the head's forward, the gradient oracle (the fp64
cluster oracle with the parameters as leaves: exact autograd, no finite differences), and the context manager that swaps the
launchers of this path for fp64 stand-ins beside pbc_train_common.emulate()."""
import contextlib
import functools

import numpy as np
import torch

import cpu_kernels
import pbc_common as P
import pbc_direct_common as D
import pbc_train_common as PT
from oracle import gemnet_oracle as GO

CASES = ("sc1", "sc08", "zoo")


# ------------------------------------------------------------------------------------------------ the adjoint in fp64
def _unit(V):
    V = np.asarray(V, np.float64)
    return V / np.linalg.norm(V, axis=1)[:, None]


def direct_force_bwd_ref(gF, V, id_swap, id_a):
    """g (E,T) float64 of gn_direct_force_bwd_f32: h[e,t] = <gF[id_a[e],t,:], V_e / |V_e|>, coupled: the mean of h[e] and
    h[id_swap[e]].  d/dterms[k] = g for every k."""
    gF = np.asarray(gF, np.float64)
    h = np.einsum("eti,ei->et", gF[np.asarray(id_a)], _unit(V))
    return h if id_swap is None else 0.5 * (h + h[np.asarray(id_swap)])


def bwd_error_bound(gF, V, id_swap, id_a):
    """(E,T) bound of |g - g_ref| of the fp32 kernel: 12 * 2^-24 * m, m[e,t] = sum_i |gF[id_a[e],t,i]| |u_{e,i}| (coupled: the mean
    of m[e] and m[id_swap[e]]).  The three products and two adds of the dot product, <= 4 ulp for the sum of squares, the square
    root and the divide behind every u_i, one add for the coupling (the halving is exact); the rest is margin."""
    gF = np.abs(np.asarray(gF, np.float64))
    m = np.einsum("eti,ei->et", gF[np.asarray(id_a)], np.abs(_unit(V)))
    if id_swap is not None:
        m = 0.5 * (m + m[np.asarray(id_swap)])
    return 12.0 * 2.0 ** -24 * m


def direct_force_torch(terms, V, id_swap, id_a, n_atoms):
    """The head's forward (pbc_direct_common.direct_force_ref) in differentiable torch: terms (K,E,T) -> F (A,T,3)."""
    c = terms.sum(0)
    if id_swap is not None:
        c = 0.5 * (c + c[id_swap.long()])
    u = V / torch.linalg.vector_norm(V, dim=1, keepdim=True)
    F = torch.zeros((n_atoms, terms.shape[2], 3), dtype=terms.dtype, device=terms.device)
    return F.index_add(0, id_a.long(), c[:, :, None] * u[:, None, :])


# ------------------------------------------------------------------------------------------------------ gradient oracle
def structures():
    return [P.structure(k, seed=i) for i, k in enumerate(D.KINDS)]


def direct_cfg(base, coupled):
    return dict(base, direct_forces=True, forces_coupled=bool(coupled))


def oracle(params, cfg, structs, names, rho_force=PT.RHO_FORCE):
    """-> dict(E (B,1), F (A,3), Et, Ft, loss, grads {name: tensor}) of the energy + force loss of training/periodic.py for a
    direct-force model: the fp64 cluster oracle on every structure (central atoms F[:n]) with the parameters as leaves, targets =
    outputs + PT.offsets, one torch.autograd.grad."""
    leaves = {k: v.detach().clone().requires_grad_(k in names) for k, v in params.items()}
    Es, Fs = [], []
    for R, Z, cell, pbc in structs:
        E, F = GO.forward(cfg, leaves, PT._cluster_inputs(R, Z, cell, pbc, cfg))
        Es.append(E[0:1])
        Fs.append(F[:len(R), 0])
    E, F = torch.cat(Es), torch.cat(Fs)
    oE, oF, _ = PT.offsets(structs)
    Et, Ft = E.detach() + torch.tensor(oE), F.detach() + torch.tensor(oF)
    S = torch.zeros(len(structs), 3, 3, dtype=torch.float64)
    loss = PT.loss_fp64(E, F, S, Et, Ft, S, rho_force=rho_force, rho_stress=0.0)
    grads = torch.autograd.grad(loss, [leaves[n] for n in names])
    return dict(E=E.detach(), F=F.detach(), Et=Et, Ft=Ft, loss=float(loss.detach()), grads=dict(zip(names, grads)))


@functools.lru_cache(maxsize=None)
def make_params(tag, coupled):
    """The oracle's weights of configuration `tag` ('cfg': pbc_common.CFG, 'wide': pbc_train_common.CFG_WIDE) as a direct-force
    model."""
    return PT.make_params(direct_cfg({"cfg": P.CFG, "wide": PT.CFG_WIDE}[tag], coupled))


# -------------------------------------------------------------------------------- fp64 stand-ins of what the path launches
class _EdgeBasisVec(torch.autograd.Function):
    """pbc.edge_basis on cpu_kernels.edge_basis_vec_fwd / _bwd, with the frequency gradient of pbc._EdgeBasisVec."""

    @staticmethod
    def forward(ctx, V, freq, z, nrm, cutoff, p):
        D_, rbf, rad = cpu_kernels.edge_basis_vec_fwd(V.detach(), freq.detach(), z, nrm, cutoff, p)
        ctx.save_for_backward(V, freq, z, nrm, D_)
        ctx.cfg = (cutoff, p)
        return D_, rbf, rad

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gD, g_rbf, g_rad):
        V, freq, z, nrm, D_ = ctx.saved_tensors
        cutoff, p = ctx.cfg
        W = gf = None
        if ctx.needs_input_grad[0]:
            W = cpu_kernels.edge_basis_vec_bwd(gD, g_rbf, g_rad, V, freq, z, nrm, cutoff, p)
        if ctx.needs_input_grad[1]:
            gf = (g_rbf * cpu_kernels.bessel_rbf(D_, freq, cutoff, p, 0, 1)).sum(dim=0)
        return W, gf, None, None, None, None


def edge_basis(V, freq, z, nrm, cutoff, p):
    return _EdgeBasisVec.apply(V, freq, z, nrm, float(cutoff), int(p))


def trip_basis(V, trip, S):
    assert not V.requires_grad      # (the edge vectors of direct-force training are constants)
    return cpu_kernels.trip_basis_vec_fwd(V, trip.reduce.idx32, trip.expand.idx32, int(S))[0]


def direct_force(terms, V, id_swap, perm, seg_off, n_atoms, out=None):
    seg = seg_off.long()
    id_a = torch.repeat_interleave(torch.arange(int(n_atoms)), seg[1:] - seg[:-1])
    if perm is not None:
        id_a = torch.empty_like(id_a).index_copy_(0, perm.long(), id_a)
    F = direct_force_torch(terms, V, id_swap, id_a, int(n_atoms))
    return F if out is None else out.copy_(F)


def direct_force_bwd(gF, V, id_swap, id_a, n_atoms, out=None):
    h = torch.einsum("eti,ei->et", gF[id_a.long()], V / torch.linalg.vector_norm(V, dim=1, keepdim=True))
    g = h if id_swap is None else 0.5 * (h + h[id_swap.long()])
    return g if out is None else out.copy_(g)


_K_NAMES = ["direct_force", "direct_force_bwd"]
_PBC_NAMES = ["edge_basis", "trip_basis"]


@contextlib.contextmanager
def emulate():
    """pbc_train_common.emulate() + the launchers of the direct-force periodic training path (tests only)."""
    import gemnet_pytorch_amd.kernels as K
    import gemnet_pytorch_amd.pbc as PB
    saved = [(m, n, getattr(m, n)) for m, names in ((K, _K_NAMES), (PB, _PBC_NAMES)) for n in names]
    with PT.emulate():
        try:
            for m, n, _ in saved:
                setattr(m, n, globals()[n])
            yield
        finally:
            for m, n, f in saved:
                setattr(m, n, f)
