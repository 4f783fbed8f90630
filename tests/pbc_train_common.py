"""Test infrastructure of periodic TRAINING (fp64, CPU): the gradient oracle of the loss of training/periodic.py built from the
cluster oracle of tests/pbc_common.py, fp64 restatements of the launchers of csrc/pbc_train.hip, and the context manager that
swaps them (and the pbc.* wrappers that call the library directly) in beside cpu_kernels.emulate().

Gradient oracle.  The periodic energy of structure b is E[0,0] of the molecular fp64 oracle on a finite cluster, with the
parameters as leaves, so grad_theta E_b is one backward.  With the cotangents gE = dL/dE, u = dL/dF, w = dL/dS at the oracle's own
E, F, S (F, S: pbc_common.fd_forces_stress) and F = -dE/dR, S = dE/d(strain)/|det cell|:

    grad_theta L = sum_b  gE_b grad_theta E_b  -  d/dh grad_theta E_b(R + h u_b)
                          +  1/|det cell_b|  d/dh grad_theta E_b(R (I + h w_b), cell_b (I + h w_b))

The h-derivatives are central differences of grad_theta E_b along the direction scaled to unit max-norm, at h = 1e-4 and 2e-4,
combined by Richardson, (4 D(h) - D(2h)) / 3.  `directional` asserts |D(h) - D(2h)| <= 1e-4 |D(h)| — a condition on the
oracle (its truncation error is then ~1e-5 of that difference), not on the code under test."""
import contextlib

import numpy as np
import torch

import cpu_kernels
import pbc_common as P
from oracle import gemnet_oracle as GO
from oracle import index_oracle as IO

KINDS = ["small", "triclinic", "slab", "cubic1"]
# cells with a height below the cutoff (self-image edges, image ranges up to |n| = 3, image distances below 1 A, exactly collinear
# triplets) and one with det < 0: tests/test_pbc_train_cells_cpu.py, tests/test_gpu_pbc_train_cells.py
HARD = ("bcc_pert", "thin", "skewed", "skewed_lh")
RHO_FORCE, RHO_STRESS = 0.9, 0.05
# the widths for which kernels.bil_train_supported(S, C, I) holds (S = 7, C = emb_size_trip = 64, I = emb_size_cbf = 16) and the
# Dense stacks are 128 wide; everything that is not a width as in pbc_common.CFG (the cluster oracle reads widths off the weights)
CFG_WIDE = dict(P.CFG, emb_size_atom=128, emb_size_edge=128, emb_size_trip=64, emb_size_cbf=16, emb_size_rbf=16,
                emb_size_bil_trip=64)
H = 1e-4


def structures():
    return [P.structure(k, seed=i) for i, k in enumerate(KINDS)]


def make_params(cfg, seed=3):
    import os
    from conftest import ROOT
    return GO.make_params(cfg, seed, GO.load_scale_factors(os.path.join(ROOT, "gemnet_pytorch_amd", "scaling_factors.json")))


# ------------------------------------------------------------------------------------------------------------ gradient oracle
def _cluster_inputs(R, Z, cell, pbc, cfg):
    Rc, Zc = P.cluster(R, Z, cell, pbc, P.RADIUS)
    n = len(R)
    idx = IO.build_indices(Rc, np.array([len(Rc)]), cfg["cutoff"], 10.0, True)
    inputs = {k: torch.tensor(v) for k, v in idx.items()}
    bs = np.zeros(len(Rc), np.int64)
    bs[n:] = 1
    inputs.update(Z=torch.tensor(Zc).long(), R=torch.tensor(Rc), batch_seg=torch.tensor(bs), N=torch.tensor([n, len(Rc) - n]))
    return inputs


def energy_gradient(params, names, R, Z, cell, pbc, cfg):
    """grad_theta of the periodic energy of one structure: one backward through the cluster oracle (as pbc_common.cluster_energy
    builds it), parameters as leaves.  -> (E, {name: gradient})."""
    leaves = {k: v.detach().clone().requires_grad_(k in names) for k, v in params.items()}
    E, _ = GO.forward(cfg, leaves, _cluster_inputs(R, Z, cell, pbc, cfg), need_forces=False)
    grads = torch.autograd.grad(E[0, 0], [leaves[n] for n in names], allow_unused=True)
    return float(E[0, 0].detach()), {n: (torch.zeros_like(leaves[n]) if g is None else g) for n, g in zip(names, grads)}


def directional(grad_at, direction, g_norm):
    """d/dh grad_at(h * direction) at h = 0 -> ({name: Richardson value}, |D(h) - Richardson| over all names).
    `g_norm`: |grad_at(0)|, which sets the rounding floor of a central difference, ~eps |g| / h — a direction along which the
    gradient does not change at all (the one atom of 'cubic1': moving it is a translation) yields nothing but that floor."""
    scale = float(np.abs(direction).max())
    if scale == 0.0:
        return None, 0.0
    d = direction / scale

    def central(h):
        gp, gm = grad_at(h * d), grad_at(-h * d)
        return {n: (gp[n] - gm[n]) / (2 * h) for n in gp}
    D1, D2 = central(H), central(2 * H)
    flat = lambda D: torch.cat([D[n].reshape(-1) for n in sorted(D)])       # noqa: E731
    f1, f2 = flat(D1), flat(D2)
    floor = 8 * np.finfo(np.float64).eps * g_norm / H
    assert float((f1 - f2).norm()) <= 1e-4 * float(f1.norm()) + floor, (float((f1 - f2).norm()), float(f1.norm()), floor)
    rich = {n: (4 * D1[n] - D2[n]) / 3 * scale for n in D1}
    return rich, float((f1 * scale - flat(rich)).norm())


def offsets(structs):
    """Fixed target offsets of magnitude 0.1 .. 1 (random signs): no |.| or norm of the loss sits at its kink."""
    rs = np.random.RandomState(11)
    draw = lambda *s: rs.uniform(0.1, 1.0, s) * rs.choice([-1.0, 1.0], s)       # noqa: E731
    A = sum(len(s[0]) for s in structs)
    return draw(len(structs), 1), draw(A, 3), draw(len(structs), 3, 3)


def loss_fp64(E, F, S, Et, Ft, St, rho_force=RHO_FORCE, rho_stress=RHO_STRESS):
    """The loss of training/periodic.py on one rank, plain torch."""
    B = E.shape[0]
    return ((1 - rho_force) * (E - Et).abs().mean() + rho_force * torch.linalg.vector_norm(F - Ft, dim=1).mean()
            + rho_stress * torch.linalg.vector_norm((S - St).reshape(B, 9), dim=1).sum() / B)


def hard_structures(kinds=HARD):
    """The structures of `kinds` as pbc_common.structure gives them (seed 0: the cells of tests/test_gpu_pbc_cases.py)."""
    return [P.structure(k) for k in kinds]


def collinear_rows(structs):
    """Edge vectors and triplets of the float32-rounded structures from the brute-force list -> (V float32 (E,3), index dict,
    cells float64 (B,3,3) (float32-rounded), rows with theta = 0, rows with theta = pi): the triplets whose cross product is
    EXACTLY zero in float32 arithmetic on the float32 edge vectors — the rows that reach the max(|u x v|, 1e-9) clamp."""
    R, Z, N, cell, pbc = P.arrays([P.f32_round(s) for s in structs])
    idx = P.brute_force(R, N, cell, pbc, P.CUTOFF)
    shift = np.einsum("ek,ekj->ej", idx["cell_offsets"].astype(np.float64), cell[idx["batch_seg"][idx["id_a"]]])
    V = (R[idx["id_a"]] - (R[idx["id_c"]] + shift)).astype(np.float32)
    u, v = -V[idx["id3_reduce_ca"]], -V[idx["id3_expand_ba"]]
    w = np.cross(u, v)
    assert w.dtype == np.float32
    zero = (w == 0).all(1)
    x = (u * v).sum(1)
    return V, idx, cell, np.nonzero(zero & (x > 0))[0], np.nonzero(zero & (x < 0))[0]


def energies_forces_stress(params, cfg, structs, richardson=False, fd_h=1e-4):
    """The cluster oracle's own (E (B,1), F (A,3), S (B,3,3)) of a batch — most of the cost of `oracle`, and independent of the
    loss weights: compute it once and hand it to `oracle(..., efs=)` for every (rho_force, rho_stress)."""
    Es, Fs, Ss = [], [], []
    for R, Z, cell, pbc in structs:
        Es.append(P.cluster_energy(params, R, Z, cell, pbc, cfg=cfg))
        # (cluster_energy's default cfg: widths come from the weights)
        F, S = P.fd_forces_stress(params, R, Z, cell, pbc, h=fd_h, richardson=richardson)
        Fs.append(F)
        Ss.append(S)
    return torch.tensor(Es, dtype=torch.float64)[:, None], torch.tensor(np.concatenate(Fs)), torch.tensor(np.stack(Ss))


def oracle(params, cfg, structs, names, rho_force=RHO_FORCE, rho_stress=RHO_STRESS, richardson=False, fd_h=1e-4, efs=None):
    """-> dict(E (B,1), F (A,3), S (B,3,3), Et, Ft, St, loss, grads {name: tensor}, trunc): the reference of the training step.
    `richardson`, `fd_h`: the oracle's own F and S (pbc_common.fd_forces_stress) — they set the targets and thereby the
    cotangents u, w; the default is the plain central difference at h = 1e-4.  `efs`: `energies_forces_stress` of the same
    batch, computed before."""
    E, F, S = (t.detach().clone().requires_grad_(True)
               for t in (efs if efs is not None else energies_forces_stress(params, cfg, structs, richardson, fd_h)))
    oE, oF, oS = offsets(structs)
    Et, Ft, St = E.detach() + torch.tensor(oE), F.detach() + torch.tensor(oF), S.detach() + torch.tensor(oS)
    loss = loss_fp64(E, F, S, Et, Ft, St, rho_force, rho_stress)
    gE, u, w = (t.numpy() for t in torch.autograd.grad(loss, (E, F, S)))
    total = {n: torch.zeros_like(params[n]) for n in names}
    trunc = 0.0
    off = 0
    for b, (R, Z, cell, pbc) in enumerate(structs):
        n = len(R)
        _, g0 = energy_gradient(params, names, R, Z, cell, pbc, cfg)
        eye = np.eye(3)
        g_norm = float(torch.cat([g0[k].reshape(-1) for k in names]).norm())
        dF, t1 = directional(lambda x: energy_gradient(params, names, R + x, Z, cell, pbc, cfg)[1], u[off:off + n], g_norm)
        dS, t2 = directional(lambda x: energy_gradient(params, names, R @ (eye + x), Z, cell @ (eye + x), pbc, cfg)[1], w[b], g_norm)
        vol = abs(np.linalg.det(cell))
        for k in names:
            total[k] += float(gE[b, 0]) * g0[k]
            if dF is not None:
                total[k] -= dF[k]
            if dS is not None:
                total[k] += dS[k] / vol
        trunc = max(trunc, t1, t2 / vol)
        off += n
    # trunc: the largest |D(h) - Richardson| of a term, relative to the largest parameter gradient — what D(h) alone would be off by
    trunc /= max(float(g.norm()) for g in total.values())
    return dict(E=E.detach(), F=F.detach(), S=S.detach(), Et=Et, Ft=Ft, St=St, loss=float(loss.detach()), grads=total, trunc=trunc)


def batch(structs, device="cpu", dtype=torch.float64):
    """The periodic input dict of `structs` from the brute-force image neighbour list (fixed index arrays)."""
    R = np.concatenate([s[0] for s in structs])
    N = [len(s[0]) for s in structs]
    cell = np.stack([s[2] for s in structs])
    idx = P.brute_force(R, N, cell, np.stack([s[3] for s in structs]), P.CUTOFF)
    inputs = {k: torch.tensor(v, device=device) for k, v in idx.items()}
    inputs.update(R=torch.tensor(R, dtype=dtype, device=device), N=torch.tensor(N, device=device),
                  Z=torch.tensor(np.concatenate([s[1] for s in structs]), device=device).long(),
                  cell=torch.tensor(cell, dtype=dtype, device=device))
    return inputs


def trainable(model, params):
    """Names of the model's trainable parameters (all of them are leaves of the oracle)."""
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    assert set(names) <= set(params)
    return names


# ---------------------------------------------------------------------------- fp64 restatements of csrc/pbc_train.hip's launchers
def dist_vec_fwd(V):
    return torch.sqrt((V * V).sum(1))


def dist_vec_bwd(gD, V):
    return gD[:, None] * V / dist_vec_fwd(V)[:, None]


def dist_vec_jvp(V, tV):
    return (V * tV).sum(1) / dist_vec_fwd(V)


def angle_vec_fwd(V, red, exp):
    return cpu_kernels._angle_uv(-V[red.long()], -V[exp.long()])


def angle_vec_bwd(g, V, red, exp):
    with torch.enable_grad():
        u = (-V[red.long()]).detach().clone().requires_grad_(True)
        v = (-V[exp.long()]).detach().clone().requires_grad_(True)
        Gu, Gv = torch.autograd.grad(cpu_kernels._angle_uv(u, v), (u, v), g.detach())
    return Gu, Gv


def angle_vec_jvp(V, tV, red, exp):
    Gu, Gv = angle_vec_bwd(torch.ones(red.shape[0], dtype=V.dtype, device=V.device), V, red, exp)
    return -(Gu * tV[red.long()]).sum(1) - (Gv * tV[exp.long()]).sum(1)


def pbc_force_stress_adj(gF, gS, V, id_c, id_a, batch_seg, cell, scale=-1.0):
    gG = gF[id_a.long()] - gF[id_c.long()]
    if gS is not None:
        b = batch_seg.long()[id_a.long()]
        k = scale / torch.linalg.det(cell).abs()
        gG = gG + k[b][:, None] * torch.einsum("ei,eij->ej", V, gS[b])
    return gG


def edge_vectors(R, plan, cell):
    R = R.detach()
    cell = cell.detach().to(R.dtype)
    a, c = plan.id_a.idx32.long(), plan.id_c.idx32.long()
    shift = torch.einsum("ek,ekj->ej", plan.cell_offsets.to(R.dtype), cell[plan.batch_seg.idx32.long()[a]])
    return R[a] - (R[c] + shift)


def stress(V, G, plan, cell):
    b = plan.batch_seg.idx32.long()[plan.id_a.idx32.long()]
    S = torch.zeros((plan.n_mol, 3, 3), dtype=V.dtype).index_add(0, b, V[:, :, None] * G[:, None, :])
    return -S / torch.linalg.det(cell.detach().to(V.dtype)).abs()[:, None, None]


_K_NAMES = ["dist_vec_fwd", "dist_vec_bwd", "dist_vec_jvp", "angle_vec_fwd", "angle_vec_bwd", "angle_vec_jvp",
            "pbc_force_stress_adj"]
_PBC_NAMES = ["edge_vectors", "stress"]      # the wrappers of pbc.py that the training path calls and that load the library


@contextlib.contextmanager
def emulate():
    """cpu_kernels.emulate() + the launchers of the periodic training path (tests only)."""
    import gemnet_pytorch_amd.kernels as K
    import gemnet_pytorch_amd.pbc as PB
    saved = [(m, n, getattr(m, n)) for m, names in ((K, _K_NAMES), (PB, _PBC_NAMES)) for n in names]
    with cpu_kernels.emulate():
        try:
            for m, n, _ in saved:
                setattr(m, n, globals()[n])
            yield
        finally:
            for m, n, f in saved:
                setattr(m, n, f)
