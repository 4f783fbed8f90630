"""Test infrastructure of periodic GemNet-Q TRAINING (fp64, CPU): the gradient oracle of tests/pbc_train_common.py restated on the
quadruplet cluster oracle of tests/pbc_q_common.py, its stored form (tests/golden/pbc_q_train.npz + shards, written by
tests/golden/make_pbc_q_train_golden.py: the oracle costs ~100 s of host time), fp64 restatements of the launchers of
csrc/pbc_quad_train.hip and of the wrappers of pbc.py that call the library directly, and the context manager that swaps them in
on top of pbc_train_common.emulate().

Gradient oracle: see pbc_train_common — the same Richardson directional derivatives of grad_theta E_b and the same `directional`
condition (a property of the oracle), with E_b the cluster energy of `pbc_q_common.cluster_energy` (radius Q.RADIUS, the index
arrays of IO.build_indices(..., cutoff, int_cutoff, False))."""
import contextlib
import glob
import os

import numpy as np
import torch

import cpu_kernels
import pbc_common as P
import pbc_q_common as Q
import pbc_train_common as PT
from oracle import gemnet_oracle as GO
from oracle import index_oracle as IO

# the widths of pbc_train_common.CFG_WIDE + the quadruplet widths of the angle form (kernels.bil_ang_train_supported(49, 32, 32)):
# one block, 546 822 parameters in 45 tensors; GemNet._train2_widths_ok holds.  The narrow Q.CFG_Q is the composite case.
CFG_QW = dict(PT.CFG_WIDE, triplets_only=False, int_cutoff=Q.INT_CUTOFF, emb_size_quad=32, emb_size_sbf=32, emb_size_bil_quad=32)
CFGS = {"qw": CFG_QW, "q": Q.CFG_Q}
RHO_FORCE, RHO_STRESS = PT.RHO_FORCE, PT.RHO_STRESS
# batch A: the four structures of the GemNet-T training tests ('slab' has a self-image interaction edge at exactly int_cutoff,
# envelope weight zero: Q.cutoff_margins_ok does not hold for it and is not asked); batch B: exactly planar and exactly collinear
# quadruplets.  ('thin' meets the oracle's condition too, but |g| = 1.4e3 at E = -77.6 at these widths: no gradient test on it.)
BATCHES = {"A": PT.KINDS, "B": ["bcc_pert"]}
STORED = {"qw": ["A", "B"], "q": ["A"]}        # what tests/golden/pbc_q_train.npz holds: configuration -> batches
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pbc_q_train.npz")
SHARD = 110000          # float64 numbers per shard file: 880 kB


def structures(tag):
    return PT.structures() if tag == "A" else [P.structure(k) for k in BATCHES[tag]]


def make_params(cfg, seed=3):
    return Q.make_params(cfg, seed)


# ------------------------------------------------------------------------------------------------------------ gradient oracle
def _cluster_inputs(R, Z, cell, pbc, cfg):
    Rc, Zc = P.cluster(R, Z, cell, pbc, Q.RADIUS)
    n = len(R)
    idx = IO.build_indices(Rc, np.array([len(Rc)]), cfg["cutoff"], cfg["int_cutoff"], False)
    inputs = {k: torch.tensor(v) for k, v in idx.items()}
    bs = np.zeros(len(Rc), np.int64)
    bs[n:] = 1
    inputs.update(Z=torch.tensor(Zc).long(), R=torch.tensor(Rc), batch_seg=torch.tensor(bs), N=torch.tensor([n, len(Rc) - n]))
    return inputs


def energy_gradient(params, names, R, Z, cell, pbc, cfg):
    """grad_theta of the periodic energy of one structure (one backward through the cluster oracle) -> (E, {name: gradient})."""
    leaves = {k: v.detach().clone().requires_grad_(k in names) for k, v in params.items()}
    E, _ = GO.forward(cfg, leaves, _cluster_inputs(R, Z, cell, pbc, cfg), need_forces=False)
    grads = torch.autograd.grad(E[0, 0], [leaves[n] for n in names], allow_unused=True)
    return float(E[0, 0].detach()), {n: (torch.zeros_like(leaves[n]) if g is None else g) for n, g in zip(names, grads)}


def efs(params, cfg, struct):
    """E (float), F (n,3), S (3,3) of one structure: the cluster energy and its central differences."""
    R, Z, cell, pbc = struct
    F, S = Q.fd_forces_stress(params, R, Z, cell, pbc, cfg)
    return Q.cluster_energy(params, R, Z, cell, pbc, cfg), F, S


def loss_terms(Es, Fs, Ss, structs, rho_force=RHO_FORCE, rho_stress=RHO_STRESS):
    """The oracle's outputs of a batch -> dict(E, F, S, Et, Ft, St, loss) and the cotangents (gE (B,1), u (A,3), w (B,3,3)) of the
    loss at them (targets: the outputs + pbc_train_common.offsets)."""
    E = torch.tensor(Es, dtype=torch.float64)[:, None].requires_grad_(True)
    F = torch.tensor(np.concatenate(Fs)).requires_grad_(True)
    S = torch.tensor(np.stack(Ss)).requires_grad_(True)
    oE, oF, oS = PT.offsets(structs)
    Et, Ft, St = E.detach() + torch.tensor(oE), F.detach() + torch.tensor(oF), S.detach() + torch.tensor(oS)
    loss = PT.loss_fp64(E, F, S, Et, Ft, St, rho_force, rho_stress)
    cot = tuple(t.numpy() for t in torch.autograd.grad(loss, (E, F, S)))
    return dict(E=E.detach(), F=F.detach(), S=S.detach(), Et=Et, Ft=Ft, St=St, loss=float(loss.detach())), cot


def contribution(params, cfg, names, struct, gE_b, u_b, w_b):
    """The term of one structure in grad_theta L for its cotangents gE_b (float), u_b (n,3), w_b (3,3)
    -> ({name: tensor}, |D(h) - Richardson| of its worst term)."""
    R, Z, cell, pbc = struct
    _, g0 = energy_gradient(params, names, R, Z, cell, pbc, cfg)
    eye = np.eye(3)
    g_norm = float(torch.cat([g0[k].reshape(-1) for k in names]).norm())
    dF, t1 = PT.directional(lambda x: energy_gradient(params, names, R + x, Z, cell, pbc, cfg)[1], u_b, g_norm)
    dS, t2 = PT.directional(lambda x: energy_gradient(params, names, R @ (eye + x), Z, cell @ (eye + x), pbc, cfg)[1], w_b, g_norm)
    vol = abs(np.linalg.det(cell))
    out = {}
    for k in names:
        out[k] = float(gE_b) * g0[k]
        if dF is not None:
            out[k] = out[k] - dF[k]
        if dS is not None:
            out[k] = out[k] + dS[k] / vol
    return out, max(t1, t2 / vol)


def oracle(params, cfg, structs, names, rho_force=RHO_FORCE, rho_stress=RHO_STRESS):
    """pbc_train_common.oracle for a quadruplet model, + `parts`: the contribution of every structure."""
    out, (gE, u, w) = loss_terms(*zip(*[efs(params, cfg, s) for s in structs]), structs, rho_force, rho_stress)
    parts, trunc, off = [], 0.0, 0
    for b, s in enumerate(structs):
        n = len(s[0])
        g, t = contribution(params, cfg, names, s, gE[b, 0], u[off:off + n], w[b])
        parts.append(g)
        trunc = max(trunc, t)
        off += n
    total = {k: sum(p[k] for p in parts) for k in names}
    return dict(out, grads=total, parts=parts, trunc=trunc / max(float(g.norm()) for g in total.values()))


# ------------------------------------------------------------------------------------------------------------- stored oracle
# pbc_q_train.npz: per batch tag E, F, S, Et, Ft, St, loss, trunc; the parameter names and sizes.  The gradients — batch A, the
# contribution of 'slab' to it, batch B — are 3 x 546 822 float64 numbers, one flat array (names sorted, tensors flattened) cut into
# shard files pbc_q_train.g<NN>.npy of SHARD numbers each.
VECTORS = ["A", "A.slab", "B"]


def prefix(cfg, tag):
    """Key prefix of a stored batch: the tag alone for CFG_QW, '<configuration>.<tag>' otherwise."""
    return tag if cfg == "qw" else f"{cfg}.{tag}"


def flatten(grads, names):
    return np.concatenate([np.asarray(grads[n], np.float64).reshape(-1) for n in sorted(names)])


def load_golden():
    """-> {tag: dict(E, F, S, Et, Ft, St, loss, trunc, grads {name: tensor})} for the batch tags of CFG_QW and 'q.A' (the narrow
    Q.CFG_Q on batch A), + 'A.slab': {name: tensor}."""
    z = np.load(GOLDEN)
    terms = lambda pre: dict({k: torch.tensor(z[f"{pre}.{k}"]) for k in ("E", "F", "S", "Et", "Ft", "St")},       # noqa: E731
                             loss=float(z[f"{pre}.loss"]), trunc=float(z[f"{pre}.trunc"]))
    names, sizes = [str(n) for n in z["names"]], z["sizes"]
    shapes = [tuple(int(v) for v in z[f"shape.{n}"]) for n in names]
    flat = np.concatenate([np.load(f) for f in sorted(glob.glob(GOLDEN[:-4] + ".g*.npy"))])
    total = int(sizes.sum())
    assert flat.shape == (len(VECTORS) * total,) and flat.dtype == np.float64
    out = {}
    for i, v in enumerate(VECTORS):
        vec, off, grads = flat[i * total:(i + 1) * total], 0, {}
        for n, s, shp in zip(names, sizes, shapes):
            grads[n] = torch.tensor(vec[off:off + s].reshape(shp))
            off += int(s)
        if v in BATCHES:
            out[v] = dict(terms(v), grads=grads)
        else:
            out[v] = grads
    for cfg, tags in STORED.items():
        for tag in tags if cfg != "qw" else ():
            pre = prefix(cfg, tag)
            out[pre] = dict(terms(pre), grads={k[len(pre) + 6:]: torch.tensor(z[k]) for k in z.files if k.startswith(pre + ".grad.")})
    return out


def batch(structs, device="cpu", dtype=torch.float64):
    """The periodic GemNet-Q input dict of `structs` from the brute-force image quadruplet list (fixed fp64 index arrays)."""
    R, Z, N, cell, pbc = P.arrays(structs)
    idx = Q.brute_force_q(R, N, cell, pbc, Q.CUTOFF, Q.INT_CUTOFF)
    inputs = {k: torch.tensor(v, device=device) for k, v in idx.items()}
    inputs.update(R=torch.tensor(R, dtype=dtype, device=device), N=torch.tensor(N, device=device),
                  Z=torch.tensor(Z, device=device).long(), cell=torch.tensor(cell, dtype=dtype, device=device))
    return inputs


# ------------------------------------------------------------------ fp64 restatements of csrc/pbc_quad_train.hip's launchers
def angle_vec2_fwd(U, iu, W, iw):
    return cpu_kernels._angle_uv(U[iu.long()], -W[iw.long()])


def angle_vec2_bwd(g, U, iu, W, iw):
    with torch.enable_grad():
        u = U[iu.long()].detach().clone().requires_grad_(True)
        w = W[iw.long()].detach().clone().requires_grad_(True)
        GU, GW = torch.autograd.grad(cpu_kernels._angle_uv(u, -w), (u, w), g.detach())
    return GU, GW


def angle_vec2_jvp(U, iu, W, iw, tU, tW):
    GU, GW = angle_vec2_bwd(torch.ones(iu.shape[0], dtype=U.dtype), U, iu, W, iw)
    out = torch.zeros(iu.shape[0], dtype=U.dtype)
    if tU is not None:
        out = out + (GU * tU[iu.long()]).sum(1)
    if tW is not None:
        out = out + (GW * tW[iw.long()]).sum(1)
    return out


# the relative clamp decisions of csrc/quad_math.h: stated once, in tests/cpu_kernels.py (the molecular launchers take them too)
REL_SIN2, _sq, _rej = cpu_kernels.REL_SIN2, cpu_kernels._sq, cpu_kernels._rej
quad_decisions, quad_angles_rel = cpu_kernels.quad_decisions, cpu_kernels.quad_angles_rel


def quad_vectors(V, Vint, q_ca, q_db, q_abd, intm_ab):
    return -V[q_ca.long()], -Vint[intm_ab.long()[q_abd.long()]], -V[q_db.long()]


def quad_angles_vec_fwd_k(V, Vint, q_ca, q_db, q_abd, intm_ab):
    return cpu_kernels.angle_form(*quad_angles_rel(*quad_vectors(V, Vint, q_ca, q_db, q_abd, intm_ab)))


def quad_angles_vec_bwd_k(g_ang, V, Vint, q_ca, q_db, q_abd, intm_ab):
    """-> Gc (Q,3), Gbd (Q,8): the per-quadruplet rows of gn_quad_angles_vec_bwd_f32."""
    with torch.enable_grad():
        uac, uab, ubd = (x.detach().clone().requires_grad_(True) for x in quad_vectors(V, Vint, q_ca, q_db, q_abd, intm_ab))
        phi, th = quad_angles_rel(uac, uab, ubd)
        g_ac, g_ab, g_bd = torch.autograd.grad((g_ang[:, 0] * phi + g_ang[:, 1] * th).sum(), (uac, uab, ubd), allow_unused=True)
    z = lambda g: torch.zeros_like(uac) if g is None else g       # noqa: E731
    Gbd = torch.zeros((uac.shape[0], 8), dtype=V.dtype)
    Gbd[:, 0:3], Gbd[:, 4:7] = -z(g_ab), -z(g_bd)
    return -z(g_ac), Gbd


def quad_angles_vec_jvp(V, Vint, tV, tVint, q_ca, q_db, q_abd, intm_ab):
    Q_ = q_ca.shape[0]
    out = torch.zeros((Q_, 4), dtype=V.dtype)
    k = intm_ab.long()[q_abd.long()]
    for col in (0, 1):
        g = torch.zeros((Q_, 4), dtype=V.dtype)
        g[:, col] = 1.0
        Gc, Gbd = quad_angles_vec_bwd_k(g, V, Vint, q_ca, q_db, q_abd, intm_ab)
        if tV is not None:
            out[:, col] += (Gc * tV[q_ca.long()]).sum(1) + (Gbd[:, 4:7] * tV[q_db.long()]).sum(1)
        if tVint is not None:
            out[:, col] += (Gbd[:, 0:3] * tVint[k]).sum(1)
    return out


# ------------------------------------------------------------------- ... and of the wrappers of pbc.py that load the library
def _qidx(plan):
    import gemnet_pytorch_amd.pbc as PB
    return PB.quad_index(plan)


def quad_angles_vec_fwd(V, Vint, plan):
    return quad_angles_vec_fwd_k(V, Vint, *_qidx(plan))


def quad_angles_vec_adjoint(g_ang, V, Vint, plan):
    import gemnet_pytorch_amd.pbc as PB
    return PB.quad_reduce(*quad_angles_vec_bwd_k(g_ang, V, Vint, *_qidx(plan)), plan)


def int_edge_vectors(R, plan, cell):
    R = R.detach()
    cell = cell.detach().to(R.dtype)
    a, b = plan.int_a.idx32.long(), plan.int_b.idx32.long()
    shift = torch.einsum("ek,ekj->ej", plan.int_cell_offsets.to(R.dtype), cell[plan.batch_seg.idx32.long()[a]])
    return R[a] - (R[b] + shift)


def stress_q(V, G, Vint, Gint, plan, cell):
    b = plan.batch_seg.idx32.long()[plan.int_a.idx32.long()]
    Si = torch.zeros((plan.n_mol, 3, 3), dtype=V.dtype).index_add(0, b, Vint[:, :, None] * Gint[:, None, :])
    return PT.stress(V, G, plan, cell) - Si / torch.linalg.det(cell.detach().to(V.dtype)).abs()[:, None, None]


def force_stress_q_ref(G, Gint, V, Vint, id_c, id_a, int_b, int_a, batch_seg, cell, n_atoms):
    """ATen composite of pbc.forces_q + pbc.stress_q, differentiable in (G, Gint): the reference of the two-set adjoint."""
    F = (torch.zeros(n_atoms, 3, dtype=G.dtype).index_add(0, id_a.long(), G).index_add(0, id_c.long(), -G)
         .index_add(0, int_a.long(), Gint).index_add(0, int_b.long(), -Gint))
    B = cell.shape[0]
    S = (torch.zeros(B, 3, 3, dtype=G.dtype).index_add(0, batch_seg.long()[id_a.long()], V[:, :, None] * G[:, None, :])
         .index_add(0, batch_seg.long()[int_a.long()], Vint[:, :, None] * Gint[:, None, :]))
    return F, -S / torch.linalg.det(cell).abs()[:, None, None]


_K_NAMES = ["angle_vec2_fwd", "angle_vec2_bwd", "angle_vec2_jvp", "quad_angles_vec_jvp"]
_PBC_NAMES = ["quad_angles_vec_fwd", "quad_angles_vec_adjoint", "int_edge_vectors", "stress_q"]
COUNTED = PT._K_NAMES + _K_NAMES


@contextlib.contextmanager
def emulate():
    """pbc_train_common.emulate() + the launchers of the periodic GemNet-Q training path (tests only)."""
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
