"""Helpers of the tests of PADDED periodic training (training.periodic.PeriodicPaddedTrainStep): the trajectory of changing
positions, cells and image neighbour lists, a float64 restatement of the one-launch periodic loss (kernels.periodic_loss,
csrc/optim.hip: periodic_loss_kernel), and the context manager that swaps it in beside pbc_train_common.emulate().

Trajectory (`trajectory`): the recipe of tests/test_gpu_pbc_padded.py::trajectory restated — structures of tests/pbc_common.py,
per step R += N(0, 0.12), cell <- cell (1 + N(0, 0.004)), positions not wrapped, inputs rounded to float32 before any list is
built, no pair within 1e-5 A of the cutoff (float32 and float64 distances then give the same list)."""
import contextlib
import functools

import numpy as np
import torch

import pbc_common as P
import pbc_train_common as PT

BATCH = ("small", "triclinic", "slab", "cubic1")
FRAMES = 6
IDX_KEYS = ("id_c", "id_a", "id_swap", "id_undir", "cell_offsets", "id3_reduce_ca", "id3_expand_ba")


@functools.lru_cache(maxsize=None)
def trajectory(kinds=BATCH, steps=FRAMES):
    """-> (Z, N, pbc, frames): frames[s] = (R float32 (A,3), cell float32 (B,3,3), brute-force index dict of that frame)."""
    structs = [P.structure(k, seed=i) for i, k in enumerate(kinds)]
    R, Z, N, cell, pbc = P.arrays(structs)
    rs = np.random.RandomState(7)
    frames = []
    for _ in range(max(steps, FRAMES)):
        R32, c32 = R.astype(np.float32), cell.astype(np.float32)
        ref = P.brute_force(R32, N, c32, pbc, P.CUTOFF)
        for d in (-1e-5, 1e-5):
            other = P.brute_force(R32, N, c32, pbc, P.CUTOFF + d)
            assert all(np.array_equal(ref[k], other[k]) for k in ref), "a pair sits on the cutoff: change the recipe"
        frames.append((R32, c32, ref))
        R = R + rs.normal(0, 0.12, R.shape)
        cell = cell @ (np.eye(3) + rs.normal(0, 0.004, (3, 3)))
    assert len({sizes(f)[:2] for f in frames[:FRAMES]}) >= 3, "the (E, T) sizes must change along the trajectory"
    return Z, N, pbc, frames[:steps]


def sizes(frame):
    """(E, T, largest in-degree) of a frame's brute-force list."""
    return len(frame[2]["id_c"]), len(frame[2]["id3_reduce_ca"]), int(np.bincount(frame[2]["id_a"]).max())


def capacities(frames):
    """(e_cap, t_cap, in-degree bound, dummy groups) that hold every frame: the sizing of tests/test_gpu_pbc_padded.py."""
    e_cap = max(sizes(f)[0] for f in frames) // 4 * 4 + 8
    t_cap = max(sizes(f)[1] for f in frames) // 2 * 2 + 2
    deg = max(sizes(f)[2] for f in frames)
    return e_cap, t_cap, deg, groups_for(frames, e_cap, deg)


def groups_for(frames, e_cap, deg):
    """Dummy groups for the largest padding of the frames: a dummy atom takes both pad edges of a quad."""
    pad = max(e_cap - min(sizes(f)[0] for f in frames), 0)
    return max(1, -(-(-(-pad // 4)) // max(deg // 2, 1)))


def targets(n_mol, n_atoms, seed=5):
    """Fixed targets of magnitude 0.1 .. 1 away from zero (float32-representable): no |.| or norm of the loss sits at its kink
    for outputs of O(0.01)."""
    rs = np.random.RandomState(seed)
    draw = lambda *s: (rs.uniform(0.1, 1.0, s) * rs.choice([-1.0, 1.0], s)).astype(np.float32).astype(np.float64)   # noqa: E731
    return draw(n_mol, 1), draw(n_atoms, 3), draw(n_mol, 3, 3)


# ------------------------------------------------------------------------------- float64 restatement of kernels.periodic_loss
def periodic_loss(E, Et, F, Ft, w_e, w_f, S=None, St=None, w_s=0.0, mask=None, w_f_dev=None):
    """-> (loss (), gE, gF, gS or None) in the closed form of csrc/optim.hip (periodic_loss_kernel), in the operands' dtype:
    loss = w_e sum|E - Et| + w_f [* w_f_dev] sum_a m_a |F_a - Ft_a|_2 + w_s sum_b |S_b - St_b|_F; a cotangent is 0 where its norm
    is 0."""
    if w_f_dev is not None:
        w_f = w_f * w_f_dev
    m = torch.ones(F.shape[0], dtype=F.dtype, device=F.device) if mask is None else mask.to(F.dtype)
    dE, dF = E - Et, F - Ft
    nF = torch.sqrt((dF * dF).sum(1))
    loss = w_e * dE.abs().sum() + (w_f * m * nF)[m != 0].sum()
    gE = w_e * torch.sign(dE)
    sF = torch.where((m != 0) & (nF > 0), w_f * m / torch.where(nF > 0, nF, torch.ones_like(nF)), torch.zeros_like(nF))
    gF = sF[:, None] * dF
    gS = None
    if S is not None:
        dS = S - St
        nS = torch.sqrt((dS * dS).sum((1, 2)))
        loss = loss + w_s * nS.sum()
        sS = torch.where(nS > 0, w_s / torch.where(nS > 0, nS, torch.ones_like(nS)), torch.zeros_like(nS))
        gS = sS[:, None, None] * dS
    return loss, gE, gF, gS


@contextlib.contextmanager
def emulate(direct=False):
    """pbc_train_common.emulate() (`direct`: pbc_direct_train_common.emulate(), which layers on it) + the loss launcher."""
    import gemnet_pytorch_amd.kernels as K
    if direct:
        import pbc_direct_train_common as DT
        base = DT.emulate
    else:
        base = PT.emulate
    saved = K.periodic_loss
    with base():
        try:
            K.periodic_loss = periodic_loss
            yield
        finally:
            K.periodic_loss = saved


# --------------------------------------------------------------------------------------------------- the two steps, on any device
def frame_tensors(frame, device, dtype):
    R32, c32, ref = frame
    idx = {k: torch.tensor(np.asarray(ref[k]), device=device) for k in IDX_KEYS}
    return torch.tensor(R32, device=device).to(dtype), torch.tensor(c32, device=device), idx


def unpadded_inputs(Z, N, frame, device, dtype):
    """The input dict of the plain PeriodicTrainStep for one frame (brute-force list)."""
    R, cell, _ = frame_tensors(frame, device, dtype)
    idx = {k: torch.tensor(np.asarray(v), device=device) for k, v in frame[2].items()}       # (batch_seg included)
    return dict(Z=torch.tensor(Z, device=device).long(), N=torch.tensor(N, device=device), R=R, cell=cell.to(dtype), **idx)
