"""A stream of molecular 4-molecule batches whose molecule SIZES change from batch to batch (tests of the atom capacity of a
molecular padded.PaddedGraphRunner(a_cap=) with the lists built inside the replay: index_device.DeviceCapacityGraphBuilder,
gn_index_gpu_layout, gn_index_gpu_padded_tv, Trainer.enable_padded_eval).  Data and CPU assertions only.

Molecules: gemnet_pytorch_amd.synthetic.make_molecule (atoms uniform in a cube, no pair below 0.9 A) plus two hand-made
two-atom molecules; positions are float32 before any list is built, CUTOFF = 2.6 (the cutoff of pbc_common.CFG):

  0  (3, 1, 5, 2)     11 atoms: a one-atom molecule — degree 0, a 1 x 1 adjacency block
  1  (2, 2, 1, 1)      6 atoms: the second two-atom molecule has its atoms 3.5 A apart — a molecule with no edge
  2  (66, 1, 3, 2)    72 atoms = A_CAP: 66 atoms = N_MAX; an atom of that molecule has 65 candidate partners, so the 64-lane loop
                      of the triplet writer takes a second round, and its 66^2 = 4 356 pairs span 18 blocks of the adjacency grid
  3  batch 0 again    atoms that were real in batch 2 are fillers again

`brute_force` is the reference list: float64 distances, the canonical order of include/gemnet_hip.h written out in plain loops.
Asserted here, on the CPU, from the brute-force lists alone: no pair within 1e-5 A of the cutoff in any batch (float32 and
float64 distances then give the same list), at least three distinct values each of A, E and T, the smallest A below A_CAP / 2,
a mean degree between 4 and 12 inside the 66-atom molecule, and every batch fits the capacities sized like
pbc_padded_train_common.capacities over the whole stream."""
import functools

import numpy as np
import torch

import pbc_padded_train_common as C
from gemnet_pytorch_amd.synthetic import make_molecule

CUTOFF = 2.6
N_MOL = 4
N_MAX = 66
IDX_KEYS = ("id_c", "id_a", "id_swap", "id_undir", "id3_reduce_ca", "id3_expand_ba")
BIG_SEED, BIG_BOX = 7, 7.6
_SIZES = ((3, 1, 5, 2), (2, 2, 1, 1), (66, 1, 3, 2), (3, 1, 5, 2))


def _molecule(n, seed):
    m = make_molecule(n, BIG_SEED, box=BIG_BOX) if n == N_MAX else make_molecule(n, seed, box=2.2)
    return m["R"].astype(np.float32), m["Z"].astype(np.int64)


def _pair(d):
    return np.array([[0.0, 0.0, 0.0], [d, 0.0, 0.0]], np.float32), np.array([6, 8], np.int64)


def pair_distances(R, N):
    """Per molecule: the float64 distances of its atom pairs (i < j)."""
    out, a0 = [], 0
    for n in N:
        r = np.asarray(R[a0:a0 + n], np.float64)
        d = np.sqrt(((r[:, None] - r[None]) ** 2).sum(-1))
        out.append(d[np.triu_indices(n, 1)])
        a0 += n
    return out


def brute_force(R, N, cutoff):
    """The index arrays of a molecular batch in the canonical order, float64 distances: edges = pairs (t < s) of one molecule
    within the cutoff, ordered by (t, s), edge e = (s -> t) and e + H its reverse; triplets ordered by reduce edge (c -> a), the
    expand edges (b -> a), b != c, in ascending edge id (sources above a first, then those below)."""
    R = np.asarray(R, np.float64)
    pairs, a0 = [], 0
    for n in N:
        for t in range(a0, a0 + n):
            for s in range(t + 1, a0 + n):
                if np.sqrt(((R[t] - R[s]) ** 2).sum()) <= cutoff:
                    pairs.append((t, s))
        a0 += n
    H = len(pairs)
    id_a = np.array([t for t, _ in pairs] + [s for _, s in pairs], np.int64)
    id_c = np.array([s for _, s in pairs] + [t for t, _ in pairs], np.int64)
    half = np.arange(H, dtype=np.int64)
    edge = {(int(a), int(c)): e for e, (a, c) in enumerate(zip(id_a, id_c))}       # (target, source) -> edge id
    nbrs = {}
    for a, c in edge:
        nbrs.setdefault(a, []).append(c)
    red, exp = [], []
    for r in range(2 * H):
        a, c = int(id_a[r]), int(id_c[r])
        srcs = sorted(nbrs[a])
        for b in [b for b in srcs if b > a] + [b for b in srcs if b < a]:
            if b != c:
                red.append(r)
                exp.append(edge[(a, b)])
    return dict(id_c=id_c, id_a=id_a, id_swap=np.concatenate([half + H, half]), id_undir=np.concatenate([half, half]),
                id3_reduce_ca=np.array(red, np.int64), id3_expand_ba=np.array(exp, np.int64))


@functools.lru_cache(maxsize=None)
def stream():
    """-> list of batches: dict(R float32 (A,3), Z int64 (A,), N list of 4, ref: the brute-force index dict)."""
    out = []
    for s, sizes in enumerate(_SIZES):
        mols = [_molecule(n, 40 + 10 * (s % 3) + slot) for slot, n in enumerate(sizes)]
        if s == 1:
            mols[0], mols[1] = _pair(1.1), _pair(3.5)
        R = np.concatenate([m[0] for m in mols]).astype(np.float32)
        Z = np.concatenate([m[1] for m in mols])
        d = np.concatenate(pair_distances(R, sizes))
        assert not len(d) or np.abs(d - CUTOFF).min() > 1e-5, "a pair sits on the cutoff: change the seeds"
        out.append(dict(R=R, Z=Z, N=list(sizes), ref=brute_force(R, sizes, CUTOFF)))
    return out


def frame(b):
    """A batch in the (R, cell, ref) form of pbc_padded_train_common's helpers (`sizes`, `capacities`)."""
    return b["R"], None, b["ref"]


def sizes(b):
    """(E, T, largest in-degree) of a batch's brute-force list."""
    return C.sizes(frame(b))


A_CAP = max(len(b["Z"]) for b in stream())
CAPS = C.capacities([frame(b) for b in stream()])        # (e_cap, t_cap, in-degree bound, dummy groups)

assert [len(b["Z"]) for b in stream()] == [11, 6, 72, 11] and A_CAP == 72
assert all(len(b["N"]) == N_MOL and max(b["N"]) <= N_MAX for b in stream()) and stream()[2]["N"][0] == N_MAX
assert np.array_equal(stream()[0]["R"], stream()[3]["R"])
assert len({len(b["Z"]) for b in stream()}) >= 3, "A must take three values"
assert len({sizes(b)[0] for b in stream()}) >= 3 and len({sizes(b)[1] for b in stream()}) >= 3, "E and T must take three values"
assert min(len(b["Z"]) for b in stream()) < A_CAP / 2
assert pair_distances(stream()[1]["R"], stream()[1]["N"])[1][0] > CUTOFF, "the second molecule of batch 1 has no edge"
_deg66 = np.bincount(stream()[2]["ref"]["id_a"], minlength=72)[:N_MAX]
assert 4 <= _deg66.mean() <= 12, _deg66.mean()
assert all(sizes(b)[0] <= CAPS[0] - 4 and sizes(b)[1] <= CAPS[1] and sizes(b)[2] <= CAPS[2] for b in stream())


def tensors(b, device, dtype=torch.float32):
    """-> R (A,3) dtype, Z (A,) int64, N (4,) int64, idx: the brute-force lists (IDX_KEYS), on `device`."""
    idx = {k: torch.tensor(np.asarray(b["ref"][k]), device=device) for k in IDX_KEYS}
    return (torch.tensor(b["R"], device=device).to(dtype), torch.tensor(b["Z"], device=device).long(),
            torch.tensor(b["N"], device=device), idx)


def targets(b, seed=5):
    """Fixed targets for one batch (pbc_padded_train_common.targets): E (4,1), F (A,3) float64."""
    return C.targets(N_MOL, len(b["Z"]), seed=seed + len(b["Z"]))[:2]
