"""A stream of periodic 4-structure batches whose structure SIZES change from batch to batch (tests of the atom capacity of
padded.PaddedGraphRunner(a_cap=, cell=) / training.periodic.PeriodicPaddedTrainStep / pbc.PeriodicCapacityGraphBuilder).

Built from tests/pbc_common.py (`structure`, `_gas_structure`, `arrays`, `brute_force_fast`), positions and cells rounded to
float32 before any list is built, CUTOFF = 2.6:

  0  (small, triclinic, slab, cubic1)          10 atoms
  1  (cubic1, bcc_pert, thin, cubic1)           6 atoms: self-image edges, images up to |n| = 2
  2  (65-atom gas, slab, small, cubic1)        72 atoms = A_CAP: the 65-atom structure crosses the 64-lane partner loop of the
                                                pair search, the slab sits in another slot than in batch 0 (the pbc rows change)
  3  batch 0 again                              atoms that were real in batch 2 are fillers again

Asserted here, on the CPU, from the brute-force lists alone: no pair within 1e-5 A of the cutoff in any batch (float32 and
float64 distances then give the same list), at least three distinct values each of A, E and T, the smallest A below A_CAP / 2,
and every batch fits the capacities sized like pbc_padded_train_common.capacities over the whole stream."""
import functools

import numpy as np
import torch

import pbc_common as P
import pbc_padded_train_common as C

CUTOFF = P.CUTOFF
assert CUTOFF == 2.6
N_MOL = 4
IDX_KEYS = C.IDX_KEYS
GAS_SEED = 3
_KINDS = (("small", "triclinic", "slab", "cubic1"),
          ("cubic1", "bcc_pert", "thin", "cubic1"),
          ("gas65", "slab", "small", "cubic1"),
          ("small", "triclinic", "slab", "cubic1"))


def _struct(kind, seed):
    if kind == "gas65":
        return P._gas_structure(65, np.random.RandomState(GAS_SEED), (True, True, True))
    return P.structure(kind, seed=seed)


@functools.lru_cache(maxsize=None)
def stream():
    """-> list of batches: dict(R float32 (A,3), Z (A,), N list of 4, cell float32 (4,3,3), pbc bool (4,3), ref: the brute-force
    index dict of the float32-rounded batch)."""
    out = []
    for kinds in _KINDS:
        structs = [P.f32_round(_struct(k, seed=i)) for i, k in enumerate(kinds)]
        R, Z, N, cell, pbc = P.arrays(structs)
        assert P.cutoff_margin_ok(R, N, cell, pbc, CUTOFF), "a pair sits on the cutoff: change the seeds"
        ref = P.brute_force_fast(R, N, cell, pbc, CUTOFF)
        out.append(dict(R=R.astype(np.float32), Z=np.asarray(Z), N=list(N), cell=cell.astype(np.float32),
                        pbc=np.asarray(pbc, dtype=bool), ref=ref))
    return out


def frame(b):
    """A batch in the (R, cell, ref) form of pbc_padded_train_common's helpers (`sizes`, `capacities`, `frame_tensors`)."""
    return b["R"], b["cell"], b["ref"]


def sizes(b):
    """(E, T, largest in-degree) of a batch's brute-force list."""
    return C.sizes(frame(b))


A_CAP = max(len(b["Z"]) for b in stream())
CAPS = C.capacities([frame(b) for b in stream()])        # (e_cap, t_cap, in-degree bound, dummy groups)

assert [len(b["Z"]) for b in stream()][:3] == [10, 6, 72] and A_CAP == 72 and stream()[2]["N"][0] == 65
assert all(len(b["N"]) == N_MOL for b in stream())
assert len({len(b["Z"]) for b in stream()}) >= 3, "A must take three values"
assert len({sizes(b)[0] for b in stream()}) >= 3 and len({sizes(b)[1] for b in stream()}) >= 3, "E and T must take three values"
assert min(len(b["Z"]) for b in stream()) < A_CAP / 2
assert not np.array_equal(stream()[0]["pbc"], stream()[2]["pbc"]), "the slab must change its slot"
assert all(sizes(b)[0] <= CAPS[0] - 4 and sizes(b)[1] <= CAPS[1] and sizes(b)[2] <= CAPS[2] for b in stream())


def tensors(b, device, dtype=torch.float32):
    """-> R (A,3) dtype, Z (A,) int64, N (4,) int64, cell (4,3,3) float32, idx: the brute-force lists (IDX_KEYS), on `device`."""
    R, cell, idx = C.frame_tensors(frame(b), device, dtype)
    return R, torch.tensor(b["Z"], device=device).long(), torch.tensor(b["N"], device=device), cell, idx


def unpadded_inputs(b, device, dtype):
    """The input dict of the plain PeriodicTrainStep / the eager model for one batch (brute-force list, batch_seg included)."""
    return C.unpadded_inputs(b["Z"], b["N"], frame(b), device, dtype)


def targets(b, seed=5):
    """Fixed targets for one batch (pbc_padded_train_common.targets): E (4,1), F (A,3), S (4,3,3) float64."""
    return C.targets(N_MOL, len(b["Z"]), seed=seed + len(b["Z"]))
