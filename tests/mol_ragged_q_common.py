"""The stream of tests/mol_ragged_common.py for quadruplet models: the same four 4-molecule batches (11, 6, 72 = a_cap and again 11
atoms; CUTOFF = 2.6) with an interaction cutoff INT_CUTOFF = 4.0 and all sixteen index arrays of a GemNet-Q (tests of
index_device.DeviceCapacityQuadGraphBuilder, gn_index_gpu_padded_qv, Trainer.enable_padded_eval(quad_caps=)).  Data and CPU
assertions only.

  batch    atoms   E     T      Eint    I       Q
  0, 3     11      28    66     28      94      120
  1        6       2     0      4       2       0       the 3.5 A pair is an interaction edge without an embedding edge; a batch
                                                        without triplets or quadruplets
  2        72      462   3 464  1 318   10 292  72 182  a 66-atom molecule (= N_MAX)

The lists are the oracle's (oracle.index_oracle.build_indices: the reference's construction in numpy, canonical order).  Asserted
here, on the CPU, from those lists and the float64 pair distances alone: the sizes above, no pair within 1e-5 A of either cutoff
(float32 and float64 distances then give the same lists), and every batch fits the capacities CAPS sized over the whole stream
(pbc_q_padded_common.caps_for: the largest count of each family plus a little) by the padding rules of
padded._check_quad_padding and the in-degree bound of the dummy atoms."""
import functools

import numpy as np
import torch

import mol_ragged_common as G
import pbc_q_padded_common as QC
from gemnet_pytorch_amd.padded import _check_quad_padding
from oracle import index_oracle as IO

CUTOFF, INT_CUTOFF = G.CUTOFF, 4.0
N_MOL, N_MAX, A_CAP = G.N_MOL, G.N_MAX, G.A_CAP
KEYS = QC.T_KEYS + QC.Q_KEYS                     # the sixteen arrays the model reads
FAMILY = {k: QC.FAMILY[k] for k in KEYS}         # 0 edges, 1 triplets, 2 interaction edges, 3 intermediate triplets, 4 quadruplets
SIZES = ((28, 66, 28, 94, 120), (2, 0, 4, 2, 0), (462, 3464, 1318, 10292, 72182), (28, 66, 28, 94, 120))


@functools.lru_cache(maxsize=None)
def stream():
    """-> list of batches: dict(R float32 (A,3), Z int64 (A,), N list of 4, ref: the oracle's index dict)."""
    out = []
    for b in G.stream():
        d = np.concatenate(G.pair_distances(b["R"], b["N"]))
        for c in (CUTOFF, INT_CUTOFF):
            assert np.abs(d - c).min() > 1e-5, "a pair sits on a cutoff: change the seeds"
        out.append(dict(R=b["R"], Z=b["Z"], N=b["N"], ref=IO.build_indices(b["R"], np.array(b["N"]), CUTOFF, INT_CUTOFF, False)))
    return out


def sizes(b):
    """(E, T, Eint, I, Q) of a batch's lists."""
    return QC.sizes(b["ref"])


def capacities(batches):
    """((e_cap, t_cap, eint_cap, i_cap, q_cap), in-degree bound, dummy groups) that hold every batch."""
    n = tuple(max(sizes(b)[k] for b in batches) for k in range(5))
    deg = max(QC.in_degree(b["ref"]) for b in batches)
    caps = QC.caps_for(n)
    return caps, deg, QC.groups_for(caps[0], min(sizes(b)[0] for b in batches), deg)


def fits(b, caps, deg, groups):
    """Does the batch fit with valid padding?  The rules of padded.PaddedGraphRunner._fill, restated."""
    pad = tuple(c - n for c, n in zip(caps, sizes(b)))
    if min(pad) < 0 or pad[0] % 2 or pad[1] % 2:
        return False
    try:
        _check_quad_padding(*pad)
    except ValueError:
        return False
    return 2 * -(-(-(-pad[0] // 6)) // groups) <= max(deg, 2)


CAPS, DEG, GROUPS = capacities(stream())

assert tuple(sizes(b) for b in stream()) == SIZES, [sizes(b) for b in stream()]
assert all(len(b["ref"]["id4_reduce_intm_ca"]) == sizes(b)[3] for b in stream())
assert all(fits(b, CAPS, DEG, GROUPS) for b in stream())
assert DEG <= N_MAX - 1


def tensors(b, device, dtype=torch.float32):
    """-> R (A,3) dtype, Z (A,) int64, N (4,) int64, idx: the oracle's lists (KEYS), on `device`."""
    idx = {k: torch.tensor(np.asarray(b["ref"][k]), device=device) for k in KEYS}
    return (torch.tensor(b["R"], device=device).to(dtype), torch.tensor(b["Z"], device=device).long(),
            torch.tensor(b["N"], device=device), idx)


def targets(b, seed=5):
    return G.targets(b, seed)
