"""Shared by tests/test_pbc_q_padded_cpu.py and tests/test_gpu_pbc_q_padded.py: periodic GemNet-Q in padded captured steps.

Trajectory (`trajectory`): structures of tests/pbc_common.py, per step R += N(0, 0.12), cell <- cell (1 + N(0, 0.004)) from
RandomState(7), 12 recorded steps, positions not wrapped, inputs rounded to float32 before any list is built, lists from the
brute force of tests/pbc_q_common.py.  `prestep`: one such step is applied before the first recorded one — the untouched 'slab'
has a lattice vector of exactly 3.0 = INT_CUTOFF, a self-image ON the cutoff.  The helper asserts on the CPU (fp64) that no pair
sits within 1e-5 A of either cutoff — float32 and float64 distances then give the same arrays and every comparison can be exact
— that each of the five counts takes at least four values and that an atom leaves its cell."""
import functools

import numpy as np

import pbc_common as P
import pbc_q_common as Q

STEPS = 12
BATCH = ("small", "triclinic", "slab", "bcc_pert")
# arguments of `trajectory`: the batch (one step before the first recorded one), and 'thin' alone from its unperturbed first
# step (images up to |n| = 2; its edge count takes three values)
TRAJ_BATCH, TRAJ_THIN = (BATCH, True, 4), (("thin",), False, 3)
T_KEYS = ("id_c", "id_a", "id_swap", "id_undir", "id3_reduce_ca", "id3_expand_ba")
Q_KEYS = ("id4_int_a", "id4_int_b", "id4_reduce_intm_ca", "id4_expand_intm_db", "id4_reduce_intm_ab", "id4_expand_intm_ab",
          "id4_reduce_ca", "id4_expand_db", "id4_reduce_cab", "id4_expand_abd")
OFF_KEYS = ("cell_offsets", "int_cell_offsets")
IDX_KEYS = T_KEYS + Q_KEYS + OFF_KEYS               # the eighteen arrays the model reads
# capacity family of every array: 0 edges, 1 triplets, 2 interaction edges, 3 intermediate triplets, 4 quadruplets
FAMILY = dict({k: 0 for k in T_KEYS[:4]}, id3_reduce_ca=1, id3_expand_ba=1, id4_int_a=2, id4_int_b=2, id4_reduce_intm_ca=3,
              id4_expand_intm_db=3, id4_reduce_intm_ab=3, id4_expand_intm_ab=3, id4_reduce_ca=4, id4_expand_db=4,
              id4_reduce_cab=4, id4_expand_abd=4, cell_offsets=0, int_cell_offsets=2)


def sizes(idx):
    """(E, T, Eint, I, Q) of an index dict."""
    return (len(idx["id_c"]), len(idx["id3_reduce_ca"]), len(idx["id4_int_a"]), len(idx["id4_expand_intm_db"]),
            len(idx["id4_reduce_ca"]))


def in_degree(idx):
    return int(np.bincount(np.asarray(idx["id_a"])).max()) if len(idx["id_a"]) else 0


@functools.lru_cache(maxsize=None)
def trajectory(kinds, prestep=True, distinct=4):
    """-> (Z, N, pbc, steps): steps[s] = (R float32 (A,3), cell float32 (B,3,3), brute-force index dict of that step).
    `distinct`: values each of the five counts must take along the trajectory (single small structures: fewer)."""
    structs = [P.structure(k, seed=i) for i, k in enumerate(kinds)]
    R, Z, N, cell, pbc = P.arrays(structs)
    rs = np.random.RandomState(7)

    def move(R, cell):
        R = R + rs.normal(0, 0.12, R.shape)
        return R, cell @ (np.eye(3) + rs.normal(0, 0.004, (3, 3)))

    if prestep:
        R, cell = move(R, cell)
    steps, outside = [], 0
    for _ in range(STEPS):
        R32, c32 = R.astype(np.float32), cell.astype(np.float32)
        assert Q.cutoff_margins_ok(R32, N, c32, pbc), "a pair sits on a cutoff: change the recipe"
        ref = Q.brute_force_q(R32, N, c32, pbc)
        off = 0
        for b, n in enumerate(N):
            f = R32[off:off + n].astype(np.float64) @ np.linalg.inv(c32[b].astype(np.float64))
            outside = max(outside, int(((f < 0) | (f >= 1))[:, pbc[b]].any(axis=1).sum()))
            off += n
        steps.append((R32, c32, ref))
        R, cell = move(R, cell)
    for k, name in enumerate(("edge", "triplet", "interaction-edge", "intermediate-triplet", "quadruplet")):
        assert len({sizes(s[2])[k] for s in steps}) >= distinct, f"the {name} count must change along the trajectory"
    assert outside >= 1, "an atom must leave the unit cell"
    return Z, N, pbc, steps


def max_sizes(steps):
    """Per family the largest count of the trajectory, and the largest in-degree."""
    return tuple(max(sizes(s[2])[k] for s in steps) for k in range(5)), max(in_degree(s[2]) for s in steps)


def caps_for(n, head=1.0, slack=(12, 2, 4, 4, 4)):
    """Capacities (e_cap, t_cap, eint_cap, i_cap, q_cap) for counts n: `head` x the count plus a little, edges in units that
    leave a complete unit of six pad edges, e_cap and t_cap even."""
    e, t, ei, i, q = (int(v * head) for v in n)
    return (e // 2 * 2 + slack[0], t // 2 * 2 + slack[1], ei + slack[2], i + slack[3], q + slack[4])


def groups_for(e_cap, e_min, deg):
    """Dummy groups for the largest padding e_cap - e_min: a unit of six puts two pad edges on atoms a and b of its group."""
    units = -(-max(e_cap - e_min, 0) // 6)
    return max(1, -(-units // max(deg // 2, 1)))


def idx_tensors(ref, keys=IDX_KEYS):
    import torch
    return {k: torch.tensor(np.asarray(ref[k])) for k in keys}


def check_padded(o, ref, A, caps, G):
    """`o`: eighteen capacity-sized numpy arrays; real rows = `ref`, the pad rows a valid graph on the dummy atoms: what
    tests/test_pbc_q_padded_cpu.py asks of `pad_indices` and the GPU tests of the kernel's output."""
    n = sizes(ref)
    for k in IDX_KEYS:
        f = FAMILY[k]
        want = np.asarray(ref[k]).reshape((n[f], 3) if k in OFF_KEYS else (n[f],))
        assert o[k].shape[0] == caps[f], k
        assert np.array_equal(o[k][:n[f]], want), k                                 # real rows first, untouched
    E, T, Ei, I, Qn = n
    assert not o["cell_offsets"][E:].any() and not o["int_cell_offsets"][Ei:].any()  # pad rows sit in image 0
    lo, hi = A, A + 4 * G
    for k, first in (("id_c", E), ("id_a", E), ("id4_int_a", Ei), ("id4_int_b", Ei)):   # pad rows name dummy atoms only
        pad = o[k][first:]
        assert pad.size == 0 or (pad.min() >= lo and pad.max() < hi), k
    for k, first, row0, cap in (("id3_reduce_ca", T, E, caps[0]), ("id3_expand_ba", T, E, caps[0]),
                                ("id4_reduce_intm_ca", I, E, caps[0]), ("id4_expand_intm_db", I, E, caps[0]),
                                ("id4_reduce_intm_ab", I, Ei, caps[2]), ("id4_expand_intm_ab", I, Ei, caps[2]),
                                ("id4_reduce_ca", Qn, E, caps[0]), ("id4_expand_db", Qn, E, caps[0]),
                                ("id4_reduce_cab", Qn, I, caps[3]), ("id4_expand_abd", Qn, I, caps[3])):
        pad = o[k][first:]                                                           # ... and pad rows only
        assert pad.size == 0 or (pad.min() >= row0 and pad.max() < cap), k
    sw = o["id_swap"]
    assert np.array_equal(sw[sw], np.arange(caps[0]))                                # an involution ...
    assert np.array_equal(o["cell_offsets"][sw], -o["cell_offsets"])                 # ... that negates the offsets
    assert np.array_equal(o["id_c"][sw], o["id_a"]) and np.array_equal(o["id_undir"][sw], o["id_undir"])
    r, x = o["id3_reduce_ca"], o["id3_expand_ba"]
    assert (r[1:] >= r[:-1]).all() and np.array_equal(o["id_a"][r], o["id_a"][x]) and (r != x).all()
    # the cross-family identities of pbc_q_common.check_invariants (lines 179-188).  Over ALL rows when the dummy molecule is one
    # group with at most one complete unit of pad edges; with more groups or units a pad row still names pad rows and dummy atoms
    # only (above), but a pad intermediate triplet may take its edges from another group than its interaction edge and a pad
    # quadruplet's reduce edge is spread over the units on its own (padded._pad_intm / _pad_quads, the molecular layout): there
    # the identities are asked of the real rows, and of every row where the layout keeps them
    rows_all = G == 1 and (caps[0] - E) // 6 <= 1
    cut = (lambda v, n: v) if rows_all else (lambda v, n: v[:n])
    id_a, id_c, int_a, int_b = o["id_a"], o["id_c"], o["id4_int_a"], o["id4_int_b"]
    ica, idb = o["id4_reduce_intm_ca"], o["id4_expand_intm_db"]
    iab_r, iab_e = o["id4_reduce_intm_ab"], o["id4_expand_intm_ab"]
    assert np.array_equal(cut(id_a[ica], I), cut(int_a[iab_r], I)) and np.array_equal(cut(id_a[idb], I), cut(int_b[iab_e], I))
    ca, db, cab, abd = (o[k] for k in ("id4_reduce_ca", "id4_expand_db", "id4_reduce_cab", "id4_expand_abd"))
    assert np.array_equal(idb[abd], db)
    assert np.array_equal(cut(ica[cab], Qn), cut(ca, Qn))
    assert np.array_equal(iab_r[cab], iab_e[abd])                                    # both halves hang on one interaction edge
    k = iab_r[cab]
    assert np.array_equal(cut(id_a[ca], Qn), cut(int_a[k], Qn)) and np.array_equal(cut(id_a[db], Qn), cut(int_b[k], Qn))
    assert np.array_equal(cut(id_c[ca], Qn), cut(id_c[ica][cab], Qn)) and np.array_equal(id_c[db], id_c[idb][abd])
    assert (iab_e[1:] >= iab_e[:-1]).all() and (ca[1:] >= ca[:-1]).all()             # the sorted lists stay sorted


def expected_error(n, deg, caps, G, deg_bound):
    """The error bits gn_pbc_qindex_padded must report for counts n = (E, T, Eint, I, Q) and a largest in-degree `deg`, restated
    from include/gemnet_hip.h: capacities first (the later families are not judged when a list they are counted from does not
    fit), then the padding rules of padded.py, then the two in-degree bounds."""
    E, T, Ei, I, Qn = n
    err = (1 if E > caps[0] else 0) | (256 if Ei > caps[2] else 0)
    if err:
        return err
    err = (2 if T > caps[1] else 0) | (512 if I > caps[3] else 0) | (1024 if Qn > caps[4] else 0)
    if err:
        return err
    ep, tp, eintp, ip, qp = (c - v for c, v in zip(caps, n))
    if (tp and ep < 6) or tp % 2:
        err |= 4
    if ((tp or ip or qp) and ep < 6) or (ip and eintp < 1) or (qp and ip < 1):
        err |= 2048
    if 2 * -(-(-(-ep // 6)) // G) > max(deg_bound, 2):
        err |= 8
    if deg > deg_bound:
        err |= 16
    return err


def tight_caps(n):
    """Capacities with zero padding in all five families when none is empty.  A capacity must be positive, so an EMPTY family
    gets the smallest padding the rules allow: one pad row (two pad triplets), together with the pad rows it refers to — a unit
    of six pad edges, a pad interaction edge under a pad intermediate triplet, a pad intermediate triplet under a pad
    quadruplet — which may pad a non-empty family as well."""
    E, T, Ei, I, Qn = n
    qp = 1 if Qn == 0 else 0
    ip = 1 if (I == 0 or qp) else 0
    eintp = 1 if (Ei == 0 or ip) else 0
    tp = 2 if T == 0 else 0
    ep = 6 if (E == 0 or tp or ip or qp) else 0
    return (E + ep, T + tp, Ei + eintp, I + ip, Qn + qp)
