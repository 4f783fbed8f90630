"""The host tables of the grouped weight-gradient launch (training/wgrad_queue.py::build_tables), without a GPU.

The two grouped kernels of csrc/gemm_tn.hip trust three tables blindly.  A numpy interpreter written from the contract in
include/gemnet_hip.h (gn_tn_problem, gn_tn_target) — not from `flush` — executes them workgroup by workgroup in float64 on
numpy arenas: every workgroup must map to exactly one (problem, slice, tile), every workspace float must be written once and
folded once, and the targets must end up holding the direct float64 sums.  "Addresses" are byte offsets (4 per element, as
for fp32 on the device) into the arenas."""
import numpy as np
import pytest

from gemnet_pytorch_amd.training import wgrad_queue as WQ
from gemnet_pytorch_amd.training.wgrad_queue import PROB, TARGET, build_tables

TILE = 64          # gn_tn_problem: ceil(M/64) * ceil(N/64) tiles per slice; gn_tn_target: ceil(n/64) fold workgroups
SIZES = (1, 6, 16, 42, 63, 64, 65, 128, 130)
KS = (1, 15, 16, 17, 2047, 4096, 4097, 9001)
K_CAP = 66 * 2048 + 5      # K // 2048 = 66 slices asked for: the cap at 64 decides


def test_struct_sizes_match_the_header():
    assert PROB.itemsize == 64 and TARGET.itemsize == 40
    assert WQ.SPLIT_ROWS == 2048, "the cases below are placed around the default slice length"


class Arena:
    """A float64 array addressed in bytes of fp32."""

    def __init__(self):
        self.chunks, self.size = [], 0

    def put(self, a, gap=0, fill=np.nan):
        addr = 4 * self.size
        self.chunks.append(np.asarray(a, dtype=np.float64).reshape(-1))
        if gap:
            self.chunks.append(np.full(gap, fill))          # (NaN between operands: nothing may read it)
        self.size += a.size + gap
        return addr

    def freeze(self):
        return np.concatenate(self.chunks) if self.chunks else np.zeros(0)


def make_case(seed=20240607):
    """-> entries for build_tables, the operand arena, the gradient arena (pre-filled) and, per entry, (X, Y) views."""
    rs = np.random.RandomState(seed)
    ops, grads = Arena(), Arena()
    entries, mats = [], []

    def operand(K, M, ld=None):
        ld = M if ld is None else ld
        buf = rs.standard_normal((K, ld))
        return ops.put(buf, gap=3), buf[:, :M], ld

    def add(tgt, K, alpha=1.0, ldx_pad=0, ldy_pad=0):
        _, M, N, _ = tgt
        xa, X, ldx = operand(K, M, M + ldx_pad)
        ya, Y, ldy = operand(K, N, N + ldy_pad)
        entries.append((tgt, xa, ya, M, N, K, ldx, ldy, alpha))
        mats.append((X, Y))

    def param(rows, cols):
        return grads.put(rs.standard_normal((rows, cols)), gap=5, fill=7.0)

    # 1. every contraction length of the list, on contiguous targets that walk through every M and every N
    for i, K in enumerate(KS):
        M, N = SIZES[i % len(SIZES)], SIZES[(i + 4) % len(SIZES)]
        add((param(M, N), M, N, N), K, alpha=(1.0, 0.5, -2.0)[i % 3], ldx_pad=i % 3, ldy_pad=(i + 1) % 2)
    for i, M in enumerate(SIZES):                                   # ... and the square / transposed pairs, K around a slice
        N = SIZES[len(SIZES) - 1 - i]
        add((param(M, N), M, N, N), (2047, 4097, 17)[i % 3])
    add((param(6, 1), 6, 1, 1), K_CAP, alpha=0.25)                  # the min(64, .) cap of the slice count
    add((param(130, 128), 130, 128, 128), 9001)                     # several slices of several tiles
    # 2. one target hit by many products of mixed length (its slice list is longer than the fold's 16 groups)
    hot = (param(16, 42), 16, 42, 42)
    for i in range(41):
        add(hot, (1, 15, 16, 17, 4097, 33)[i % 6], alpha=1.0 if i % 2 else -0.5)
    # 3. the three column blocks of a concat weight (rows 42, widths 63 + 64 + 65), two products each
    widths = (63, 64, 65)
    wcat = param(42, sum(widths))
    c0 = 0
    for w in widths:
        for K in (17, 4097):
            add((wcat + 4 * c0, 42, w, sum(widths)), K)
        c0 += w
    # 4. the (C, O) regions of a bilinear weight (C, I, O): rows c with pitch I * O
    C, I, O = 16, 6, 42
    wbil = param(C, I * O)
    for i in range(I):
        add((wbil + 4 * i * O, C, O, I * O), (15, 4096)[i % 2], ldx_pad=(I - 1) * C)       # X = P[:, i, :] of (K, I, C)
    # 5. empty contractions: into the hot target, into a concat block, and into a parameter nothing else reaches
    lonely = param(64, 64)
    for tgt in (hot, (wcat, 42, 63, sum(widths)), (lonely, 64, 64, 64), (lonely, 64, 64, 64)):
        add(tgt, 0)
    order = rs.permutation(len(entries))                            # tile counts of neighbours differ wildly
    entries = [entries[i] for i in order]
    mats = [mats[i] for i in order]
    return entries, mats, ops.freeze(), grads.freeze(), dict(hot=hot, lonely=lonely)


def find_by_wg_begin(table, wg):
    """The kernels' search: the last row with wg_begin <= wg."""
    lo, hi = 0, len(table) - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if table[mid]["wg_begin"] <= wg:
            lo = mid
        else:
            hi = mid - 1
    return lo


def interpret(probs, targets, slice_off, total_wg, total_fold_wg, ws_floats, ops, grads):
    """Run both grouped kernels as include/gemnet_hip.h describes them.  -> (grads after, writes per workspace float,
    folds per workspace float, (problem, z, tm, tn) per workgroup)."""
    ws = np.full(ws_floats, np.nan)
    written = np.zeros(ws_floats, dtype=np.int64)
    seen = []
    for wg in range(total_wg):
        p = probs[find_by_wg_begin(probs, wg)]
        M, N, K, ldx, ldy, kchunk = (int(p[f]) for f in ("M", "N", "K", "ldx", "ldy", "kchunk"))
        tiles_m, tiles_n = -(-M // TILE), -(-N // TILE)
        local = wg - int(p["wg_begin"])
        z, local = divmod(local, tiles_m * tiles_n)
        tm, tn = divmod(local, tiles_n)
        assert 0 <= z < int(p["splitk"])
        seen.append((int(p["wg_begin"]), z, tm, tn))
        kbeg, kend = z * kchunk, min(K, (z + 1) * kchunk)
        assert kbeg < kend
        r0, r1, c0, c1 = tm * TILE, min(M, (tm + 1) * TILE), tn * TILE, min(N, (tn + 1) * TILE)
        k = np.arange(kbeg, kend)[:, None]
        X = ops[int(p["X"]) // 4 + k * ldx + np.arange(r0, r1)[None, :]]
        Y = ops[int(p["Y"]) // 4 + k * ldy + np.arange(c0, c1)[None, :]]
        tile = float(p["alpha"]) * (X.T @ Y)
        base = int(p["ws_off"]) + z * M * N
        idx = base + np.arange(r0, r1)[:, None] * N + np.arange(c0, c1)[None, :]
        ws[idx] = tile
        written[idx] += 1
    out = grads.copy()
    folded = np.zeros(ws_floats, dtype=np.int64)
    for wg in range(total_fold_wg):
        t = targets[find_by_wg_begin(targets, wg)]
        n, cols, ld = int(t["n"]), int(t["cols"]), int(t["ld"])
        i = (wg - int(t["wg_begin"])) * 64 + np.arange(64)
        i = i[i < n]
        assert i.size > 0
        acc = np.zeros(i.size)
        for k in range(int(t["slice_begin"]), int(t["slice_end"])):
            acc += ws[int(slice_off[k]) + i]
            folded[int(slice_off[k]) + i] += 1
        o = (i // cols) * ld + (i % cols) if cols > 0 else i
        out[int(t["out"]) // 4 + o] += acc
    return out, written, folded, seen


@pytest.fixture(scope="module")
def case():
    entries, mats, ops, grads, named = make_case()
    tables = build_tables(entries)
    return entries, mats, ops, grads, named, tables


def test_the_case_holds_what_it_is_meant_to(case):
    entries, _, _, _, named, _ = case
    assert len(entries) >= 60
    Ks = [e[5] for e in entries]
    assert set(KS) <= set(Ks) and max(Ks) >= K_CAP and Ks.count(0) >= 3
    assert {e[3] for e in entries} >= set(SIZES) and {e[4] for e in entries} >= set(SIZES)
    assert sum(1 for e in entries if e[0] == named["hot"] and e[5] > 0) >= 40
    assert sum(1 for e in entries if e[0][3] != e[0][2]) >= 12          # column blocks and (C, O) regions


def test_table_invariants(case):
    entries, _, _, _, named, (probs, targets, slice_off, total_wg, total_fold_wg, ws_floats) = case
    live = [e for e in entries if e[5] > 0]
    assert len(probs) == len(live)
    assert [int(k) for k in probs["K"]] == [e[5] for e in live], "products keep their enqueue order"
    M, N, K = (probs[f].astype(np.int64) for f in ("M", "N", "K"))
    splitk, kchunk = probs["splitk"].astype(np.int64), probs["kchunk"].astype(np.int64)
    assert (kchunk % 16 == 0).all() and (kchunk > 0).all() and (splitk >= 1).all() and (splitk <= 64).all()
    assert ((splitk - 1) * kchunk < K).all(), "an empty slice"
    assert (splitk * kchunk >= K).all(), "rows of the contraction left out"
    assert int(splitk.max()) == 64 and int(splitk[K == 4097][0]) == 2 and int(splitk[K == 2047][0]) == 1
    wgs = -(-M // TILE) * -(-N // TILE) * splitk
    assert probs["wg_begin"][0] == 0 and (np.diff(probs["wg_begin"]) > 0).all()
    assert (probs["wg_begin"] == np.concatenate([[0], np.cumsum(wgs)[:-1]])).all() and total_wg == int(wgs.sum())
    # the workspace: the slices [ws_off + z M N, + M N) tile [0, ws_floats) without overlap
    starts = np.concatenate([int(o) + np.arange(int(s)) * int(m * n) for o, s, m, n in zip(probs["ws_off"], splitk, M, N)])
    sizes = np.concatenate([np.full(int(s), int(m * n)) for s, m, n in zip(splitk, M, N)])
    order = np.argsort(starts)
    assert starts[order][0] == 0 and (starts[order][1:] == (starts + sizes)[order][:-1]).all()
    assert int((starts + sizes).max()) == ws_floats == int((splitk * M * N).sum())
    # every slice in exactly one target's list, exactly once; the lists partition slice_off
    assert sorted(int(s) for s in slice_off) == sorted(int(s) for s in starts)
    assert targets["slice_begin"][0] == 0 and int(targets["slice_end"][-1]) == len(slice_off)
    assert (targets["slice_begin"][1:] == targets["slice_end"][:-1]).all() and (targets["slice_end"] > targets["slice_begin"]).all()
    size_of = dict(zip(starts.tolist(), sizes.tolist()))
    for t in targets:
        assert all(size_of[int(s)] == int(t["n"]) for s in slice_off[int(t["slice_begin"]):int(t["slice_end"])])
    fwg = -(-targets["n"] // 64)
    assert targets["wg_begin"][0] == 0 and (np.diff(targets["wg_begin"]) > 0).all()
    assert (targets["wg_begin"] == np.concatenate([[0], np.cumsum(fwg)[:-1]])).all() and total_fold_wg == int(fwg.sum())
    # one target per distinct region; strided regions carry cols / ld, contiguous ones 0 / 0
    regions = list(dict.fromkeys(e[0] for e in live))
    assert len(targets) == len(regions)
    for t, (addr, rows, cols, ld) in zip(targets, regions):
        assert (int(t["out"]), int(t["n"])) == (addr, rows * cols)
        assert (int(t["cols"]), int(t["ld"])) == ((cols, ld) if ld != cols else (0, 0))
    assert named["lonely"] not in targets["out"].tolist(), "a target of empty contractions only has no row"
    hot = [t for t in targets if int(t["out"]) == named["hot"][0]]
    assert len(hot) == 1 and int(hot[0]["slice_end"] - hot[0]["slice_begin"]) > 40


def reference(entries, mats, grads):
    """-> (grads + the direct float64 sums, sum |alpha| |X|^T |Y| per element: 0 outside every target region)."""
    want = grads.copy()
    scale = np.zeros_like(grads)
    for (tgt, _, _, M, N, K, _, _, alpha), (X, Y) in zip(entries, mats):
        addr, rows, cols, ld = tgt
        idx = addr // 4 + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
        want[idx] += alpha * (X.T @ Y)
        scale[idx] += abs(alpha) * (np.abs(X).T @ np.abs(Y))
    return want, scale


def test_interpreted_kernels_cover_the_workspace_once_and_give_the_float64_sums(case):
    entries, mats, ops, grads, named, tables = case
    out, written, folded, seen = interpret(*tables, ops, grads)
    assert (written == 1).all(), "a workspace float written twice or never"
    assert (folded == 1).all(), "a workspace float folded twice or never"
    assert len(set(seen)) == len(seen) == tables[3], "two workgroups with the same (problem, slice, tile)"
    # everything outside the regions stays as it was; inside: 1e-12 relative to the sum of the magnitudes of the terms (the
    # measure of a dot product's rounding error: two float64 summation orders differ by ~1e-16 sqrt(K) of it)
    want, scale = reference(entries, mats, grads)
    touched = scale > 0
    assert touched.any() and not touched.all()
    assert np.array_equal(out[~touched], grads[~touched]), "an element outside every target region changed"
    err = np.abs(out - want)[touched]
    assert (err <= 1e-12 * scale[touched]).all(), float((err / scale[touched]).max())
    lonely = named["lonely"] // 4
    assert np.array_equal(out[lonely:lonely + 64 * 64], grads[lonely:lonely + 64 * 64])
    assert len(tables[0]) < len(entries)


def test_empty_contractions_alone_give_empty_tables():
    probs, targets, slice_off, total_wg, total_fold_wg, ws_floats = build_tables(
        [((1024, 8, 8, 8), 0, 0, 8, 8, 0, 8, 8, 1.0), ((4096, 4, 2, 2), 0, 0, 4, 2, 0, 4, 2, -1.0)])
    assert len(probs) == len(targets) == len(slice_off) == 0 and (total_wg, total_fold_wg, ws_floats) == (0, 0, 0)
    assert build_tables([])[3:] == (0, 0, 0)


def test_interpreter_notices_a_broken_table(case):
    """The checks above are not vacuous: a slice listed twice, or a slice length 16 rows short, fails them."""
    entries, mats, ops, grads, named, (probs, targets, slice_off, total_wg, total_fold_wg, ws_floats) = case
    bad_off = slice_off.copy()
    bad_off[3] = bad_off[4]
    _, _, folded, _ = interpret(probs, targets, bad_off, total_wg, total_fold_wg, ws_floats, ops, grads)
    assert not (folded == 1).all()
    bad = probs.copy()
    j = int(np.argmax(bad["K"] == 9001))
    bad["kchunk"][j] -= 16                                           # rows at the end of every slice are never read
    out, written, folded, _ = interpret(bad, targets, slice_off, total_wg, total_fold_wg, ws_floats, ops, grads)
    want, scale = reference(entries, mats, grads)
    assert (written == 1).all() and (folded == 1).all()
    assert (np.abs(out - want)[scale > 0] / scale[scale > 0]).max() > 1e-6
