"""-m gpu: the two hand-written kernels that end every training step, each against an independent float64 reference.

  * gn_gemm_tn_grouped_f32 (csrc/gemm_tn.hip) through training/wgrad_queue.py::WeightGradQueue on raw tensors: split-K slices,
    K tails, the scalar-load path, strided operands and strided fold targets, more than 16 slices per target, capture.
  * gn_adamw_ema_step_f32 (csrc/optim.hip) on raw flat buffers against torch.optim.AdamW in float64, step by step.

Inputs, references and bounds are built on the CPU (seeded); only the kernels under test run on the device.  Every bound is
derived from the arithmetic (see the comments at `gemm_bound` and `optimizer_bounds`), and for each kernel a set of
deliberately wrong references shows that the bound would notice them."""
import math
import time

import numpy as np
import pytest
import torch

from conftest import SCALE_FILE
from gemnet_pytorch_amd import _lib
from gemnet_pytorch_amd.training import wgrad_queue as WQ
from gemnet_pytorch_amd.training.wgrad_queue import WeightGradQueue
from redzone import put, redzone  # noqa: F401  (autouse: every test of this module runs under the red-zone harness)

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24          # unit roundoff of fp32


# =====================================================================================================================
# grouped weight gradients
# =====================================================================================================================
def split_of(K):
    """Slices of a contraction of K rows as the contract of gn_tn_problem asks: kchunk a multiple of 16, no empty slice."""
    splitk = max(1, min(64, K // 2048))
    kchunk = (-(-K // splitk) + 15) // 16 * 16
    return -(-K // kchunk), kchunk


class GemmCase:
    """Leaves with a pre-filled .grad and a list of products into them.  Operands are positive (uniform [0.5, 1.5) times a
    factor per column in [0.5, 1.5)): |X|^T |Y| = X^T Y, nothing cancels, so a dropped slice or a misplaced block is as
    large against the rounding bound as it can be, and every row and column of a product has its own magnitude."""

    def __init__(self, seed=1234):
        self.gen = torch.Generator().manual_seed(seed)
        self.leaves = {}        # name -> (rows, cols) of the 2-D picture of the leaf's .grad
        self.shape = {}         # name -> shape of the leaf itself
        self.grad0 = {}
        self.ops = {}           # name -> fp32 CPU tensor (operand storage)
        self.items = []         # dict(leaf, r0, c0, M, N, x=(op, index), y=(op, index), alpha, how)

    def rand(self, *shape):
        return torch.rand(*shape, generator=self.gen) + 0.5

    def operand(self, name, K, *rest):
        t = self.rand(K, *rest) * self.rand(*rest)
        self.ops[name] = t.float()
        return name

    def leaf(self, name, rows, cols, shape=None):
        self.leaves[name] = (rows, cols)
        self.shape[name] = shape or (rows, cols)
        self.grad0[name] = (torch.randn(rows, cols, generator=self.gen) * 2).float()

    def product(self, leaf, x, y, alpha=1.0, how="leaf", r0=0, c0=0):
        """x, y: (operand name, index expression applied to the stored tensor) -> a 2-D (K, M) / (K, N) view."""
        X, Y = self.view(x), self.view(y)
        assert X.shape[0] == Y.shape[0]
        self.items.append(dict(leaf=leaf, r0=r0, c0=c0, M=X.shape[1], N=Y.shape[1], K=X.shape[0], x=x, y=y,
                               alpha=alpha, how=how))

    def view(self, spec, ops=None):
        name, idx = spec
        t = (ops or self.ops)[name]
        return t if idx is None else t[idx]


def main_case():
    c = GemmCase()
    sl = slice
    # split slices, plain leaves ----------------------------------------------------------------------------------------
    for name, K, M, N, alpha in [("k4097", 4097, 16, 64, 1.0),          # 2 slices, the last 1 row past a 16-multiple
                                 ("k6151", 6151, 64, 16, 0.5),          # 3 slices, K % 16 = 7
                                 ("k2047", 2047, 16, 16, -2.0),         # 1 slice, K % 16 = 15
                                 ("k17", 17, 64, 64, 1.0),              # 1 slice of 2 K-steps, the second 1 row
                                 ("k40000", 40000, 64, 64, 1.0),        # 19 slices: the shape of full-size training
                                 ("m6", 100, 6, 16, 1.0),               # M % 4 != 0: scalar loads
                                 ("m42", 4097, 42, 64, 0.5),            # ... over two slices
                                 ("p65", 333, 65, 130, 1.0),            # partial tiles in both directions, 2 x 3 tiles
                                 ("p1", 17, 1, 1, -2.0)]:
        c.leaf(name, M, N)
        c.product(name, (c.operand(name + ".x", K, M), None), (c.operand(name + ".y", K, N), None), alpha)
    # an operand 8-byte but not 16-byte aligned: X = big[:, 2:18] (M % 4 == 0, ldx % 4 == 0: only the address rules out float4)
    c.leaf("mis", 16, 64)
    c.product("mis", (c.operand("mis.big", 300, 24), (sl(None), sl(2, 18))), (c.operand("mis.y", 300, 64), None))
    # the (C, O) regions of a bilinear weight (C, I, O) from X = P[:, i, :] of (K, I, C), Y = Q[:, i, :] of (K, I, O)
    C, I, O, K = 64, 16, 64, 4500
    c.leaf("bil", C, I * O, shape=(C, I, O))
    c.operand("bil.P", K, I, C)
    c.operand("bil.Q", K, I, O)
    for i in range(I):
        c.product("bil", ("bil.P", (sl(None), i)), ("bil.Q", (sl(None), i)), how="region", c0=i * O)
    # more than 16 slices into one target: 20 x 2 = 40, exactly 8 x 2 = 16, and 8 x 2 + 1 = 17
    c.operand("pool.x", 4097 + 20 * 96, 128)
    c.operand("pool.y", 4097 + 20 * 96, 128)
    for name, count, M, N, extra in [("s40", 20, 128, 128, 0), ("s16", 8, 16, 16, 0), ("s17", 8, 16, 64, 1)]:
        c.leaf(name, M, N)
        for j in range(count):      # (row windows of one pool: every product has its own data, the storage stays small)
            c.product(name, ("pool.x", (sl(96 * j, 96 * j + 4097), sl(0, M))), ("pool.y", (sl(96 * j + 32, 96 * j + 32 + 4097), sl(0, N))))
        if extra:
            c.product(name, ("pool.x", (sl(5, 5 + 2047), sl(0, M))), ("pool.y", (sl(9, 9 + 2047), sl(0, N))))
    # the three column blocks of a concat weight, two products each; Y_b = Y[:, block] (row pitch 384)
    c.leaf("cat", 128, 384)
    for k, (K, alpha) in enumerate([(4097, 1.0), (150, 0.5)]):
        c.operand(f"cat.x{k}", K, 128)
        c.operand(f"cat.y{k}", K, 384)
        for b in range(3):
            c.product("cat", (f"cat.x{k}", None), (f"cat.y{k}", (sl(None), sl(128 * b, 128 * b + 128))), alpha, how="view", c0=128 * b)
    # empty contractions: into a live target and into a leaf nothing else reaches
    c.leaf("lonely", 8, 8)
    c.operand("e0.x", 0, 16)
    c.operand("e0.y", 0, 64)
    c.operand("e1.x", 0, 8)
    c.operand("e1.y", 0, 8)
    c.product("k4097", ("e0.x", None), ("e0.y", None))
    c.product("lonely", ("e1.x", None), ("e1.y", None), alpha=0.5)
    c.items.insert(7, c.items.pop())        # (not at the end of the queue)
    return c


def gemm_reference(c):
    """float64: -> {leaf: grad0 + sum alpha X^T Y}, {leaf: sum |alpha| |X|^T |Y|}, {leaf: (longest slice, slices)}."""
    ref = {n: g.double().clone() for n, g in c.grad0.items()}
    mag = {n: torch.zeros_like(r) for n, r in ref.items()}
    info = {n: [0, 0] for n in ref}
    for it in c.items:
        if it["K"] == 0:
            continue
        X, Y = c.view(it["x"]).double(), c.view(it["y"]).double()
        assert float(X.min()) > 0 and float(Y.min()) > 0            # |X|^T |Y| = X^T Y
        splitk, kchunk = split_of(it["K"])
        info[it["leaf"]][0] = max(info[it["leaf"]][0], min(kchunk, it["K"]))
        info[it["leaf"]][1] += splitk
        prod = X.T @ Y
        ref[it["leaf"]][region_of(it)] += it["alpha"] * prod
        mag[it["leaf"]][region_of(it)] += abs(it["alpha"]) * prod
    return ref, mag, info


def region_of(it):
    return slice(it["r0"], it["r0"] + it["M"]), slice(it["c0"], it["c0"] + it["N"])


def gemm_bound(ref, mag, info):
    """Per element.  One slice is a dot product of at most `kc` terms accumulated in fp32 (the matrix-core accumulator) and
    scaled by alpha: |error| <= (kc + 1) u sum|x||y| (Higham, Accuracy and Stability, (3.5)).  The fold adds the S slices of a
    target in 16 groups of ceil(S/16), then the 16 group sums, then adds the total to .grad: a partial passes through at most
    ceil(S/16) + 16 additions, each with relative error u on a partial sum of magnitude <= sum |alpha||x||y|, and the last
    addition rounds grad0 + sum once.  So  gamma = (kc + 1 + ceil(S/16) + 16) u  on  |alpha| |X|^T |Y|  plus  u |result|."""
    return {n: (info[n][0] + 1 + -(-info[n][1] // 16) + 16) * U * mag[n] + U * ref[n].abs() for n in ref}


@pytest.fixture(scope="module")
def gemm():
    c = main_case()
    ref, mag, info = gemm_reference(c)
    return c, ref, mag, gemm_bound(ref, mag, info)


class Device:
    """The case on the device: leaves (requires_grad, .grad = grad0) and operand storage; `enqueue` adds every product."""

    def __init__(self, c):
        self.c = c
        self.ops = {n: put(t) for n, t in c.ops.items()}
        self.param = {}
        for n in c.leaves:
            p = torch.zeros(c.shape[n], device=DEV, requires_grad=True)
            p.grad = torch.empty(c.shape[n], device=DEV)
            self.param[n] = p
        self.reset()

    def reset(self, zero=False):
        for n, p in self.param.items():
            p.grad.copy_(torch.zeros_like(p.grad) if zero else self.c.grad0[n].to(DEV).view_as(p.grad))

    def grads(self):
        return {n: p.grad.detach().reshape(self.c.leaves[n]).clone() for n, p in self.param.items()}

    def enqueue(self, q, items=None):
        for it in (self.c.items if items is None else items):
            X, Y, p = self.c.view(it["x"], self.ops), self.c.view(it["y"], self.ops), self.param[it["leaf"]]
            if it["how"] == "leaf":
                q.add(p, X, Y, it["alpha"])
            elif it["how"] == "view":                   # a column block W[:, a:b] of the leaf, a fresh view object each time
                q.add(p[:, it["c0"]:it["c0"] + it["N"]], X, Y, it["alpha"])
            else:                                       # an explicit (C, O) region with pitch I * O
                ld = self.c.leaves[it["leaf"]][1]
                q.add_region((p.grad.data_ptr() + 4 * (it["r0"] * ld + it["c0"]), it["M"], it["N"], ld), X, Y, keep=p, alpha=it["alpha"])


def test_case_reaches_the_paths_it_names(gemm):
    c = gemm[0]
    assert WQ.SPLIT_ROWS == 2048
    by = {}
    for it in c.items:
        by.setdefault(it["leaf"], []).append(split_of(it["K"])[0] if it["K"] else 0)
    assert by["k4097"] == [2, 0] and by["k6151"] == [3] and by["k2047"] == [1] and by["k17"] == [1] and by["k40000"] == [19]
    assert (sum(by["s40"]), sum(by["s16"]), sum(by["s17"])) == (40, 16, 17)
    assert by["lonely"] == [0] and len(by["bil"]) == 16 and len(by["cat"]) == 6
    X = c.view(c.items[[it["leaf"] for it in c.items].index("mis")]["x"])
    assert X.storage_offset() * 4 % 16 == 8 and X.stride(0) % 4 == 0 and X.shape[1] % 4 == 0 and WQ._rowmajor(X) is X
    P = c.view(("bil.P", (slice(None), 3)))
    assert WQ._rowmajor(P) is P and P.stride(0) == 16 * 64


def test_grouped_gemm_bound_notices_a_dropped_slice_and_a_misplaced_fold_group(gemm):
    """No kernel runs here: the two corruptions are applied to the float64 reference; each must exceed the bound 100 times."""
    c, ref, mag, bound = gemm
    worst = {}
    first_region = {}
    for j, it in enumerate(c.items):
        if it["K"] == 0:
            continue
        first_region.setdefault(it["leaf"], it)
        # the last slice (the shortest) of this product never reaches the fold
        X, Y = c.view(it["x"]).double(), c.view(it["y"]).double()
        splitk, kchunk = split_of(it["K"])
        bad = ref[it["leaf"]].clone()
        bad[region_of(it)] -= it["alpha"] * (X[(splitk - 1) * kchunk:].T @ Y[(splitk - 1) * kchunk:])
        worst[("slice dropped", it["leaf"], j)] = float(((bad - ref[it["leaf"]]).abs() / bound[it["leaf"]]).max())
    for n, it in first_region.items():
        if it["M"] * it["N"] < 64 + it["N"]:
            continue                                    # (the 1 x 1 target has no second row)
        # the sums of the first fold workgroup (64 consecutive elements of the region) land one row further down
        inc = (ref[n] - c.grad0[n].double())[region_of(it)].reshape(-1)
        moved = inc[:64].clone()
        inc[:64] -= moved
        inc[it["N"]:it["N"] + 64] += moved
        bad = c.grad0[n].double().clone()
        other = ref[n] - c.grad0[n].double()
        other[region_of(it)] = inc.reshape(it["M"], it["N"])
        bad += other
        worst[("fold group one row off", n)] = float(((bad - ref[n]).abs() / bound[n]).max())
    assert sum(k[0] == "fold group one row off" for k in worst) == len(c.leaves) - 2
    k = min(worst, key=worst.get)
    print(f"corrupted references: smallest excess over the bound {worst[k]:.0f}x {k}")
    assert worst[k] >= 100, (k, worst[k])


def check_grads(got, ref, bound, what):
    worst = 0.0
    for n in ref:
        ratio = float(((got[n].double().cpu() - ref[n]).abs() / bound[n].clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (what, n, ratio)
    return worst


def test_grouped_gemm_matches_float64_and_is_deterministic(gemm):
    """One flush with every case against grad0 + sum alpha X^T Y in float64, element by element within `gemm_bound`.
    Measured on MI355X: the largest |error| / bound over all targets is 0.11 (printed at every run); the smallest corruption
    of the test above is 204 times the bound."""
    c, ref, mag, bound = gemm
    t0 = time.perf_counter()
    d = Device(c)
    q = WeightGradQueue()
    d.enqueue(q)
    q.flush()
    torch.cuda.synchronize()
    g1 = d.grads()
    worst = check_grads(g1, ref, bound, "first flush")
    assert torch.equal(g1["lonely"].cpu(), c.grad0["lonely"]), "an empty contraction adds nothing"
    # the three column blocks together: the gradient of the whole concat weight, X^T Y with the full Y
    full = c.grad0["cat"].double() + sum(a * (c.ops[f"cat.x{k}"].double().T @ c.ops[f"cat.y{k}"].double()) for k, a in [(0, 1.0), (1, 0.5)])
    assert float(((g1["cat"].double().cpu() - full).abs() / bound["cat"]).max()) <= 1.0
    # the same products again into the same start values: bit for bit
    d.reset()
    d.enqueue(q)
    q.flush()
    torch.cuda.synchronize()
    g2 = d.grads()
    assert all(torch.equal(g1[n], g2[n]) for n in g1)
    print(f"grouped GEMM: largest |error| / bound = {worst:.4f}  ({time.perf_counter() - t0:.2f} s)")


def test_flush_of_empty_contractions_only_launches_nothing(gemm):
    c = gemm[0]
    d = Device(c)
    q = WeightGradQueue()
    d.enqueue(q, [it for it in c.items if it["K"] == 0])
    assert len(q.items) == 2
    q.flush()
    torch.cuda.synchronize()
    assert q.items == [] and q._ring == [] and q._keep is None, "no table, no workspace, no launch"
    got = d.grads()
    assert all(torch.equal(got[n].cpu(), c.grad0[n]) for n in got)


def test_grouped_gemm_captured_replays_add_the_eager_increment(gemm):
    """Into zeroed gradients the increment is the gradient itself: eager, first replay (bitwise the same), second replay on
    top of the first (x + x is exact in fp32: bitwise twice the increment)."""
    c = gemm[0]
    d = Device(c)
    q = WeightGradQueue()
    d.reset(zero=True)
    d.enqueue(q)
    q.flush()                                           # eager: also leaves the spare table slot the capture takes
    torch.cuda.synchronize()
    inc = d.grads()
    assert float(inc["k40000"].abs().min()) > 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d.enqueue(q)
        q.flush()
    d.reset(zero=True)
    graph.replay()
    torch.cuda.synchronize()
    once = d.grads()
    assert all(torch.equal(inc[n], once[n]) for n in inc)
    graph.replay()
    torch.cuda.synchronize()
    twice = d.grads()
    assert all(torch.equal(inc[n] + inc[n], twice[n]) for n in inc)


# =====================================================================================================================
# fused AdamW / EMA
# =====================================================================================================================
F32 = lambda x: float(np.float32(x))      # the C ABI takes float: the oracle gets the same numbers
LR, WD, EMA_DECAY, BETA1, BETA2, EPS = F32(1e-2), F32(0.05), F32(0.9), F32(0.9), F32(0.999), F32(1e-7)
SIZES = (1, 63, 2048 * 3 + 5, 2_097_152 + 2048 + 7)
# (gradient scale, max_norm) per step; a gradient of scale 1 has norm 3 (after gscale).  "main": the drop by 1e-3 leaves
# vmax > v in steps 3 and 4, the last step is clipped.  "tiny": norms of 4e-6 against max_norm 2e-6, where the "+ 1e-6" of the
# clip coefficient is a factor 0.8 (at max_norm 10 it is below fp32 resolution: that schedule cannot see it).
SCHEDULES = {"main": [(1.0, 10.0), (1.0, 10.0), (1e-3, 10.0), (1e-3, 10.0), (1.0, 10.0), (30.0, 10.0)],
             "tiny": [(4e-6 / 3, 2e-6), (4e-6 / 3, 2e-6)]}


def optimizer_inputs(n, schedule, seed=7):
    """fp32 CPU tensors: p0, wd, gscale, [g_t], plus the index sets of the special blocks."""
    gen = torch.Generator().manual_seed(seed + n % 1000)
    p0 = torch.randn(n, generator=gen)
    half = (n + 1) // 2
    wd = torch.zeros(n)
    wd[:half] = WD                                              # a contiguous half decays
    gscale = torch.ones(n)
    gscale[n // 4:n // 2] = 1.0 / 3.0
    gscale[n // 2:(3 * n) // 4] = 1.0 / 5.0
    w = max(1, n // 16) if n >= 32 else 0
    eps_block = slice(n // 8, n // 8 + w)
    zero_block = slice(half - w, half + w)                     # across the decay boundary
    grads = []
    for scale, _ in SCHEDULES[schedule]:
        g = torch.randn(n, generator=gen)
        g[zero_block] = 0.0
        g[eps_block] = 0.0
        g = g * (3.0 * scale / float((g.double() * gscale.double()).norm()))        # scaled norm 3 * scale
        small = 1e-8 * (torch.rand(n, generator=gen) + 0.5) * torch.sign(torch.randn(n, generator=gen))
        g[eps_block] = small[eps_block]                         # sqrt(v) ~ 1e-8 << eps = 1e-7
        grads.append(g.float())
    return p0.float(), wd.float(), gscale.float(), grads, eps_block, zero_block


def library_oracle(p0, wd, gscale, grads, schedule):
    """float64, torch.optim.AdamW(amsgrad) with the two groups.  -> per step dict(p, m, v, vmax, ema, norm, coef, ghat, upd)."""
    n = p0.numel()
    half = int((wd > 0).sum())
    assert bool((wd[:half] > 0).all()) and not bool((wd[half:] > 0).any())
    p = p0.double().clone()
    parts = [torch.nn.Parameter(p[:half].clone()), torch.nn.Parameter(p[half:].clone())]
    opt = torch.optim.AdamW([dict(params=[parts[0]], weight_decay=WD), dict(params=[parts[1]], weight_decay=0.0)],
                            lr=LR, betas=(BETA1, BETA2), eps=EPS, amsgrad=True, foreach=False)
    ema = p.clone()
    out = []
    for g, (_, max_norm) in zip(grads, SCHEDULES[schedule]):
        g64 = g.double() * gscale.double()
        norm = float(g64.norm())
        coef = min(1.0, F32(max_norm) / (norm + 1e-6))
        ghat = g64 * coef
        parts[0].grad, parts[1].grad = ghat[:half].clone(), ghat[half:].clone()
        opt.step()
        pn = torch.cat([parts[0].detach(), parts[1].detach()]).clone()
        ema = ema - (1.0 - EMA_DECAY) * (ema - pn)
        st = [opt.state[q] for q in parts]
        cat = lambda k: torch.cat([s[k] for s in st]).clone()
        out.append(dict(p=pn, m=cat("exp_avg"), v=cat("exp_avg_sq"), vmax=cat("max_exp_avg_sq"), ema=ema.clone(), norm=norm,
                        coef=coef, ghat=ghat))
    return out


def formula_oracle(p0, wd, gscale, grads, schedule, eps=EPS, amsgrad=True, decay_all=False, use_gscale=True, clip_eps=1e-6,
                   t_shift=0, ema_first=False):
    """The same step written out in float64 (checked against `library_oracle`), with switches for the wrong variants."""
    p, ema = p0.double().clone(), p0.double().clone()
    m, v, vmax = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    wd64 = torch.full_like(p, WD) if decay_all else wd.double()
    out = []
    for t, (g, (_, max_norm)) in enumerate(zip(grads, SCHEDULES[schedule]), start=1):
        g64 = g.double() * (gscale.double() if use_gscale else 1.0)
        norm = float(g64.norm())
        ghat = g64 * min(1.0, F32(max_norm) / (norm + clip_eps))
        if ema_first:
            ema = ema - (1.0 - EMA_DECAY) * (ema - p)
        m = m + (1.0 - BETA1) * (ghat - m)
        v = BETA2 * v + (1.0 - BETA2) * ghat * ghat
        vmax = torch.maximum(vmax, v)
        b1, b2 = 1.0 - BETA1 ** (t + t_shift), 1.0 - BETA2 ** (t + t_shift)
        p = p * (1.0 - LR * wd64) - (LR / b1) * m / ((vmax if amsgrad else v).sqrt() / math.sqrt(b2) + eps)
        if not ema_first:
            ema = ema - (1.0 - EMA_DECAY) * (ema - p)
        out.append(dict(p=p.clone(), m=m.clone(), v=v.clone(), vmax=vmax.clone(), ema=ema.clone(), norm=norm))
    return out


def optimizer_bounds(oracle):
    """Per element and step, from the kernel's fp32 formula (u = 2^-24; float64 quantities below are the oracle's).

    norm   accumulated in double, rounded to float once:                                   2 u norm
    ghat   g * gscale * clip, clip = max_norm / (norm + 1e-6) in fp32: 2 + 3 roundings:     rel 6 u;  G_t = max_{s<=t} |ghat_s|
    m      lerp: local error 0.1 (6u |g| + 2u |g - m|) + u |m'| <= 2 u G, damped by 0.9:     e_m(t) = 2 u G_t (1 - 0.9^t) / 0.1
    v      beta2 v + (1 - beta2) ghat^2: rel 14 u on the new term, 2 u on the sum, per step: e_v(t) = (2 t + 16) u V_t,
           V_t = max_{s<=t} v_s = vmax_t;  |max(a,b) - max(a',b')| <= max of the errors:      e_vmax(t) = e_v(t)
    update lr / bias1 * m / (sqrt(vmax) / bias2_sqrt + eps).  bias1 = 1 - powf(beta1, t), bias2_sqrt = sqrt(1 - powf(beta2, t))
           are computed in fp32 on the host: powf is good to 1 ulp = 2^-24 of a value in [0.5, 1), the subtraction is exact, so
           rel(bias1) <= 2^-24 / (1 - beta1^t) and rel(bias2_sqrt) <= 2^-25 / (1 - beta2^t) + u  — 3.0e-5 at t = 1, the
           dominant term, shrinking like 1/t.  rel(sqrt(vmax)) <= e_v / (2 vmax) + u = (t + 9) u.  Eight more roundings
           (two divisions by the bias terms, sqrt, + eps, m / denom, the products; each within 1 u with correctly rounded
           division and square root).  m enters with its ABSOLUTE error (it may cancel):
           e_upd(t) = |upd| (rel(bias1) + rel(bias2_sqrt) + (t + 17) u) + lr / bias1 * e_m(t) / denom
           (|upd| <= ~lr: this is the c_t * lr of the bound, with c_1 = 3.2e-5, c_2 = 1.7e-5, ... c_6 = 7e-6)
    p      p (1 - lr wd) - update: four roundings at |p| (k = 4 half-ulps), errors add up over the steps:
           e_p(t) = e_p(t-1) + 4 u |p_t| + e_upd(t)
    ema    ema - 0.1 (ema - p):   e_ema(t) = 0.9 e_ema(t-1) + 0.1 e_p(t) + 3 u max(|ema|, |p|)
    """
    out = []
    G = V = e_p = e_ema = None
    for t, o in enumerate(oracle, start=1):
        G = o["ghat"].abs() if G is None else torch.maximum(G, o["ghat"].abs())
        V = o["vmax"]
        e_m = 2 * U * G * (1 - 0.9 ** t) / 0.1
        e_v = (2 * t + 16) * U * V
        b1, b2 = 1.0 - BETA1 ** t, 1.0 - BETA2 ** t
        denom = V.sqrt() / math.sqrt(b2) + EPS
        adam = (LR / b1) * o["m"] / denom                   # the Adam part of the update (without the decay)
        rel = 2.0 ** -24 / b1 + 2.0 ** -25 / b2 + U + (t + 17) * U
        e_upd = adam.abs() * rel + (LR / b1) * e_m / denom
        e_p = (0 if e_p is None else e_p) + 4 * U * o["p"].abs() + e_upd
        e_ema = 0.9 * (0 if e_ema is None else e_ema) + 0.1 * e_p + 3 * U * torch.maximum(o["ema"].abs(), o["p"].abs())
        out.append(dict(p=e_p.clone(), m=e_m, v=e_v, vmax=e_v, ema=e_ema.clone(), norm=2 * U * o["norm"], c_t=rel))
    return out


_ORACLES = {}


def oracle_for(n, schedule):
    """(inputs, library oracle, bounds), computed once per (size, schedule) and left unchanged."""
    key = (n, schedule)
    if key not in _ORACLES:
        inp = optimizer_inputs(n, schedule)
        orc = library_oracle(*inp[:4], schedule)
        _ORACLES[key] = (inp, orc, optimizer_bounds(orc))
    return _ORACLES[key]


def excess(states, oracle, bounds):
    """Largest |state - oracle| / bound over the steps, quantities and elements."""
    worst = {}
    for st, o, b in zip(states, oracle, bounds):
        for k in ("p", "m", "v", "vmax", "ema"):
            err = (st[k].double() - o[k]).abs()
            worst[k] = max(worst.get(k, 0.0), float((err / b[k].clamp_min(1e-300)).max()) if bool((err > 0).any()) else 0.0)
        worst["norm"] = max(worst.get("norm", 0.0), abs(st["norm"] - o["norm"]) / b["norm"])
    return worst


MUTATIONS = {"eps 1e-8": ("main", dict(eps=1e-8)),
             "amsgrad off": ("main", dict(amsgrad=False)),
             "decay on every element": ("main", dict(decay_all=True)),
             "gscale ignored": ("main", dict(use_gscale=False)),
             "clip without + 1e-6": ("tiny", dict(clip_eps=0.0)),
             "bias correction one step late": ("main", dict(t_shift=1)),
             "EMA before the parameter": ("main", dict(ema_first=True))}


@pytest.mark.parametrize("n", [63, 2048 * 3 + 5])
def test_optimizer_bound_notices_every_wrong_variant(n):
    """No kernel runs here.  The written-out float64 step equals the library's; each wrong variant exceeds the bound 10 times."""
    for schedule in SCHEDULES:
        inp, orc, bounds = oracle_for(n, schedule)
        own = formula_oracle(*inp[:4], schedule)
        for a, b in zip(own, orc):
            for k in ("p", "m", "v", "vmax", "ema"):
                assert float((a[k] - b[k]).abs().max()) <= 1e-13 * max(1.0, float(b[k].abs().max())), (schedule, k)
        assert max(excess(own, orc, bounds).values()) <= 1e-3
        regimes = [o["coef"] < 1.0 for o in orc]
        assert regimes == ([False] * 5 + [True] if schedule == "main" else [True, True]), regimes
        if schedule == "main":
            assert bool((orc[2]["vmax"] > orc[2]["v"]).any()) and bool((orc[3]["vmax"] > orc[3]["v"]).any())
    for name, (schedule, kw) in MUTATIONS.items():
        inp, orc, bounds = oracle_for(n, schedule)
        worst = excess(formula_oracle(*inp[:4], schedule, **kw), orc, bounds)
        k = max(worst, key=worst.get)
        print(f"n = {n}: {name}: {worst[k]:.3g}x the bound (in {k}); in p {worst['p']:.3g}x")
        assert worst[k] >= 10, (name, worst)


class Buffers:
    def __init__(self, p0, wd, gscale, with_ema=True):
        n = p0.numel()
        self.n = n
        self.p, self.wd, self.gscale = put(p0), put(wd), put(gscale)
        self.m, self.v, self.vmax = (torch.zeros(n, device=DEV) for _ in range(3))
        self.ema = self.p.clone() if with_ema else None
        self.lib = _lib.load()
        self.partial = torch.zeros(max(1, int(self.lib.gn_optim_blocks(n))), device=DEV, dtype=torch.float64)
        self.norm = torch.zeros(1, device=DEV)

    def step(self, g, t, max_norm, flag=None, flag_bit=0, n=None):
        ptr = _lib.ptr
        return self.lib.gn_adamw_ema_step_f32(ptr(self.p), ptr(g), ptr(self.gscale), ptr(self.wd), ptr(self.m), ptr(self.v),
                                              ptr(self.vmax), ptr(self.ema), self.n if n is None else n, ptr(self.partial),
                                              max_norm, LR, BETA1, BETA2, EPS, t, EMA_DECAY, ptr(self.norm), ptr(flag), flag_bit,
                                              _lib.stream())

    def state(self):
        torch.cuda.synchronize()
        return dict(p=self.p.cpu(), m=self.m.cpu(), v=self.v.cpu(), vmax=self.vmax.cpu(), ema=self.ema.cpu(), norm=float(self.norm))


@pytest.mark.parametrize("schedule", ["main", "tiny"])
@pytest.mark.parametrize("n", SIZES)
def test_fused_adamw_ema_matches_float64_adamw(n, schedule):
    """Every step of every size against torch.optim.AdamW in float64 within `optimizer_bounds`.
    Measured on MI355X, largest |error| / bound over steps and elements (printed at every run): p 0.35, m 0.17, v 0.33,
    vmax 0.33, ema 0.33, norm 0.46; the weakest wrong variant of the test above (amsgrad off) is 13.9 times the bound."""
    t0 = time.perf_counter()
    (p0, wd, gscale, grads, eps_block, zero_block), orc, bounds = oracle_for(n, schedule)
    t_oracle = time.perf_counter() - t0
    b = Buffers(p0, wd, gscale)
    states = []
    for t, (g, (_, max_norm)) in enumerate(zip(grads, SCHEDULES[schedule]), start=1):
        assert b.step(put(g), t, max_norm) == 0
        states.append(b.state())
    worst = excess(states, orc, bounds)
    print(f"n = {n} [{schedule}]: largest |error| / bound: " + ", ".join(f"{k} {r:.3f}" for k, r in worst.items())
          + f"; c_t = {[float('%.2g' % x['c_t']) for x in bounds]}  ({time.perf_counter() - t0:.2f} s, oracle {t_oracle:.2f} s)")
    assert max(worst.values()) <= 1.0, worst
    # the block whose gradient is 0 for ever: moments stay 0, the parameter only decays (and not at all without decay)
    last = states[-1]
    z = zero_block
    assert not bool(last["m"][z].any()) and not bool(last["v"][z].any()) and not bool(last["vmax"][z].any())
    no_decay = wd[z] == 0
    assert torch.equal(last["p"][z][no_decay], p0[z][no_decay])
    if bool((~no_decay).any()):
        ratio = last["p"][z][~no_decay].double() / p0[z][~no_decay].double()
        want = (1.0 - LR * WD) ** len(grads)
        assert float((ratio - want).abs().max()) <= 4 * len(grads) * U


def test_skip_path_counts_skipped_steps_and_leaves_everything_alone():
    n = SIZES[-1]
    (p0, wd, gscale, grads, _, _), orc, bounds = oracle_for(n, "main")
    GRAD = 2
    for bad_value in (float("inf"), float("nan")):
        b = Buffers(p0, wd, gscale)
        word = torch.zeros(1, dtype=torch.int32, device=DEV)
        g_bad = put(grads[0])
        g_bad[n - 1] = bad_value                        # the last element: the grid-stride tail of the last block
        before = {k: v.clone() for k, v in b.state().items() if k != "norm"}
        assert b.step(g_bad, 1, 10.0, flag=word, flag_bit=GRAD) == 0
        after = b.state()
        assert all(torch.equal(before[k], after[k]) for k in before), bad_value
        assert not math.isfinite(after["norm"]) and int(word) == GRAD | 256
        assert b.step(g_bad, 1, 10.0, flag=word, flag_bit=GRAD) == 0
        after = b.state()
        assert all(torch.equal(before[k], after[k]) for k in before) and int(word) == GRAD | 512
        # a finite step afterwards: the normal update (step 1: the skipped calls did not count), the word stays
        assert b.step(put(grads[0]), 1, 10.0, flag=word, flag_bit=GRAD) == 0
        assert max(excess([b.state()], orc[:1], bounds[:1]).values()) <= 1.0
        assert int(word) == GRAD | 512
    # without a flag word a non-finite norm is not intercepted (documented: the reference writes NaN too): only the return code
    b = Buffers(p0[:63], wd[:63], gscale[:63])
    g_bad = put(grads[0][:63])
    g_bad[62] = float("inf")
    assert b.step(g_bad, 1, 10.0) == 0
    torch.cuda.synchronize()


def test_step_zero_is_an_error_and_an_empty_buffer_a_no_op():
    (p0, wd, gscale, grads, _, _), _, _ = oracle_for(63, "main")
    b = Buffers(p0, wd, gscale)
    before = b.state()
    assert b.step(put(grads[0]), 0, 10.0) != 0
    assert b.step(put(grads[0]), 1, 10.0, n=0) == 0
    after = b.state()
    assert all(torch.equal(before[k], after[k]) for k in ("p", "m", "v", "vmax", "ema"))


# =====================================================================================================================
# the parameter groups FusedAdamWEMA packs
# =====================================================================================================================
def test_fused_optimizer_packs_the_parameter_groups_of_make_optimizer():
    from gemnet_pytorch_amd.model.gemnet import GemNet
    from gemnet_pytorch_amd.training.ddp import make_optimizer
    from gemnet_pytorch_amd.training.fused_optim import FusedAdamWEMA
    from test_gpu_rangeflag import CFG
    torch.manual_seed(3)
    model = GemNet(**CFG, scale_file=SCALE_FILE).to(DEV).train()
    wd_value = 0.03
    fused = FusedAdamWEMA(model, lr=1e-3, weight_decay=wd_value)
    groups = make_optimizer(model, weight_decay=wd_value).param_groups
    decayed = {id(p) for p in groups[0]["params"]}
    plain = {id(p) for p in groups[1]["params"]}
    assert groups[0]["weight_decay"] == wd_value and groups[1]["weight_decay"] == 0.0
    nb = model.num_blocks
    scale_of = {id(l.weight): 1.0 / nb for l in (model.mlp_rbf3, model.mlp_cbf3, model.mlp_rbf_h)}
    scale_of[id(model.mlp_rbf_out.weight)] = 1.0 / (nb + 1)
    wd, gscale, flat_p = fused.wd.cpu(), fused.gscale.cpu(), fused.flat_p.cpu()
    covered = torch.zeros(fused.n, dtype=torch.bool)
    off = 0
    seen = dict(decay=0, plain=0, shared=0)
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        k = p.numel()
        assert p.data_ptr() == fused.flat_p.data_ptr() + 4 * off and p.grad.data_ptr() == fused.flat_g.data_ptr() + 4 * off, name
        assert (id(p) in decayed) != (id(p) in plain), name
        by_name = not any(s in name for s in ("atom_emb", "frequencies", "bias"))
        assert by_name == (id(p) in decayed), name
        assert bool((wd[off:off + k] == (F32(wd_value) if by_name else 0.0)).all()), name
        want = F32(scale_of.get(id(p), 1.0))
        assert bool((gscale[off:off + k] == want).all()), name
        seen["decay" if by_name else "plain"] += 1
        seen["shared"] += id(p) in scale_of
        covered[off:off + k] = True
        off += (k + 63) // 64 * 64
    assert off == fused.n and seen["decay"] > 0 and seen["plain"] > 0 and seen["shared"] == 4, seen
    gaps = ~covered
    assert bool(gaps.any()), "this configuration has tensors whose size is no multiple of 64"
    assert not bool(flat_p[gaps].any()) and not bool(wd[gaps].any()) and bool((gscale[gaps] == 1.0).all())
    # one step with a gradient in every parameter: the gaps stay 0, everything else moves
    gen = torch.Generator().manual_seed(5)
    for p in fused.params:
        p.grad.copy_(torch.randn(p.shape, generator=gen).to(DEV))
    assert not bool(fused.flat_g.cpu()[gaps].any())
    fused.step()
    torch.cuda.synchronize()
    after = fused.flat_p.cpu()
    assert not bool(after[gaps].any()) and bool((after[covered] != flat_p[covered]).all())
    assert not bool(fused.ema.cpu()[gaps].any())
