"""Sparse and degenerate molecules for the full-width molecular models (numpy / fp64 oracle): a batch whose atoms have degree
0, 1 and 2 next to dense clusters, edges without triplets or quadruplets, one-atom molecules, molecules without an embedding
edge, and atoms that only the 10 A interaction cutoff reaches.  Every other molecular fixture at these widths comes from
`synthetic.make_molecule` (random points at >= 0.9 A in a box of <= 7 A under a 5 A cutoff: every atom has many neighbours).
docs/MOLECULE_ZOO.md has the recipe and the counts; tests/test_molecule_zoo_cpu.py pins them."""
import functools

import numpy as np
import torch

from conftest import SCALE_FILE
from gemnet_pytorch_amd.synthetic import make_molecule
from oracle import gemnet_oracle as GO
from oracle import index_oracle as IO

CUTOFF, INT_CUTOFF = 5.0, 10.0
HEAD_KEYS = ("out_energy.weight", "out_forces.weight")
Q_LEAVES_OUT = ("dense33",)          # keeps the quadruplet count near 3e4


def cfg_full(kind, num_blocks=2):
    """The published widths (`cfg_full` of tests/golden/make_golden.py, restated): what the fused kernels take."""
    return dict(num_spherical=7, num_radial=6, num_blocks=num_blocks, emb_size_atom=128, emb_size_edge=128, emb_size_trip=64,
                emb_size_quad=32, emb_size_rbf=16, emb_size_cbf=16, emb_size_sbf=32, emb_size_bil_quad=32, emb_size_bil_trip=64,
                num_before_skip=1, num_after_skip=1, num_concat=1, num_atom=2, triplets_only=(kind == "T"))


def zoo(seed=5):
    """-> {name: (R (n, 3) float64 rounded through float32, Z (n,) int64)} in the order of docs/MOLECULE_ZOO.md.  The jitter is
    0.15 * RandomState(seed).standard_normal, drawn in this order; Z comes from {1, 6, 8} by RandomState(seed + 100), and the
    first atom of `dense15` is Z = 93 (the last row of the embedding tables).  The `make_molecule` seeds are those of the document
    at seed 5 and move by 100 per unit of `seed`: another seed keeps every molecule's size and changes the list lengths."""
    rs, rz = np.random.RandomState(seed), np.random.RandomState(seed + 100)
    jit = lambda pts: np.asarray(pts, np.float64) + 0.15 * rs.standard_normal((len(pts), 3))      # noqa: E731
    chain = lambda n, d: [[d * i, 0.9 * (i % 2), 0.4 * ((i // 2) % 2)] for i in range(n)]           # noqa: E731
    mol = lambda n, s, **kw: make_molecule(n, s + 100 * (seed - 5), **kw)["R"].astype(np.float64)   # noqa: E731
    out = {}
    out["atom"] = np.zeros((1, 3))
    out["dimer"] = jit([(0, 0, 0), (1.2, 0, 0)])
    out["far_dimer"] = np.array([(0, 0, 0), (7.5, 0, 0)], np.float64)
    out["trimer_open"] = jit([(0, 0, 0), (3, 0, 0), (6.5, 0.5, 0)])
    out["linear4"] = np.array([(0, 0, 0), (1.1, 0, 0), (2.2, 0, 0), (3.3, 0, 0)], np.float64)
    out["chain12"] = jit(chain(12, 3.0))
    out["chain17"] = jit(chain(17, 2.0))
    out["cluster+far"] = np.concatenate([mol(8, 11, box=3.5), [[11.0, 1.0, 1.0]]])
    out["two_clusters"] = np.concatenate([mol(6, 12, box=3.0), mol(5, 13, box=3.0) + np.array([9.5, 0.0, 0.0])])
    out["dense15"] = mol(15, 14)
    out["dense33"] = mol(33, 15)
    res = {}
    for name, R in out.items():
        Z = rz.choice(np.array([1, 6, 8]), size=len(R)).astype(np.int64)
        if name == "dense15":
            Z[0] = 93
        res[name] = (np.asarray(R, np.float32).astype(np.float64), Z)
    return res


def names(kind):
    return [n for n in zoo() if kind == "T" or n not in Q_LEAVES_OUT]


def arrays(kind, seed=5, only=None):
    """-> R (A, 3) float64, Z (A,), N (B,) of the zoo batch of a kind ("T" / "Q"), or of the structures named in `only`."""
    z = zoo(seed)
    use = names(kind) if only is None else list(only)
    return (np.concatenate([z[n][0] for n in use]), np.concatenate([z[n][1] for n in use]),
            np.array([len(z[n][0]) for n in use], np.int64))


def rows(kind):
    """{name: (molecule number, slice of its atoms)} in the zoo batch of a kind."""
    out, off = {}, 0
    z = zoo()
    for b, n in enumerate(names(kind)):
        out[n] = (b, slice(off, off + len(z[n][0])))
        off += len(z[n][0])
    return out


def inputs_of(R, Z, N, kind, dtype=torch.float64):
    """The model's input dict (CPU tensors) with the index lists of oracle.index_oracle."""
    idx = IO.build_indices(R, N, CUTOFF, INT_CUTOFF, kind == "T")
    inputs = {k: torch.tensor(v) for k, v in idx.items()}
    inputs.update(Z=torch.tensor(Z).long(), R=torch.tensor(R, dtype=dtype), N=torch.tensor(N).long())
    return inputs


def batch(kind, seed=5, only=None, dtype=torch.float64):
    return inputs_of(*arrays(kind, seed, only), kind, dtype)


def _raw_params(cfg, seed):
    return GO.make_params(cfg, seed, GO.load_scale_factors(SCALE_FILE), standardize=True)


@functools.lru_cache(maxsize=None)
def out_scale(kind, num_blocks, seed=7):
    """1 / mean|F| of the zoo batch under the generated weights (float64): the factor on the output heads."""
    _, F = GO.forward(cfg_full(kind, num_blocks), _raw_params(cfg_full(kind, num_blocks), seed), batch(kind))
    return 1.0 / float(F.detach().abs().mean())


def params(cfg, seed=7):
    """Standardised generator weights with the project's scale factors; the output heads (E and F are linear in them) times
    `out_scale`, which brings mean|F| of the zoo batch to 1 so that the 1e-5 force bar is literal."""
    sc = out_scale("T" if cfg["triplets_only"] else "Q", cfg["num_blocks"], seed)
    return {k: (v * sc if k.endswith(HEAD_KEYS) else v) for k, v in _raw_params(cfg, seed).items()}


def targets(kind, seed=104):
    """Training targets E ~ N(0, 1) (drawn first) and F ~ N(0, 1), float32 values held in float64."""
    R, _, N = arrays(kind)
    rs = np.random.RandomState(seed)
    Et = rs.standard_normal((len(N), 1)).astype(np.float32).astype(np.float64)
    Ft = rs.standard_normal(R.shape).astype(np.float32).astype(np.float64)
    return torch.tensor(Et), torch.tensor(Ft)


def run_oracle(kind, num_blocks, grads, dtype=torch.float64):
    """`GO.forward` on the zoo batch in `dtype` -> dict of float64 numpy E (B, 1), F (A, 3) and, with grads, `loss` and
    `grads` {name: tensor} of `GO.training_loss` against `targets` (second order: through the force)."""
    cfg = cfg_full(kind, num_blocks)
    P = {k: v.to(dtype) for k, v in params(cfg).items()}
    inputs = batch(kind, dtype=dtype)
    if not grads:
        E, F = GO.forward(cfg, P, inputs)
        return dict(E=E.detach().double().numpy(), F=F.detach().double().numpy())
    names_ = [k for k, v in P.items() if v.dim() > 0]
    for k in names_:
        P[k].requires_grad_(True)
    E, F = GO.forward(cfg, P, inputs, create_graph=True)
    Et, Ft = targets(kind)
    loss = GO.training_loss(E[:, :1], F, Et.to(dtype), Ft.to(dtype))
    g = torch.autograd.grad(loss, [P[k] for k in names_], allow_unused=True)
    return dict(E=E.detach().double().numpy(), F=F.detach().double().numpy(), loss=float(loss.detach()),
                grads={k: (None if v is None else v.detach().double()) for k, v in zip(names_, g)})


@functools.lru_cache(maxsize=None)
def reference(kind, num_blocks, grads=False):
    """The float64 oracle on the zoo batch, computed once per process and left unchanged."""
    return run_oracle(kind, num_blocks, grads)


# ----------------------------------------------------------------------------------------------------------------- the bars
FORCE_TOL = 1e-5          # force MAE at mean|F| = 1 (test_gpu_model.FORCE_TOL)
FORCE_MAX_TOL = 1e-4      # largest force error (test_gpu_pbc_cases)
ENERGY_TOL = 2e-5         # of max(1, max|E_ref|)
LOSS_RTOL = 2e-5
GRAD_RTOL, GRAD_ATOL = 2e-3, 1e-6     # ||g - g_ref|| <= GRAD_RTOL ||g_ref|| + GRAD_ATOL max_p ||g_ref,p||


def _sticky(x):
    """A figure that is not finite (a NaN or inf anywhere in what it was computed from) becomes +inf: it wins every `>` and
    `max` from then on and fails every `<= bar`, where a NaN would lose the comparisons and drop out."""
    return x if np.isfinite(x) else float("inf")


def force_energy_figures(E, F, ref, kind, sel=None):
    """Errors of E (B, 1), F (A, 3) (numpy, float64) against `ref`; `sel`: names of the structures E and F hold (default all).
    -> dict(f_mae, f_max, e_err, e_bar, fmean, worst=(name, MAE / bar of that structure))."""
    rw = rows(kind)
    use = names(kind) if sel is None else list(sel)
    Er = np.concatenate([ref["E"][rw[n][0]:rw[n][0] + 1] for n in use])
    Fr = np.concatenate([ref["F"][rw[n][1]] for n in use])
    assert E.shape == Er.shape and F.shape == Fr.shape, (E.shape, Er.shape, F.shape, Fr.shape)
    worst, off = ("", 0.0), 0
    for n in use:
        k = rw[n][1].stop - rw[n][1].start
        fr = Fr[off:off + k]
        ratio = _sticky(float(np.abs(F[off:off + k] - fr).mean()) / (FORCE_TOL * max(1.0, float(np.abs(fr).mean()))))
        if ratio > worst[1]:
            worst = (n, ratio)
        off += k
    return dict(f_mae=float(np.abs(F - Fr).mean()), f_max=float(np.abs(F - Fr).max()), e_err=float(np.abs(E - Er).max()),
                e_bar=ENERGY_TOL * max(1.0, float(np.abs(Er).max())), fmean=float(np.abs(Fr).mean()), worst=worst)


def assert_force_energy(fig, tag):
    print(f"{tag}: force MAE {fig['f_mae']:.3e} (max {fig['f_max']:.3e}; mean|F_ref| {fig['fmean']:.3f}), energy err "
          f"{fig['e_err']:.3e} (bar {fig['e_bar']:.1e}); worst structure {fig['worst'][0]} at {fig['worst'][1]:.3f} of its bar")
    assert np.isfinite(fig["f_mae"]) and np.isfinite(fig["e_err"])
    assert fig["f_mae"] <= FORCE_TOL, tag
    assert fig["f_max"] <= FORCE_MAX_TOL, tag
    assert fig["e_err"] <= fig["e_bar"], tag
    assert fig["worst"][1] <= 1.0, (tag, fig["worst"])


def grad_figures(grads, ref):
    """-> (worst ||g - g_ref|| / bar, its name, worst ||g - g_ref|| / ||g_ref||) over every parameter of ref["grads"]; a
    missing gradient counts as zero, a gradient with a NaN or inf in it as an infinite error (the first such parameter is named)."""
    gref = {k: v for k, v in ref["grads"].items() if v is not None}
    top = max(float(v.norm()) for v in gref.values())
    worst, name, rel = 0.0, "", 0.0
    for k, gr in gref.items():
        g = grads.get(k)
        g = torch.zeros_like(gr) if g is None else g.detach().double().cpu().reshape(gr.shape)
        err, nrm = float((g - gr).norm()), float(gr.norm())
        ratio = _sticky(err / (GRAD_RTOL * nrm + GRAD_ATOL * top))
        if ratio > worst:
            worst, name = ratio, k
        if nrm > 0:
            rel = max(rel, _sticky(err / nrm))
    return worst, name, rel
