"""Exactly planar and exactly linear molecules in general orientation (numpy / fp64 oracle): every other molecular fixture is a
random point cloud or lies along an axis.  In fp32 the cross products of an exactly degenerate quadruplet are rounding residues
of relative size 1e-7 once the molecule is rotated off the axes — far above the reference's absolute max(|u x v|, 1e-9) — so the
molecular kernels have to take their clamp decisions relative to the vectors (csrc/quad_math.h).

The reference is the float64 oracle on the UNROUNDED AXIS-ALIGNED coordinates (where the degeneracies are exact and sit on the
reference's clamp), carried over by the rotation: E unchanged, F @ Q.T.  The oracle is never run on rotated or rounded
coordinates: float64 on them sees the 1e-7 residues and differentiates them.  docs/SYMMETRIC_MOLECULES.md has the recipes and
the counts; tests/test_symmetric_molecules_cpu.py pins them."""
import functools

import numpy as np
import torch

import molecule_zoo as MZ
from oracle import gemnet_oracle as GO
from oracle import index_oracle as IO

MOLECULES = ("planar9", "linear5", "benzene")
ORIENTATIONS = ("axis", "rot3", "rot11")
SHIFT = np.array([0.3, -1.2, 2.1])
# the first seed from 4 upwards that meets every condition of tests/test_symmetric_molecules_cpu.py (seed 4 has a triplet with
# sin = 0.00996; 64 ... 548 are well conditioned but carry mean|F_ref| of 1.7 ... 6 under the zoo's weights)
PLANAR_SEED = 550
R_C, R_H = 1.39, 2.48                   # benzene: the radii of the carbon and the hydrogen hexagon
TRAIN = ("planar9", "linear5")          # the molecules that have a force reference


@functools.lru_cache(maxsize=None)
def _coordinates(name):
    if name == "planar9":
        rs, pts = np.random.RandomState(PLANAR_SEED), []
        while len(pts) < 9:
            p = rs.uniform(0, 4.5, 2)
            if all(np.linalg.norm(p - q) >= 0.95 for q in pts):
                pts.append(p)
        R = np.concatenate([np.array(pts), np.zeros((9, 1))], axis=1)
        Z = [6, 1, 8, 6, 1, 1, 8, 6, 1]
    elif name == "linear5":
        R = np.zeros((5, 3))
        R[:, 0] = [0, 1.16, 2.32, 3.4, 4.6]
        Z = [8, 6, 8, 6, 1]
    elif name == "benzene":
        # a regular hexagon with exact half-integers in x: para atoms are exact negatives of each other
        h = np.sqrt(3.0) / 2
        ring = np.array([(1, 0, 0), (0.5, h, 0), (-0.5, h, 0), (-1, 0, 0), (-0.5, -h, 0), (0.5, -h, 0)])
        R = np.concatenate([R_C * ring, R_H * ring])
        Z = [6] * 6 + [1] * 6
    else:
        raise KeyError(name)
    return R, np.array(Z, np.int64)


def coordinates(name):
    """-> R (n, 3) float64 (unrounded, axis-aligned: z = 0, resp. y = z = 0, exactly), Z (n,)."""
    R, Z = _coordinates(name)
    return R.copy(), Z.copy()


def rotation(orient):
    """-> Q (3, 3) proper rotation, shift (3,): a placed molecule is R @ Q.T + shift."""
    if orient == "axis":
        return np.eye(3), np.zeros(3)
    Q, _ = np.linalg.qr(np.random.RandomState(int(orient[3:])).randn(3, 3))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q, SHIFT.copy()


def placed(name, orient, rounded=True):
    """The coordinates the model receives: rotated in float64, shifted and (rounded) rounded through float32."""
    R, _ = coordinates(name)
    Q, s = rotation(orient)
    R = R @ Q.T + s
    return R.astype(np.float32).astype(np.float64) if rounded else R


def inputs_of(names, orient, kind, dtype=torch.float64, rounded=True):
    """The model's input dict (CPU tensors) of the batch of `names` in one orientation, with the oracle's index lists."""
    R = np.concatenate([placed(n, orient, rounded) for n in names])
    Z = np.concatenate([coordinates(n)[1] for n in names])
    N = np.array([len(coordinates(n)[1]) for n in names], np.int64)
    return MZ.inputs_of(R, Z, N, kind, dtype)


def all_nine(kind, dtype=torch.float64):
    """One batch of every molecule in every orientation (molecule-major) -> inputs, [(name, orient)]."""
    order = [(n, o) for n in MOLECULES for o in ORIENTATIONS]
    R = np.concatenate([placed(n, o) for n, o in order])
    Z = np.concatenate([coordinates(n)[1] for n, _ in order])
    N = np.array([len(coordinates(n)[1]) for n, _ in order], np.int64)
    return MZ.inputs_of(R, Z, N, kind, dtype), order


def index_lists(name, orient, kind="Q"):
    R = placed(name, orient)
    return IO.build_indices(R, np.array([len(R)], np.int64), MZ.CUTOFF, MZ.INT_CUTOFF, kind == "T")


def quad_atoms(idx):
    """The four atoms (c, a, b, d) of every quadruplet c -> a - b <- d of an index dict, int32 tensors."""
    id_c, id_a = np.asarray(idx["id_c"]), np.asarray(idx["id_a"])
    ca, db = np.asarray(idx["id4_reduce_ca"]), np.asarray(idx["id4_expand_db"])
    return tuple(torch.tensor(x.astype(np.int32)) for x in (id_c[ca], id_a[ca], id_a[db], id_c[db]))


def trip_atoms(idx):
    """The three atoms (c, a, b) of every triplet c -> a <- b, int32 tensors."""
    id_c, id_a = np.asarray(idx["id_c"]), np.asarray(idx["id_a"])
    ca, ba = np.asarray(idx["id3_reduce_ca"]), np.asarray(idx["id3_expand_ba"])
    return tuple(torch.tensor(x.astype(np.int32)) for x in (id_c[ca], id_a[ca], id_c[ba]))


def params(kind, dtype=torch.float64):
    cfg = MZ.cfg_full(kind, 2)
    return cfg, {k: v.to(dtype) for k, v in MZ.params(cfg).items()}


def run_oracle(name, orient, kind, dtype=torch.float64, rounded=True):
    cfg, P = params(kind, dtype)
    E, F = GO.forward(cfg, P, inputs_of([name], orient, kind, dtype, rounded))
    return E.detach().double().numpy(), F.detach().double().numpy()


@functools.lru_cache(maxsize=None)
def axis_reference(name, kind):
    """E (1, 1), F (n, 3): the float64 oracle on the unrounded axis-aligned coordinates, once per process.  The forces of
    `benzene` under GemNet-Q are NOT a reference (float64 autograd differentiates atan2(1e-9, ~1e-16) on its collinear rows)."""
    return run_oracle(name, "axis", kind, rounded=False)


def reference(name, orient, kind):
    """-> E (1, 1), F (n, 3) in the orientation's frame; F is None where no force reference exists."""
    E, F = axis_reference(name, kind)
    if name == "benzene" and kind == "Q":
        return E, None
    return E, F @ rotation(orient)[0].T


def force_energy_figures(E, F, name, orient, kind):
    """The figures of molecule_zoo.force_energy_figures for one molecule (F against a reference only where one exists)."""
    Er, Fr = reference(name, orient, kind)
    fig = dict(e_err=MZ._sticky(float(np.abs(E - Er).max())), e_bar=MZ.ENERGY_TOL * max(1.0, float(np.abs(Er).max())),
               finite=bool(np.isfinite(F).all()))
    if Fr is not None:
        fmean = float(np.abs(Fr).mean())
        fig.update(f_mae=MZ._sticky(float(np.abs(F - Fr).mean())), f_max=MZ._sticky(float(np.abs(F - Fr).max())), fmean=fmean,
                   scale=max(1.0, fmean))
    return fig


def assert_force_energy(fig, tag):
    """molecule_zoo's bars; per molecule the force bars scale with max(1, mean|F_ref|), as its per-structure figure does."""
    if "f_mae" in fig:
        print(f"{tag}: force MAE {fig['f_mae']:.3e} (max {fig['f_max']:.3e}; mean|F_ref| {fig['fmean']:.3f}), energy err "
              f"{fig['e_err']:.3e} (bar {fig['e_bar']:.1e})")
    else:
        print(f"{tag}: energy err {fig['e_err']:.3e} (bar {fig['e_bar']:.1e}); no force reference")
    assert fig["finite"], tag
    assert fig["e_err"] <= fig["e_bar"], tag
    if "f_mae" in fig:
        assert fig["f_mae"] <= MZ.FORCE_TOL * fig["scale"], tag
        assert fig["f_max"] <= MZ.FORCE_MAX_TOL * fig["scale"], tag


# ------------------------------------------------------------------------------------------- training on planar9 + linear5
def train_targets(orient, seed=204):
    """E ~ N(0, 1) (drawn first) and F ~ N(0, 1) in the axis frame, float32 values held in float64; the force targets turn
    with the molecule, so the loss and every parameter gradient are those of the axis frame."""
    n = sum(len(coordinates(m)[1]) for m in TRAIN)
    rs = np.random.RandomState(seed)
    Et = rs.standard_normal((len(TRAIN), 1)).astype(np.float32).astype(np.float64)
    Ft = rs.standard_normal((n, 3)).astype(np.float32).astype(np.float64)
    return torch.tensor(Et), torch.tensor(Ft @ rotation(orient)[0].T)


def run_training_oracle(kind, orient="axis", dtype=torch.float64, rounded=False):
    cfg, P = params(kind, dtype)
    names_ = [k for k, v in P.items() if v.dim() > 0]
    for k in names_:
        P[k].requires_grad_(True)
    E, F = GO.forward(cfg, P, inputs_of(TRAIN, orient, kind, dtype, rounded), create_graph=True)
    Et, Ft = train_targets(orient)
    loss = GO.training_loss(E[:, :1], F, Et.to(dtype), Ft.to(dtype))
    g = torch.autograd.grad(loss, [P[k] for k in names_], allow_unused=True)
    return dict(loss=float(loss.detach()), grads={k: (None if v is None else v.detach().double()) for k, v in zip(names_, g)})


@functools.lru_cache(maxsize=None)
def training_reference(kind):
    """Loss and parameter gradients (second order) of the float64 oracle on the unrounded axis-aligned batch."""
    return run_training_oracle(kind)


# ------------------------------------------------------------------- a narrow GemNet-Q: the widths no fused quadruplet path takes
def cfg_narrow():
    """The published widths except the quadruplet branch (emb_size_quad = emb_size_sbf = 16): the model then evaluates the
    explicit (Q, 49) harmonics in eval mode and the ATen composite closure (GemNet.calculate_angles) in training mode."""
    return dict(MZ.cfg_full("Q", 2), emb_size_quad=16, emb_size_sbf=16, emb_size_bil_quad=16)


@functools.lru_cache(maxsize=None)
def narrow_reference(name="planar9"):
    """-> params (heads scaled to mean|F_ref| = 1 on `name`), E (1, 1), F (n, 3) of the float64 oracle on the exact axis-aligned
    coordinates."""
    cfg = cfg_narrow()
    P = MZ._raw_params(cfg, 7)
    inputs = inputs_of([name], "axis", "Q", rounded=False)
    _, F = GO.forward(cfg, P, inputs)
    sc = 1.0 / float(F.detach().abs().mean())
    P = {k: (v * sc if k.endswith(MZ.HEAD_KEYS) else v) for k, v in P.items()}
    E, F = GO.forward(cfg, P, inputs)
    return P, E.detach().double().numpy(), F.detach().double().numpy()
