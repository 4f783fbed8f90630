"""Generate tests/golden/pbc_q_train.npz and its gradient shards pbc_q_train.g<NN>.npy: the gradient oracle of periodic GemNet-Q
training (tests/pbc_q_train_common.py: the fp64 cluster oracle of tests/pbc_q_common.py, parameters as leaves, Richardson
directional derivatives along the loss cotangents) for make_params(seed=3), rho_force = 0.9, rho_stress = 0.05 and what
`pbc_q_train_common.STORED` lists: configuration CFG_QW on both batches of `BATCHES`, the narrow Q.CFG_Q on batch A.  Stored per
batch: E, F, S, the targets, the loss and `trunc`; as float64 gradients of CFG_QW (shards): batch A, the contribution of 'slab' to
it (recomputed by tests/test_pbc_q_train_cpu.py), batch B; the gradients of the narrow model inside the .npz.
Needs nothing but this repository (a few minutes on 8 cores):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pbc_q_train_golden.py
"""
import glob
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
THREADS = 3


def _setup(cfg):
    import torch
    torch.set_num_threads(THREADS)
    import pbc_q_train_common as QT
    return QT, QT.make_params(QT.CFGS[cfg])


def _names(QT, cfg, params):
    import pbc_train_common as PT
    from test_model_cpu import build
    with QT.emulate():
        return PT.trainable(build(QT.CFGS[cfg], params), params)


def _efs(job):
    cfg, tag, i = job
    QT, params = _setup(cfg)
    return job, QT.efs(params, QT.CFGS[cfg], QT.structures(tag)[i])


def _part(job):
    cfg, tag, i, gE, u, w = job
    QT, params = _setup(cfg)
    g, t = QT.contribution(params, QT.CFGS[cfg], _names(QT, cfg, params), QT.structures(tag)[i], gE, u, w)
    return (cfg, tag, i), {k: v.numpy() for k, v in g.items()}, t


def main():
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    import pbc_q_train_common as QT
    stored = [(cfg, tag) for cfg, tags in QT.STORED.items() for tag in tags]
    jobs = [(cfg, tag, i) for cfg, tag in stored for i in range(len(QT.BATCHES[tag]))]
    out, names = {}, {}
    for cfg in QT.STORED:
        params = QT.make_params(QT.CFGS[cfg])
        names[cfg] = sorted(_names(QT, cfg, params))
        if cfg == "qw":
            out["names"] = np.array(names[cfg])
            out["sizes"] = np.array([params[n].numel() for n in names[cfg]], np.int64)
            for n in names[cfg]:
                out[f"shape.{n}"] = np.array(params[n].shape, np.int64)
    with ProcessPoolExecutor(max_workers=min(len(jobs), (os.cpu_count() or 8) // 2), mp_context=mp.get_context("spawn")) as pool:
        res = dict(pool.map(_efs, jobs))
        second = []
        for cfg, tag in stored:
            structs, pre = QT.structures(tag), QT.prefix(cfg, tag)
            terms, (gE, u, w) = QT.loss_terms(*zip(*[res[(cfg, tag, i)] for i in range(len(structs))]), structs)
            for k in ("E", "F", "S", "Et", "Ft", "St"):
                out[f"{pre}.{k}"] = terms[k].numpy()
            out[f"{pre}.loss"] = np.array(terms["loss"])
            off = 0
            for i, s in enumerate(structs):
                second.append((cfg, tag, i, float(gE[i, 0]), u[off:off + len(s[0])], w[i]))
                off += len(s[0])
            print(pre, "loss", terms["loss"], flush=True)
        parts, trunc = {}, {}
        for key, g, t in pool.map(_part, second):
            parts[key], trunc[key] = g, t
    vectors = []
    for cfg, tag in stored:
        kinds, pre = QT.BATCHES[tag], QT.prefix(cfg, tag)
        total = {n: sum(parts[(cfg, tag, i)][n] for i in range(len(kinds))) for n in names[cfg]}
        gmax = max(float(np.linalg.norm(v)) for v in total.values())
        gmin = min(float(np.linalg.norm(v)) for v in total.values())
        out[f"{pre}.trunc"] = np.array(max(trunc[(cfg, tag, i)] for i in range(len(kinds))) / gmax)
        print(pre, "trunc", float(out[f"{pre}.trunc"]), "max |g|", gmax, "min |g| / max |g|", gmin / gmax, flush=True)
        if cfg != "qw":          # a narrow model's gradients are small: they go into the .npz
            for n in names[cfg]:
                out[f"{pre}.grad.{n}"] = total[n]
            continue
        vectors.append(QT.flatten(total, names[cfg]))
        if tag == "A":
            vectors.append(QT.flatten(parts[(cfg, "A", kinds.index("slab"))], names[cfg]))
    assert len(vectors) == len(QT.VECTORS)
    flat = np.concatenate(vectors)
    stem = QT.GOLDEN[:-4]
    for f in glob.glob(stem + ".g*.npy"):
        os.remove(f)
    for k, start in enumerate(range(0, len(flat), QT.SHARD)):
        np.save(f"{stem}.g{k:02d}.npy", flat[start:start + QT.SHARD])
    np.savez_compressed(QT.GOLDEN, **out)
    print("pbc_q_train.npz", len(out), "arrays;", k + 1, "gradient shards of", QT.SHARD, "float64")


if __name__ == "__main__":
    main()
