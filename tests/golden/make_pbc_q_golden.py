"""Generate tests/golden/pbc_q_cases.npz: energy, central-difference forces and stress of the periodic GemNet-Q cluster oracle
(tests/pbc_q_common.py: the project's own fp64 molecular oracle with triplets_only=False on a finite cluster of images,
radius 3 cutoff + int_cutoff + 0.5) for the structures of `pbc_q_common.GOLDEN_CASES` and both parameter sets — 'q' (P.CFG
widths: Y_lm rows) and 'ang' (emb_size_quad = emb_size_sbf = 32: the angle form).  h = 1e-4, the recipe of
`pbc_common.fd_forces_stress`.  Needs nothing but this repository:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pbc_q_golden.py

tests/test_pbc_q_cpu.py recomputes one stored case from the oracle and checks the radius-independence of the energies."""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _case(job):
    import torch
    torch.set_num_threads(1)
    import pbc_common as P
    import pbc_q_common as Q
    tag, kind = job
    cfg = Q.CFGS[tag]
    params = Q.make_params(cfg)
    R, Z, cell, pbc = P.structure(kind)
    E = Q.cluster_energy(params, R, Z, cell, pbc, cfg)
    F, S = Q.fd_forces_stress(params, R, Z, cell, pbc, cfg)
    return f"{tag}.{kind}", dict(R=R, Z=Z, cell=cell, pbc=pbc, E=np.array(E), F=F, S=S)


def main():
    from concurrent.futures import ProcessPoolExecutor
    import multiprocessing as mp
    import pbc_q_common as Q
    jobs = [(tag, kind) for tag, kinds in Q.GOLDEN_CASES.items() for kind in kinds]
    out = {}
    with ProcessPoolExecutor(max_workers=len(jobs), mp_context=mp.get_context("spawn")) as pool:
        for name, res in pool.map(_case, jobs):
            for k, v in res.items():
                out[f"{name}.{k}"] = v
            print(name, "E", float(res["E"]), "|F|max", float(np.abs(res["F"]).max()), "S diag", np.diag(res["S"]), flush=True)
    np.savez_compressed(os.path.join(HERE, "pbc_q_cases.npz"), **out)
    print("pbc_q_cases.npz", len(out), "arrays")


if __name__ == "__main__":
    main()
