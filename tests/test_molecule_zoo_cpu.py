"""The recipe of tests/molecule_zoo.py, pinned: the structural facts that make the zoo hard (atoms of degree 0 and 1, edges
without triplets / quadruplets, atoms only the interaction cutoff reaches, an atom count off the 16-row tiles) with their exact
counts, and the float32 ORACLE held to every bar tests/test_gpu_molecule_zoo.py sets for the HIP path — the guarantee that
those bars are about the kernels and not about the fixture."""
import numpy as np
import pytest
import torch

import molecule_zoo as MZ

COUNTS = {
    "T": dict(atoms=109, edges=968, triplets=13184, degree0=4, degree1=6, edges_without_triplet=6),
    "Q": dict(atoms=76, edges=392, triplets=2840, degree0=4, degree1=6, edges_without_triplet=6, int_edges=564,
              intm_triplets=4002, quadruplets=29188, edges_without_quadruplet=6, degree0_with_int_edges=3),
}


def _facts(kind):
    b = {k: v.numpy() for k, v in MZ.batch(kind).items()}
    A, E = len(b["Z"]), len(b["id_a"])
    deg = np.bincount(b["id_a"], minlength=A)
    out = dict(atoms=A, edges=E, triplets=len(b["id3_reduce_ca"]), degree0=int((deg == 0).sum()), degree1=int((deg == 1).sum()),
               edges_without_triplet=int((np.bincount(b["id3_reduce_ca"], minlength=E) == 0).sum()))
    if kind == "Q":
        assert len(b["id4_reduce_intm_ca"]) == len(b["id4_expand_intm_db"])
        out.update(int_edges=len(b["id4_int_a"]), intm_triplets=len(b["id4_reduce_intm_ca"]), quadruplets=len(b["id4_reduce_ca"]),
                   edges_without_quadruplet=int((np.bincount(b["id4_reduce_ca"], minlength=E) == 0).sum()))
    return out, deg, b


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_the_zoo_is_sparse_and_degenerate(kind):
    facts, deg, b = _facts(kind)
    assert facts["degree0"] >= 1 and facts["degree1"] >= 1 and facts["edges_without_triplet"] >= 1
    assert facts["atoms"] % 16 != 0
    if kind == "Q":
        assert facts["edges_without_quadruplet"] >= 1
        int_deg = np.bincount(b["id4_int_a"], minlength=facts["atoms"])
        facts["degree0_with_int_edges"] = int(((deg == 0) & (int_deg > 0)).sum())
        assert facts["degree0_with_int_edges"] >= 1                  # only the 10 A cutoff reaches these atoms
    assert facts == COUNTS[kind]


def test_recipe_details():
    z = MZ.zoo()
    assert list(z) == ["atom", "dimer", "far_dimer", "trimer_open", "linear4", "chain12", "chain17", "cluster+far", "two_clusters",
                       "dense15", "dense33"]
    assert MZ.names("Q") == list(z)[:-1]
    for R, Z in z.values():
        assert R.dtype == np.float64 and np.array_equal(R, R.astype(np.float32).astype(np.float64))
        assert set(Z.tolist()) <= {1, 6, 8, 93}
    assert z["dense15"][1][0] == 93 and [len(z[n][0]) for n in ("chain17", "cluster+far", "two_clusters")] == [17, 9, 11]
    assert np.array_equal(z["linear4"][0][:, 0], np.array([0, 1.1, 2.2, 3.3], np.float32).astype(np.float64))
    d = lambda R, i, j: float(np.linalg.norm(R[i] - R[j]))                # noqa: E731
    assert d(z["dimer"][0], 0, 1) < 5.0 and d(z["far_dimer"][0], 0, 1) == 7.5
    R = z["trimer_open"][0]
    assert d(R, 0, 1) < 5.0 and d(R, 1, 2) < 5.0 and 5.0 < d(R, 0, 2) < 10.0      # the end atoms do not see each other
    R = z["cluster+far"][0]
    assert 5.0 < min(d(R, 8, i) for i in range(8)) < 10.0                 # degree 0, inside the interaction cutoff
    R = z["two_clusters"][0]
    assert min(d(R, i, j) for i in range(6) for j in range(6, 11)) > 5.0      # joined by interaction edges only
    # another seed: the same molecule sizes, other edge and triplet counts (what the padded runner is fed)
    a, b = MZ.batch("T", seed=5), MZ.batch("T", seed=6)
    assert torch.equal(a["N"], b["N"]) and len(a["id_a"]) != len(b["id_a"]) and len(a["id3_reduce_ca"]) != len(b["id3_reduce_ca"])
    for k in ("atom", "far_dimer", "linear4"):
        assert np.array_equal(MZ.zoo(6)[k][0], z[k][0])


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_structures_without_an_embedding_edge_have_exactly_zero_energy_and_force(kind):
    ref, rw = MZ.reference(kind, 2), MZ.rows(kind)
    for n in ("atom", "far_dimer"):
        assert float(ref["E"][rw[n][0], 0]) == 0.0 and not ref["F"][rw[n][1]].any()
    far = rw["cluster+far"][1].stop - 1
    assert not ref["F"][far].any()          # (Q too: an interaction pair without a neighbour on both ends carries no quadruplet)
    assert 0.3 <= float(np.abs(ref["F"]).mean()) <= 1.6


@pytest.mark.parametrize("num_blocks", [2, 4])
@pytest.mark.parametrize("kind", ["T", "Q"])
def test_float32_oracle_meets_the_force_and_energy_bars(kind, num_blocks):
    ref = MZ.reference(kind, num_blocks)
    assert abs(float(np.abs(ref["F"]).mean()) - 1.0) < 1e-9
    got = MZ.run_oracle(kind, num_blocks, False, dtype=torch.float32)
    MZ.assert_force_energy(MZ.force_energy_figures(got["E"], got["F"], ref, kind), f"float32 oracle {kind} x{num_blocks}")


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_float32_oracle_meets_the_gradient_bars_and_every_parameter_gets_a_gradient(kind):
    ref = MZ.reference(kind, 2, True)
    assert all(g is not None and float(g.norm()) > 0 for g in ref["grads"].values())
    got = MZ.run_oracle(kind, 2, True, dtype=torch.float32)
    assert abs(got["loss"] - ref["loss"]) <= MZ.LOSS_RTOL * abs(ref["loss"])
    worst, name, rel = MZ.grad_figures(got["grads"], ref)
    print(f"float32 oracle {kind}: loss {got['loss']:.6f}; worst gradient error {worst:.3f} of its bar ({name}), "
          f"worst ||g32 - g64|| / ||g64|| = {rel:.2e}")
    assert worst <= 1.0, name


@pytest.mark.parametrize("kind", ["T", "Q"])
def test_module_wiring_takes_batches_without_edges(kind):
    """The GemNet module above the C ABI (launchers emulated by tests/cpu_kernels.py, float64) on `atom`, `far_dimer` and `dimer`
    as batches of their own — E = 0, resp. no triplet — in eval and in training mode: the oracle's rows, exact zeros included."""
    import cpu_kernels
    from test_model_cpu import build
    cfg, ref = MZ.cfg_full(kind, 2), MZ.reference(kind, 2)
    with cpu_kernels.emulate():
        for train in (False, True):
            model = build(cfg, MZ.params(cfg))
            model = model.train() if train else model.eval()
            for n in ("atom", "far_dimer", "dimer"):
                E, F = model(MZ.batch(kind, only=[n]))
                if train:
                    (E.sum() + (F ** 2).sum()).backward()
                E, F = E.detach().numpy(), F.detach().numpy()
                fig = MZ.force_energy_figures(E, F, ref, kind, sel=[n])
                assert fig["f_max"] <= 1e-12 and fig["e_err"] <= 1e-12, (n, train, fig)
                assert n == "dimer" or not (E.any() or F.any())


@pytest.mark.parametrize("defect", ["nan", "inf", "missing", "one-nan-element"])
def test_gradient_figures_do_not_lose_a_bad_gradient_in_the_middle(defect):
    """The helper behind every gradient assertion of the zoo: a NaN / inf / missing gradient on a MIDDLE parameter (finite,
    exact ones before and after it) must come out as a ratio above 1 under that parameter's name, and a NaN must not drop out
    of the relative figure either."""
    g = torch.Generator().manual_seed(3)
    ref = {"grads": {k: torch.randn(4, 5, generator=g, dtype=torch.float64) for k in "abcde"}}
    grads = {k: v.float() for k, v in ref["grads"].items()}
    worst, _, rel = MZ.grad_figures(grads, ref)
    assert worst <= 1e-3 and rel <= 1e-6                      # fp32 copies of the reference pass
    if defect == "missing":
        del grads["c"]
    elif defect == "one-nan-element":
        grads["c"] = grads["c"].clone()
        grads["c"][2, 3] = float("nan")
    else:
        grads["c"] = torch.full((4, 5), float(defect))
    worst, name, rel = MZ.grad_figures(grads, ref)
    assert worst > 1.0 and name == "c", (worst, name)
    assert rel >= 1.0
    if defect != "missing":
        assert worst == float("inf") and rel == float("inf")


def test_force_figures_do_not_lose_a_nan_structure():
    """The per-structure figure stands on its own: NaN forces on one structure in the middle name that structure."""
    ref = MZ.reference("T", 2)
    E, F = ref["E"].copy(), ref["F"].copy()
    F[MZ.rows("T")["linear4"][1]] = np.nan
    fig = MZ.force_energy_figures(E, F, ref, "T")
    assert fig["worst"] == ("linear4", float("inf"))
    with pytest.raises(AssertionError):
        MZ.assert_force_energy(fig, "nan forces")
