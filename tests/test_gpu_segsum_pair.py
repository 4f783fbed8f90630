"""-m gpu: gn_segsum_pair_f32 (two CSR segmented sums of the same rows in one launch) against two gn_segsum_rows_f32
launches — bit for bit, since the per-row order of addition is the single launch's — and against float64."""
import pytest
import torch

from gemnet_pytorch_amd import kernels as K
from gemnet_pytorch_amd.graph import RowIndex
from redzone import put, redzone  # noqa: F401  (autouse: every test of this module runs under the red-zone harness)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _keys(kind, M, n_rows, g):
    if kind == "random":          # with n_rows > M some segments are empty
        return torch.randint(0, n_rows, (M,), generator=g)
    if kind == "one":             # one segment holds every row, the others are empty
        return torch.full((M,), n_rows // 2, dtype=torch.int64)
    if kind == "sorted":          # no permutation (perm = None) on this side
        return torch.sort(torch.randint(0, n_rows, (M,), generator=g)).values
    raise ValueError(kind)


@pytest.mark.parametrize("C", [128, 4, 3])       # float4 rows, one float4, the scalar path
@pytest.mark.parametrize("M", [1, 17, 1000])
@pytest.mark.parametrize("kinds,n1,n2", [(("random", "random"), 37, 64), (("one", "random"), 5, 1), (("random", "one"), 1, 9),
                                         (("sorted", "random"), 2000, 33), (("random", "random"), 5000, 12)])
def test_pair_equals_two_single_launches(kinds, n1, n2, M, C):
    """n_rows = 1 on either side; 2000 rows for at most 1000 entries (mostly empty segments); 5000 rows on one side: beyond
    the workgroup-per-row form, where the entry point issues the two single launches itself."""
    g = torch.Generator().manual_seed(M * 131 + C)
    y = torch.randn(M, C, generator=g)
    k1, k2 = _keys(kinds[0], M, n1, g), _keys(kinds[1], M, n2, g)
    yd = put(y)
    p1, s1 = RowIndex(put(k1), n1).csr
    p2, s2 = RowIndex(put(k2), n2).csr
    want1, want2 = K.segsum(yd, p1, s1, n1), K.segsum(yd, p2, s2, n2)
    got1, got2 = K.segsum_pair(yd, p1, s1, n1, p2, s2, n2)
    assert got1.shape == (n1, C) and got2.shape == (n2, C)
    assert torch.equal(got1, want1) and torch.equal(got2, want2)
    for got, k, n in ((got1, k1, n1), (got2, k2, n2)):
        ref = torch.zeros(n, C, dtype=torch.float64).index_add_(0, k, y.double())
        # fp32 sums of at most M unit-variance terms
        assert float((got.double().cpu() - ref).abs().max()) <= 2e-6 * max(1.0, float(ref.abs().max())) * max(1.0, M ** 0.5)
