"""BatchedScorer scores only the rows that exist.

For the linear model the captured graph reads a per-bucket device row
count instead of scoring a padded bucket; the result must stay bitwise
what ``model.predict`` gives, also when the count changes between
replays of the same bucket and after a hot redeploy.  Other models keep
the pad-and-slice path.

Sizes: 5 and 16 (inside / exactly the 16-row bucket), 257 (4096 bucket,
float4 body + tail), 2^20+1 (first row past a bucket edge: 2^22 bucket,
several blocks, grid-stride).
"""
import pytest
import torch

from bodywork_mlops_demo_amd.models import GPULinearRegressor, GPUPolyRegressor
from bodywork_mlops_demo_amd.serving.scorer import BatchedScorer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [5, 16, 257, (1 << 20) + 1]


@pytest.fixture(scope="module")
def rows():
    g = torch.Generator(device="cpu").manual_seed(5)
    return (torch.rand((1 << 20) + 8, generator=g) * 100).to(DEV)


@pytest.mark.parametrize("n", SIZES)
def test_linear_scorer_matches_predict(rows, n):
    model = GPULinearRegressor(1.1, 0.47, device=DEV)
    scorer = BatchedScorer(model, DEV, use_graphs=True)
    X = rows[:n]
    got = scorer.score_tensor(X)
    assert scorer.use_graphs, "graph capture fell back to direct launches"
    assert got.shape == X.shape
    assert torch.equal(got, model.predict(X))

    # a different row count in the same bucket: the count must reach the
    # captured kernel, and stale rows of the static buffers must not leak
    b = scorer._bucket(n)
    n2 = n - 3 if scorer._bucket(n - 3) == b else n + 3
    assert scorer._bucket(n2) == b
    X2 = rows[-n2:] + 1.0
    got2 = scorer.score_tensor(X2)
    assert got2.shape == X2.shape
    assert torch.equal(got2, model.predict(X2))
    assert sorted(scorer._graphs) == [b]  # one capture served both
    # the first result was a copy, not a view of the static output
    assert torch.equal(got, model.predict(X))

    # hot redeploy: new weights reach the captured graph
    assert scorer.update_model(GPULinearRegressor(-2.5, 1.75, device=DEV))
    fresh = GPULinearRegressor(-2.5, 1.75, device=DEV)
    assert torch.equal(scorer.score_tensor(X), fresh.predict(X))
    assert sorted(scorer._graphs) == [b]


def test_live_count_is_clamped_to_the_buffer(rows):
    """A count larger than the buffer must not make the kernel run past
    it: the op clamps to the tensor's length."""
    from bodywork_mlops_demo_amd import ops

    X = rows[:1000]
    ab = torch.tensor([1.1, 0.47], device=DEV)
    n_dev = torch.tensor([1 << 40], device=DEV, dtype=torch.int64)
    got = ops.linear_score(X, ab=ab, n_dev=n_dev)
    assert torch.equal(got, ops.linear_score(X, ab=ab))
    n_dev.fill_(10)
    got = ops.linear_score(X, ab=ab, n_dev=n_dev)
    assert torch.equal(got[:10], ops.linear_score(X[:10], ab=ab))


@pytest.mark.parametrize("n", [5, 257])
def test_poly_scorer_still_pads_and_matches(rows, n):
    model = GPUPolyRegressor(degree=2, device=DEV)
    model.coef_t_ = [3.0, 0.8, -0.25]
    scorer = BatchedScorer(model, DEV, use_graphs=True)
    assert not scorer._live_rows
    X = rows[:n]
    got = scorer.score_tensor(X)
    assert torch.equal(got, model.predict(X))
    b = scorer._bucket(n)
    assert scorer._graphs[b][3] is None  # no count tensor: padded path
    if n < b:
        assert bool((scorer._graphs[b][1][n:] == 1.0).all())
