"""The one-kernel skinny MLP forward (``ops.mlp_skinny_score``), 1..64 rows.

Exact tests: every operand an integer in [-2, 2], mu = 0, sigma = 1.  Then
h1 <= 6 is exact in bf16, |acc| <= 6*2*640 = 7680, |relu(acc + b2) * w3| <=
15364 and |y| <= 640 * 15364 + 2 < 2^24: every partial sum, in any order, is
an integer that fp32 holds, so ``torch.equal`` against fp64 is the check.
H = 128 and 256 leave waves of a workgroup without a K chunk, 640 splits
2/1/1/1; the row counts sit either side of each row-fragment boundary.
The kernel walks K in groups (4096 wide for up to 32 rows, 2048 wide
above) and reuses its LDS copy of w1/b1 from one group to the next: (40,
2304) runs two groups with a partial second one, (16, 4224) and (20, 4224)
a second group of a single chunk for 1 and 2 row fragments.  There the
worst-case bound above exceeds 2^24, so the reference asserts the bound it
needs on its own operands: sum_n |w3_n| relu(.)_n + |b3| < 2^24 per row
bounds every partial sum of the head in any order (|acc| <= 12 H < 2^24
holds outright).

Real-valued test: layer 1 from ``ops.expand1d_bf16`` on the same xn, the
rest fp64; per row |y - ref| <= 2 (K + N + 4) 2^-24 S with S = |b3| + sum_n
|w3_n| (|b2_n| + sum_k |h1_k W2_nk|), the forward bound of fp32 summation
in any order (factor 2 for the second-order terms).
"""
import functools

import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.models import GPUMLPRegressor
from bodywork_mlops_demo_amd.serving.scorer import BatchedScorer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MU, SIGMA = GPUMLPRegressor.X_MU, GPUMLPRegressor.X_SIGMA


def _ints(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-2, 3, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def _int_problem(H):
    """64 rows of integer operands on the device and the fp64 reference."""
    x, w1, b1 = _ints((64,), 1), _ints((H,), 2), _ints((H,), 3)
    w2, b2, w3, b3 = (_ints((H, H), 4), _ints((H,), 5), _ints((H,), 6),
                      _ints((1,), 7))
    h1 = torch.relu(torch.outer(x.double(), w1.double()) + b1.double())
    h2 = torch.relu(h1 @ w2.double().t() + b2.double())
    ref = h2 @ w3.double() + b3.double()
    assert (h2 @ w3.double().abs() + b3.double().abs()).max() < 2 ** 24
    assert ref.abs().max() < 2 ** 24 and (ref != 0).sum() > 32
    dev = [t.to(DEV) for t in (w1.bfloat16(), b1.bfloat16(), w2.bfloat16(),
                               b2, w3, b3)]
    return x.to(DEV), dev, ref.float().to(DEV)


MULTI_GROUP = [(40, 2304), (16, 4224), (20, 4224)]


@pytest.mark.parametrize(
    "m,H", [(m, H) for m in (1, 5, 16, 17, 33, 64) for H in (128, 256, 640)]
    + MULTI_GROUP)
def test_integer_operands_are_exact(m, H):
    x, weights, ref = _int_problem(H)
    y = ops.mlp_skinny_score(x[:m], 0.0, 1.0, *weights)
    assert y.shape == (m,) and y.dtype == torch.float32
    assert torch.equal(y, ref[:m])


@pytest.mark.parametrize("m", [16, 48])
def test_live_count_zeroes_and_isolates_dead_rows(m):
    x, weights, ref = _int_problem(256)
    for n in (0, 1, m - 1, m, 1 << 40):
        live = min(n, m)
        xs = x[:m].clone()
        xs[live:] = float("nan")
        n_dev = torch.tensor([n], device=DEV, dtype=torch.int64)
        y = ops.mlp_skinny_score(xs, 0.0, 1.0, *weights, n_dev=n_dev)
        assert torch.equal(y[:live], ref[:live])
        assert torch.equal(y[live:], torch.zeros(m - live, device=DEV))


@pytest.mark.parametrize("m,H", [(1, 512), (16, 512), (40, 512)]
                         + MULTI_GROUP[:2])
def test_real_operands_within_the_fp32_summation_bound(m, H):
    g = torch.Generator(device="cpu").manual_seed(11)
    w1 = (torch.randn(H, generator=g) * 2.0 ** 0.5).bfloat16()
    b1 = (torch.randn(H, generator=g) * 0.1).bfloat16()
    w2 = (torch.randn(H, H, generator=g) * (2.0 / H) ** 0.5).bfloat16()
    b2 = torch.randn(H, generator=g) * 0.1
    w3 = torch.randn(H, generator=g) * (2.0 / H) ** 0.5
    b3 = torch.randn(1, generator=g)
    x = torch.rand(m, generator=g) * 100
    xn = (x - MU) / SIGMA  # fp32 subtract and IEEE divide, as in the kernel
    h1 = ops.expand1d_bf16(xn.to(DEV), w1.to(DEV), b1.to(DEV),
                           relu=True).cpu().double()
    ref = (torch.relu(h1 @ w2.double().t() + b2.double()) @ w3.double()
           + b3.double())
    S = (b2.abs().double() + h1.abs() @ w2.double().abs().t()) \
        @ w3.abs().double() + b3.abs().double()
    bound = 2 * (H + H + 4) * 2.0 ** -24 * S
    args = [t.to(DEV) for t in (x, w1, b1, w2, b2, w3, b3)]
    y = ops.mlp_skinny_score(args[0], MU, SIGMA, *args[1:])
    err = (y.cpu().double() - ref).abs()
    assert (err <= bound).all()
    assert torch.equal(ops.mlp_skinny_score(args[0], MU, SIGMA, *args[1:]), y)


def test_model_and_scorer_take_the_skinny_path():
    g = torch.Generator(device="cpu").manual_seed(12)
    rows = (torch.rand(256, generator=g) * 100).to(DEV)
    model = GPUMLPRegressor(hidden=512, device=DEV, seed=3,
                            skinny_scoring=True)
    plain = GPUMLPRegressor(hidden=512, device=DEV, seed=3,
                            skinny_scoring=False)

    def direct(mdl, X):
        return ops.mlp_skinny_score(X, MU, SIGMA, mdl.w1_bf, mdl.b1_bf,
                                    mdl.W2w_bf, mdl.b2, mdl.w3, mdl.b3)

    for n in (1, 16, 40):
        assert torch.equal(model.predict(rows[:n]), direct(model, rows[:n]))
    assert not torch.equal(model.predict(rows[:40]), plain.predict(rows[:40]))
    assert torch.equal(model.predict(rows[:65]), plain.predict(rows[:65]))

    scorer = BatchedScorer(model, DEV, use_graphs=True)
    for rnd in range(2):  # the second round replays the captured buckets
        for n in (1, 5, 16):
            X = rows[100 * rnd + n:100 * rnd + 2 * n]
            assert torch.equal(scorer.score_tensor(X),
                               scorer.model.predict(X))
    assert scorer.use_graphs and sorted(scorer._graphs) == [1, 16]
    new = GPUMLPRegressor(hidden=512, device=DEV, seed=77,
                          skinny_scoring=True)
    assert scorer.update_model(new)
    for n in (1, 5, 16):
        got = scorer.score_tensor(rows[:n])
        assert torch.equal(got, new.predict(rows[:n]))
        assert not torch.equal(got, direct(plain, rows[:n]))
    assert sorted(scorer._graphs) == [1, 16]
