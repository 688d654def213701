"""The one-kernel mini-batch MLP forward (``ops.mlp_mid_score``), 1..256 rows.

Exact tests as in tests/test_mlp_skinny_gpu.py: every operand an integer in
[-2, 2], mu = 0, sigma = 1, so every partial sum, in any order, is an
integer that fp32 holds and ``torch.equal`` against fp64 is the check; the
fixture asserts the bound it needs on its own operands (sum_n |w3_n|
relu(.)_n + |b3| < 2^24 per row; |acc| <= 12 H < 2^24 holds outright).
H = 128 and 256 leave waves of a workgroup without a K chunk, 640 splits
2/1/1/1; the row counts sit either side of a row fragment (16) and of a
block of four fragments (64), the unit of the kernel's rolled loop.  The
kernel walks K in groups of 2048 and keeps the accumulators of a block in
LDS from one group to the next: (40, 2304) and (256, 2304) run a second
group of two chunks (two waves without one), with one partial block and
with all four; the live-count test runs (40, 2304) too, so that fragments
are skipped in a second group.

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
    """256 rows of integer operands on the device and the fp64 reference."""
    x, w1, b1 = _ints((256,), 1), _ints((H,), 2), _ints((H,), 3)
    w2, b2, w3, b3 = (_ints((H, H), 4), _ints((H,), 5), _ints((H,), 6),
                      _ints((1,), 7))
    h1 = torch.relu(torch.outer(x.double(), w1.double()) + b1.double())
    h2 = torch.relu(h1 @ w2.double().t() + b2.double())
    ref = h2 @ w3.double() + b3.double()
    assert (h2 @ w3.double().abs() + b3.double().abs()).max() < 2 ** 24
    assert ref.abs().max() < 2 ** 24 and (ref != 0).sum() > 128
    dev = [t.to(DEV) for t in (w1.bfloat16(), b1.bfloat16(), w2.bfloat16(),
                               b2, w3, b3)]
    return x.to(DEV), dev, ref.float().to(DEV)


MULTI_GROUP = [(40, 2304), (256, 2304)]


@pytest.mark.parametrize(
    "m,H", [(m, H) for m in (1, 17, 64, 65, 129, 240, 256)
            for H in (128, 256, 640)] + MULTI_GROUP)
def test_integer_operands_are_exact(m, H):
    x, weights, ref = _int_problem(H)
    y = ops.mlp_mid_score(x[:m], 0.0, 1.0, *weights)
    assert y.shape == (m,) and y.dtype == torch.float32
    assert torch.equal(y, ref[:m])


@pytest.mark.parametrize("m,H", [(32, 256), (256, 256), MULTI_GROUP[0]])
def test_live_count_zeroes_and_isolates_dead_rows(m, H):
    x, weights, ref = _int_problem(H)
    for n in (0, 1, 16, 17, m - 1, m, 1 << 40):
        live = min(n, m)
        xs = x[:m].clone()
        xs[live:] = float("nan")
        n_dev = torch.tensor([n], device=DEV, dtype=torch.int64)
        y = ops.mlp_mid_score(xs, 0.0, 1.0, *weights, n_dev=n_dev)
        assert torch.equal(y[:live], ref[:live])
        assert torch.equal(y[live:], torch.zeros(m - live, device=DEV))


@functools.lru_cache(maxsize=None)
def _real_problem(H):
    g = torch.Generator(device="cpu").manual_seed(11)
    w1 = (torch.randn(H, generator=g) * 2.0 ** 0.5).bfloat16()
    b1 = (torch.randn(H, generator=g) * 0.1).bfloat16()
    w2 = (torch.randn(H, H, generator=g) * (2.0 / H) ** 0.5).bfloat16()
    b2 = torch.randn(H, generator=g) * 0.1
    w3 = torch.randn(H, generator=g) * (2.0 / H) ** 0.5
    b3 = torch.randn(1, generator=g)
    x = torch.rand(256, generator=g) * 100
    return x, (w1, b1, w2, b2, w3, b3)


@pytest.mark.parametrize("m,H", [(17, 512), (200, 512), MULTI_GROUP[0]])
def test_real_operands_within_the_fp32_summation_bound(m, H):
    x, (w1, b1, w2, b2, w3, b3) = _real_problem(H)
    x = x[:m]
    xn = (x - MU) / SIGMA  # fp32 subtract and IEEE divide, as in the kernel
    h1 = ops.expand1d_bf16(xn.to(DEV), w1.to(DEV), b1.to(DEV),
                           relu=True).cpu().double()
    ref = (torch.relu(h1 @ w2.double().t() + b2.double()) @ w3.double()
           + b3.double())
    S = (b2.abs().double() + h1.abs() @ w2.double().abs().t()) \
        @ w3.abs().double() + b3.abs().double()
    bound = 2 * (H + H + 4) * 2.0 ** -24 * S
    args = [t.to(DEV) for t in (x, w1, b1, w2, b2, w3, b3)]
    y = ops.mlp_mid_score(args[0], MU, SIGMA, *args[1:])
    err = (y.cpu().double() - ref).abs()
    print(f"m={m} H={H} max err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    assert torch.equal(ops.mlp_mid_score(args[0], MU, SIGMA, *args[1:]), y)


def test_a_live_row_does_not_depend_on_the_batch_or_the_count():
    x, weights = _real_problem(512)
    args = [t.to(DEV) for t in weights]
    xs = x.to(DEV).clone()
    n_dev = torch.tensor([40], device=DEV, dtype=torch.int64)
    padded = ops.mlp_mid_score(xs, MU, SIGMA, *args, n_dev=n_dev)
    alone = ops.mlp_mid_score(xs[:40], MU, SIGMA, *args)
    assert torch.equal(padded[:40], alone) and alone.abs().max() > 0


def test_model_and_scorer_take_the_mid_path():
    g = torch.Generator(device="cpu").manual_seed(12)
    rows = (torch.rand(600, generator=g) * 100).to(DEV)
    model = GPUMLPRegressor(hidden=512, device=DEV, seed=3, mid_scoring=True)
    plain = GPUMLPRegressor(hidden=512, device=DEV, seed=3,
                            mid_scoring=False, skinny_scoring=False)
    both = GPUMLPRegressor(hidden=512, device=DEV, seed=3, mid_scoring=True,
                           skinny_scoring=True)

    def direct(op, mdl, X):
        return op(X, MU, SIGMA, mdl.w1_bf, mdl.b1_bf, mdl.W2w_bf, mdl.b2,
                  mdl.w3, mdl.b3)

    for n in (17, 100, 256):
        got = model.predict(rows[:n])
        assert torch.equal(got, direct(ops.mlp_mid_score, model, rows[:n]))
        assert not torch.equal(got, plain.predict(rows[:n]))
    assert torch.equal(model.predict(rows[:257]), plain.predict(rows[:257]))
    assert torch.equal(both.predict(rows[:40]),
                       direct(ops.mlp_skinny_score, both, rows[:40]))

    scorer = BatchedScorer(model, DEV, use_graphs=True)
    for rnd in range(2):  # the second round replays the captured bucket
        for n in (17, 100, 256):
            X = rows[300 * rnd + 7:300 * rnd + 7 + n]
            assert torch.equal(scorer.score_tensor(X),
                               scorer.model.predict(X))
    assert scorer.use_graphs and sorted(scorer._graphs) == [256]
    new = GPUMLPRegressor(hidden=512, device=DEV, seed=77, mid_scoring=True)
    assert scorer.update_model(new)
    for n in (17, 100, 256):
        got = scorer.score_tensor(rows[:n])
        assert torch.equal(got, new.predict(rows[:n]))
        assert not torch.equal(got, direct(ops.mlp_mid_score, plain,
                                           rows[:n]))
    assert sorted(scorer._graphs) == [256]
