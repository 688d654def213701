"""The two-kernel mini-batch MLP forward on MXFP4 operands
(``ops.mlp_mid_score_mxfp4``), 1..256 rows.

Exact tests as in tests/test_mlp_skinny_mx4_gpu.py: integers in [-2, 2], mu =
0, sigma = 1.  W2 survives the quantiser exactly; h1 = relu(x w1 + b1) is an
integer in 0..6 whose 5s tie to 4, so the reference quantises it with
``quantize_mxfp4_cpu`` and a kernel that skips or misrounds the activation
quantiser fails.  Every partial sum is an integer below 2^24 (asserted on the
fixture's own operands), so ``torch.equal`` against fp64 is the check.  The
row counts sit either side of a row fragment (16) and of a block of four
fragments (64, 128), the unit the head kernel is built for; H = 256 leaves
two waves without a chunk and covers all four scale byte positions, 512 gives
one chunk per wave (no loop pass, the short tail), 4352 splits the chunks
9/9/8/8 (loop passes and both tails).

Real-valued test: both operands are the fp64 decode of what the device
quantisers write (``ops.expand1d_mxfp4`` on the same xn, rows padded to a
multiple of 64; ``ops.quantize_mxfp4`` of W2), the rest fp64; per row
|y - ref| <= 2 (2H + 4) 2^-24 S, the fp32 summation bound of
tests/test_mlp_skinny_gpu.py.
"""
import functools

import numpy as np
import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.models import GPUMLPRegressor
from bodywork_mlops_demo_amd.ops import reference
from bodywork_mlops_demo_amd.serving.scorer import BatchedScorer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MU, SIGMA = GPUMLPRegressor.X_MU, GPUMLPRegressor.X_SIGMA


def _dq(q, s, K):
    return reference.mxfp4_decode_cpu(q, s, K, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _int_problem(H):
    """256 rows of integer operands on the device and the fp64 reference."""
    def ints(shape, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return torch.randint(-2, 3, shape, generator=g).float()

    x, w1, b1 = ints((256,), 1), ints((H,), 2), ints((H,), 3)
    w2, b2, w3, b3 = (ints((H, H), 4), ints((H,), 5), ints((H,), 6),
                      ints((1,), 7))
    h1 = torch.relu(torch.outer(x, w1) + b1) + 0.0
    h1q = _dq(*reference.quantize_mxfp4_cpu(h1), H)
    assert not torch.equal(h1q, h1.double())
    # W2 is quantised on the device only (the CPU quantiser takes 11 s at
    # H = 4352); its decode is asserted to be W2 itself
    w2q, w2s = ops.quantize_mxfp4(w2.to(DEV))
    assert torch.equal(_dq(w2q, w2s, H), w2.double())
    h2 = torch.relu(h1q @ w2.double().t() + b2.double())
    ref = h2 @ w3.double() + b3.double()
    assert (h2 @ w3.double().abs() + b3.double().abs()).max() < 2 ** 24
    assert ref.abs().max() < 2 ** 24 and (ref != 0).sum() > 128
    dev = [t.to(DEV) for t in (w1.bfloat16(), b1.bfloat16())] + [w2q, w2s]
    dev += [t.to(DEV) for t in (b2, w3, b3)]
    return x.to(DEV), dev, ref.float().to(DEV)


@pytest.mark.parametrize(
    "m,H", [(m, H) for m in (1, 17, 64, 65, 129, 240, 256)
            for H in (256, 512)] + [(40, 4352), (256, 4352)])
def test_integer_operands_are_exact(m, H):
    x, weights, ref = _int_problem(H)
    y = ops.mlp_mid_score_mxfp4(x[:m], 0.0, 1.0, *weights)
    assert y.shape == (m,) and y.dtype == torch.float32
    assert torch.equal(y, ref[:m])


@pytest.mark.parametrize("m,H", [(32, 256), (256, 256), (40, 4352)])
def test_live_count_zeroes_and_isolates_dead_rows(m, H):
    x, weights, ref = _int_problem(H)
    for n in (0, 1, 16, 17, m - 1, m, 1 << 40):
        live = min(n, m)
        xs = x[:m].clone()
        xs[live:] = float("nan")
        n_dev = torch.tensor([n], device=DEV, dtype=torch.int64)
        y = ops.mlp_mid_score_mxfp4(xs, 0.0, 1.0, *weights, n_dev=n_dev)
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
    w2q, w2s = ops.quantize_mxfp4(w2.to(DEV))
    dev = [w1.to(DEV), b1.to(DEV), w2q, w2s, b2.to(DEV), w3.to(DEV),
           b3.to(DEV)]
    return x, (b2, w3, b3), dev


@pytest.mark.parametrize("m,H", [(17, 512), (200, 512), (40, 4352)])
def test_real_operands_within_the_fp32_summation_bound(m, H):
    x, (b2, w3, b3), dev = _real_problem(H)
    x = x[:m]
    xn = torch.zeros(-(-m // 64) * 64)
    xn[:m] = (x - MU) / SIGMA  # fp32 subtract and IEEE divide, as the kernel
    h1 = _dq(*ops.expand1d_mxfp4(xn.to(DEV), dev[0], dev[1]), H)[:m]
    w2d = _dq(dev[2], dev[3], H)
    ref = torch.relu(h1 @ w2d.t() + b2.double()) @ w3.double() + b3.double()
    S = (b2.abs().double() + h1.abs() @ w2d.abs().t()) \
        @ w3.abs().double() + b3.abs().double()
    bound = 2 * (H + H + 4) * 2.0 ** -24 * S
    y = ops.mlp_mid_score_mxfp4(x.to(DEV), MU, SIGMA, *dev)
    err = (y.cpu().double() - ref).abs()
    print(f"m={m} H={H} max err/bound {(err / bound).max().item():.2e}")
    assert (err <= bound).all()
    assert torch.equal(ops.mlp_mid_score_mxfp4(x.to(DEV), MU, SIGMA, *dev), y)


def test_a_live_row_does_not_depend_on_the_batch_or_the_count():
    x, _, dev = _real_problem(512)
    xs = x.to(DEV)
    n_dev = torch.tensor([40], device=DEV, dtype=torch.int64)
    padded = ops.mlp_mid_score_mxfp4(xs, MU, SIGMA, *dev, n_dev=n_dev)
    alone = ops.mlp_mid_score_mxfp4(xs[:40], MU, SIGMA, *dev)
    assert torch.equal(padded[:40], alone) and alone.abs().max() > 0


def test_model_and_scorer_take_the_mid_fp4_path():
    g = torch.Generator(device="cpu").manual_seed(12)
    rows = (torch.rand(600, generator=g) * 100).to(DEV)

    def mlp(seed=3, **flags):
        return GPUMLPRegressor(hidden=512, device=DEV, seed=seed, **flags)

    def direct(mdl, X):
        mdl._ensure_fp4_weights()
        return ops.mlp_mid_score_mxfp4(X, MU, SIGMA, mdl.w1_bf, mdl.b1_bf,
                                       *mdl._w2_q4, mdl.b2, mdl.w3, mdl.b3)

    def bf16(mdl, X):
        return ops.mlp_mid_score(X, MU, SIGMA, mdl.w1_bf, mdl.b1_bf,
                                 mdl.W2w_bf, mdl.b2, mdl.w3, mdl.b3)

    model, plain = mlp(mid_fp4=True), mlp()
    for n in (17, 100, 256):
        y = model.predict(rows[:n])
        assert torch.equal(y, direct(plain, rows[:n]))
        assert not torch.equal(y, bf16(plain, rows[:n]))
    assert torch.equal(model.predict(rows[:257]), plain.predict(rows[:257]))
    assert torch.equal(model.predict(rows[:16]), plain.predict(rows[:16]))

    scorer = BatchedScorer(model, DEV, use_graphs=True)
    for rnd in range(2):  # the second round replays the captured bucket
        for n in (17, 100, 256):
            X = rows[300 * rnd + 7:300 * rnd + 7 + n]
            assert torch.equal(scorer.score_tensor(X), direct(plain, X))
    assert scorer.use_graphs and sorted(scorer._graphs) == [256]
    new = mlp(seed=77)
    assert scorer.update_model(new)
    for n in (17, 100, 256):
        got = scorer.score_tensor(rows[:n])
        assert torch.equal(got, direct(new, rows[:n]))
        assert not torch.equal(got, direct(plain, rows[:n]))
    assert sorted(scorer._graphs) == [256]
