"""CPU side of the skinny MLP forward: the fp32 oracle against the fp64
formula (same bound as tests/test_mlp_skinny_gpu.py: 2 (K + N + 4) 2^-24 S
per row, S the sum of the absolute terms) and the flag's resolution."""
import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.models import GPUMLPRegressor

MU, SIGMA = GPUMLPRegressor.X_MU, GPUMLPRegressor.X_SIGMA


def test_cpu_oracle_matches_the_fp64_formula():
    m, H = 3, 128
    g = torch.Generator(device="cpu").manual_seed(21)
    w1 = (torch.randn(H, generator=g) * 2.0 ** 0.5).bfloat16()
    b1 = (torch.randn(H, generator=g) * 0.1).bfloat16()
    w2 = (torch.randn(H, H, generator=g) * (2.0 / H) ** 0.5).bfloat16()
    b2 = torch.randn(H, generator=g) * 0.1
    w3 = torch.randn(H, generator=g) * (2.0 / H) ** 0.5
    b3 = torch.randn(1, generator=g)
    x = torch.rand(m, generator=g) * 100
    # layer 1 in plain torch: x*w1 + b1 in fp64 (the product is exact there,
    # so this is the fused multiply-add), relu, one rounding to bf16
    xn = ((x - MU) / SIGMA).double()
    h1 = torch.relu(xn[:, None] * w1.double() + b1.double()).bfloat16().double()
    ref = (torch.relu(h1 @ w2.double().t() + b2.double()) @ w3.double()
           + b3.double())
    S = (b2.abs().double() + h1.abs() @ w2.double().abs().t()) \
        @ w3.abs().double() + b3.abs().double()
    y = ops.mlp_skinny_score(x, MU, SIGMA, w1, b1, w2, b2, w3, b3)
    assert y.shape == (m,) and y.dtype == torch.float32
    assert ((y.double() - ref).abs() <= 2 * (2 * H + 4) * 2.0 ** -24 * S).all()
    n_dev = torch.tensor([2])
    y2 = ops.mlp_skinny_score(x, MU, SIGMA, w1, b1, w2, b2, w3, b3,
                              n_dev=n_dev)
    assert torch.equal(y2[:2], y[:2]) and y2[2] == 0


@pytest.mark.parametrize("env", ["0", "1"])
def test_flag_argument_beats_environment(monkeypatch, env):
    monkeypatch.setenv("BODYWORK_MLP_SKINNY", env)
    assert GPUMLPRegressor(hidden=256).skinny_scoring is (env == "1")
    assert GPUMLPRegressor(hidden=256, skinny_scoring=True).skinny_scoring
    assert not GPUMLPRegressor(hidden=256,
                               skinny_scoring=False).skinny_scoring
    sk = GPUMLPRegressor(hidden=256).to_sklearn()
    assert GPUMLPRegressor.from_sklearn(sk).skinny_scoring is (env == "1")


def test_flag_changes_nothing_on_cpu():
    x = torch.rand(5, generator=torch.Generator().manual_seed(22)) * 100
    on = GPUMLPRegressor(hidden=256, seed=5, skinny_scoring=True)
    off = GPUMLPRegressor(hidden=256, seed=5, skinny_scoring=False)
    assert not on._use_skinny(5)
    assert torch.equal(on.predict(x), off.predict(x))
