"""CPU side of the skinny MXFP4 forward: the fp32 oracle against the fp64
formula on integer operands (exact: see tests/test_mlp_skinny_mx4_gpu.py) and
the flag's resolution."""
import numpy as np
import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.models import GPUMLPRegressor
from bodywork_mlops_demo_amd.ops import reference


def test_cpu_oracle_matches_the_fp64_formula():
    m, H = 5, 256
    g = torch.Generator(device="cpu").manual_seed(31)
    x, w1, b1, w2, b2, w3, b3 = (
        torch.randint(-2, 3, s, generator=g).float()
        for s in ((m,), (H,), (H,), (H, H), (H,), (H,), (1,)))
    h1 = torch.zeros(64, H)
    h1[:m] = torch.relu(torch.outer(x, w1) + b1) + 0.0
    h1q = reference.mxfp4_decode_cpu(*reference.quantize_mxfp4_cpu(h1), H,
                                     dtype=np.float64)[:m]
    assert not torch.equal(h1q, h1[:m].double())  # 5 ties to 4
    ref = (torch.relu(h1q @ w2.double().t() + b2.double()) @ w3.double()
           + b3.double())
    args = (x, 0.0, 1.0, w1.bfloat16(), b1.bfloat16(),
            *ops.quantize_mxfp4(w2), b2, w3, b3)
    y = ops.mlp_skinny_score_mxfp4(*args)
    assert y.dtype == torch.float32 and torch.equal(y.double(), ref)
    y2 = ops.mlp_skinny_score_mxfp4(*args, n_dev=torch.tensor([2]))
    assert torch.equal(y2[:2], y[:2]) and not y2[2:].any()


@pytest.mark.parametrize("env", ["0", "1"])
def test_flag_argument_beats_environment(monkeypatch, env):
    monkeypatch.setenv("BODYWORK_MLP_SKINNY_FP4", env)
    assert GPUMLPRegressor(hidden=256).skinny_fp4 is (env == "1")
    assert GPUMLPRegressor(hidden=256, skinny_fp4=True).skinny_fp4
    assert not GPUMLPRegressor(hidden=256, skinny_fp4=False).skinny_fp4
    sk = GPUMLPRegressor(hidden=256).to_sklearn()
    assert GPUMLPRegressor.from_sklearn(sk).skinny_fp4 is (env == "1")


def test_flag_changes_nothing_on_cpu():
    x = torch.rand(5, generator=torch.Generator().manual_seed(32)) * 100
    on = GPUMLPRegressor(hidden=256, seed=5, skinny_fp4=True)
    off = GPUMLPRegressor(hidden=256, seed=5)
    assert not on._use_skinny_fp4(5) and on._w2_q4 is None
    assert torch.equal(on.predict(x), off.predict(x))
