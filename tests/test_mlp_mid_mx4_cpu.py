"""CPU side of the mini-batch MXFP4 forward: ``ops.mlp_mid_score_mxfp4`` falls
to the skinny fp4 op's oracle, whose row pad follows the batch (100 rows: two
scale row groups), against the fp64 formula on integer operands (exact: see
tests/test_mlp_skinny_mx4_gpu.py), plus the live count and the flag."""
import numpy as np
import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.models import GPUMLPRegressor
from bodywork_mlops_demo_amd.ops import reference


def test_cpu_branch_is_the_widened_oracle_and_honours_the_count():
    m, H = 100, 256
    g = torch.Generator(device="cpu").manual_seed(41)
    x, w1, b1, w2, b2, w3, b3 = (
        torch.randint(-2, 3, s, generator=g).float()
        for s in ((m,), (H,), (H,), (H, H), (H,), (H,), (1,)))
    h1 = torch.zeros(128, H)
    h1[:m] = torch.relu(torch.outer(x, w1) + b1) + 0.0
    h1q = reference.mxfp4_decode_cpu(*reference.quantize_mxfp4_cpu(h1), H,
                                     dtype=np.float64)[:m]
    assert not torch.equal(h1q[64:], h1[64:m].double())  # 5 ties to 4
    ref = (torch.relu(h1q @ w2.double().t() + b2.double()) @ w3.double()
           + b3.double())
    args = (x, 0.0, 1.0, w1.bfloat16(), b1.bfloat16(),
            *ops.quantize_mxfp4(w2), b2, w3, b3)
    y = ops.mlp_mid_score_mxfp4(*args)
    assert y.dtype == torch.float32 and torch.equal(y.double(), ref)
    assert torch.equal(y, reference.mlp_skinny_score_mxfp4_cpu(*args))
    y2 = ops.mlp_mid_score_mxfp4(*args, n_dev=torch.tensor([70]))
    assert torch.equal(y2[:70], y[:70]) and not y2[70:].any()


@pytest.mark.parametrize("env", ["0", "1"])
def test_flag_argument_beats_environment_and_is_off_on_cpu(monkeypatch, env):
    monkeypatch.setenv("BODYWORK_MLP_MID_FP4", env)
    assert GPUMLPRegressor(hidden=256).mid_fp4 is (env == "1")
    assert not GPUMLPRegressor(hidden=256, mid_fp4=False).mid_fp4
    sk = GPUMLPRegressor(hidden=256).to_sklearn()
    assert GPUMLPRegressor.from_sklearn(sk).mid_fp4 is (env == "1")
    on = GPUMLPRegressor(hidden=256, seed=5, mid_fp4=True)
    x = torch.rand(100, generator=torch.Generator().manual_seed(42)) * 100
    assert on.mid_fp4 and not on._use_mid_fp4(100) and on._w2_q4 is None
    assert torch.equal(on.predict(x),
                       GPUMLPRegressor(hidden=256, seed=5).predict(x))
