"""MXFP4 (e2m1 codes, per-32-element E8M0 block scales) oracle and the
fp4 scoring flag, on the CPU."""
import numpy as np
import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.ops import reference as ref

GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _roundtrip(x):
    q, s = ops.quantize_mxfp4(x)
    return q, s, ref.mxfp4_decode_cpu(q, s, x.shape[1])


@pytest.mark.parametrize("k", [-20, -1, 0, 3, 40])
def test_grid_values_round_trip(k):
    """Every grid value times 2^k, both signs, comes back exactly; blocks
    that hold a 4 or a 6 and blocks that do not."""
    vals = torch.tensor(GRID + [-v for v in GRID[1:]])
    g = torch.Generator().manual_seed(k + 100)
    x = vals[torch.randint(0, 15, (64, 256), generator=g)] * 2.0 ** k
    x[:, ::64] = 6.0 * 2.0 ** k
    _, _, back = _roundtrip(x)
    assert torch.equal(back, x)


@pytest.mark.parametrize("k", [-126, -3, 0, 5, 120])
def test_exponent_rule_at_the_boundary(k):
    """amax = 6 * 2^k gives e = k, the next float above gives k + 1."""
    top = np.float32(6.0 * 2.0 ** k)
    above = np.nextafter(top, np.float32(np.inf))
    assert ref.mxfp4_block_exponent(np.array([top, above])).tolist() == [
        k, k + 1]
    x = torch.zeros(64, 256)
    x[0, 5], x[1, 40] = float(top), float(above)
    _, s, _ = _roundtrip(x)
    idx = ref.mxfp4_scale_index(64, 256)
    assert int(s[idx[0, 0]]) == k + 127 and int(s[idx[1, 1]]) == k + 128


@pytest.mark.parametrize("value, want", [
    (2.5, 2.0), (3.5, 4.0), (5.0, 4.0), (0.25, 0.0), (0.75, 1.0),
    (1.25, 1.0), (-2.5, -2.0), (-5.0, -4.0)])
def test_ties_go_to_the_even_code(value, want):
    x = torch.zeros(64, 256)
    x[:, 0] = 6.0  # pins every first block's exponent at 0
    x[3, 7] = value
    q, _, back = _roundtrip(x)
    assert back[3, 7].item() == want
    code = (int(q[3, 3]) >> 4) & 0xF  # element 7 = high nibble of byte 3
    assert GRID[code & 7] == abs(want) and bool(code & 8) == (value < 0)


def test_zero_block_and_packing():
    x = torch.zeros(64, 256)
    x[0, 32:64] = torch.arange(32) % 7 - 3.0
    q, s, back = _roundtrip(x)
    idx = ref.mxfp4_scale_index(64, 256)
    assert int(s[idx[0, 0]]) == 127 and int(s[idx[5, 3]]) == 127
    assert torch.equal(back, x)
    assert sorted(idx.reshape(-1).tolist()) == list(range(64 * 8))
    # bf16 input is widened, not re-rounded
    qb, sb = ops.quantize_mxfp4(x.bfloat16())
    assert torch.equal(qb, q) and torch.equal(sb, s)


def test_cpu_gemm_and_head_follow_the_decode():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(256, 256, generator=g), torch.randn(256, 256,
                                                           generator=g)
    (aq, sa), (bq, sb) = ops.quantize_mxfp4(a), ops.quantize_mxfp4(b)
    want = (ref.mxfp4_decode_cpu(aq, sa, 256)
            @ ref.mxfp4_decode_cpu(bq, sb, 256).t())
    assert torch.equal(ops.gemm_mxfp4_nt(aq, sa, bq, sb, out_fp32=True), want)
    b2, w3 = torch.randn(256, generator=g), torch.randn(256, generator=g)
    y = ops.gemm_mxfp4_relu_dot(aq, sa, bq, sb, b2, w3,
                                n_dev=torch.tensor([100]))
    torch.testing.assert_close(y[:100], (torch.relu(want + b2) @ w3)[:100])
    assert (y[100:] == 0).all()
    with pytest.raises(RuntimeError):
        ops.quantize_mxfp4(torch.zeros(32, 256))


def test_model_name_and_flags(monkeypatch):
    from bodywork_mlops_demo_amd.models import GPUMLPRegressor
    from bodywork_mlops_demo_amd.pipeline.loop import resolve_model

    assert resolve_model("mlp-fp4") == ("mlp", {"BODYWORK_MLP_FP4": "1"})
    assert not GPUMLPRegressor(hidden=256).fp4_scoring
    monkeypatch.setenv("BODYWORK_MLP_FP4", "1")
    m_env = GPUMLPRegressor(hidden=256)
    assert m_env.fp4_scoring
    assert GPUMLPRegressor.from_sklearn(m_env.to_sklearn()).fp4_scoring
    monkeypatch.delenv("BODYWORK_MLP_FP4")
    m = GPUMLPRegressor(hidden=256, fp4_scoring=True)
    plain = GPUMLPRegressor(hidden=256)
    X = torch.rand(256) * 100
    # on the CPU predict takes the normal path, as with the fp8 flag
    assert torch.equal(m.predict(X), plain.predict(X))
    assert m._w2_q4 is None
