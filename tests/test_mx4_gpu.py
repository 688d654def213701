"""MXFP4 (e2m1 codes, per-32-element E8M0 block scales) kernels on hardware.

The exact tests decide the fragment layout: nibble order, which lane's scale
byte scales which 32-element block, and the op_sel byte of each fragment.
Operands are (grid value) x 2^s with s varying over rows AND blocks, so the
products are multiples of 2^-2 bounded by 576 and every partial sum over
K = 1024 stays below 2^20: exact in fp32 in any order.  All references are
plain fp64/fp32 torch on the decoded operands.
"""
import functools

import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.ops import reference as ref
from mx4_data import grid_operand

pytestmark = pytest.mark.gpu

DEV = "cuda"
K = 1024  # smallest K that turns the three-slot rotation fully over


@functools.lru_cache(maxsize=None)
def _exact():
    # the construction lives in tests/mx4_data.py, which takes K; the other
    # tile counts are in tests/test_mx4_edges_gpu.py
    a = grid_operand(768, 1, (1, 1), K).to(DEV)
    b = grid_operand(512, 2, (2, 1), K).to(DEV)
    c = (a.double() @ b.double().t())
    g = torch.Generator().manual_seed(3)
    b2 = torch.randint(-8, 9, (512,), generator=g).float().to(DEV)
    w3 = torch.randint(-8, 9, (512,), generator=g).float().to(DEV)
    h2 = torch.relu(c + b2.double())
    assert ((h2 * w3.double().abs()).sum(1).max() < 2 ** 22)  # exact in fp32
    return a, b, c.float(), b2, w3, (h2 @ w3.double()).float()


def _decode(q, s):
    return ref.mxfp4_decode_cpu(q.cpu(), s.cpu(), q.shape[1] * 2).to(DEV)


@pytest.mark.parametrize("M", [512, 768])
def test_layout_and_scales_exact(M):
    a, b, c, *_ = _exact()
    (aq, sa), (bq, sb) = ops.quantize_mxfp4(a[:M]), ops.quantize_mxfp4(b)
    assert torch.equal(_decode(aq, sa), a[:M])
    assert torch.equal(_decode(bq, sb), b)
    got = ops.gemm_mxfp4_nt(aq, sa, bq, sb, out_fp32=True)
    assert torch.equal(got, c[:M]), (got - c[:M]).abs().max().item()


@pytest.mark.parametrize("n_dev", [None, 0, 300, 512])
def test_fused_head_exact(n_dev):
    a, b, _, b2, w3, y = _exact()
    M = 512
    (aq, sa), (bq, sb) = ops.quantize_mxfp4(a[:M]), ops.quantize_mxfp4(b)
    live = M if n_dev is None else n_dev
    if live <= 300:  # dead rows hold NaN scales and all-ones codes
        aq[300:] = 0xFF
        sa[ref.mxfp4_scale_index(M, K)[300:].reshape(-1).to(DEV)] = 0xFF
    nd = None if n_dev is None else torch.tensor([n_dev], device=DEV)
    got = ops.gemm_mxfp4_relu_dot(aq, sa, bq, sb, b2, w3, n_dev=nd)
    assert torch.equal(got[:live], y[:live])
    assert (got[live:] == 0).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_device_quantiser_equals_oracle(dtype):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(64, 256, generator=g)
    # block amaxes over many binades, one zero block
    x = x * 2.0 ** torch.randint(-12, 12, (64, 8), generator=g).float(
        ).repeat_interleave(32, dim=1)
    x[5, 64:96] = 0.0
    x = x.to(dtype)
    q, s = ops.quantize_mxfp4(x.to(DEV))
    cq, cs = ref.quantize_mxfp4_cpu(x)
    assert torch.equal(q.cpu(), cq) and torch.equal(s.cpu(), cs)
    assert torch.equal(_decode(q, s).cpu(), ref.mxfp4_decode_cpu(cq, cs, 256))


@pytest.mark.parametrize("n_dev", [None, 0, 100, 256])
def test_expand1d_equals_quantiser_of_the_activation(n_dev):
    """Inputs whose arithmetic is exact in fp32 (x multiples of 1/8, w and b
    bf16-exact multiples of 1/4), so fmaf and mul-then-add cannot differ."""
    g = torch.Generator().manual_seed(8)
    n, H = 256, 512
    x = (torch.randint(-16, 17, (n,), generator=g) / 8.0).to(DEV)
    w = (torch.randint(-16, 17, (H,), generator=g) / 4.0).bfloat16().to(DEV)
    b = (torch.randint(-16, 17, (H,), generator=g) / 4.0).bfloat16().to(DEV)
    nd = None if n_dev is None else torch.tensor([n_dev], device=DEV)
    q, s = ops.expand1d_mxfp4(x, w, b, n_dev=nd)
    h = torch.relu(x[:, None] * w.float()[None, :] + b.float()[None, :])
    wq, ws = ops.quantize_mxfp4(h)
    live = n if n_dev is None else n_dev
    idx = ref.mxfp4_scale_index(n, H)[:live].reshape(-1).to(DEV)
    assert torch.equal(q[:live], wq[:live])
    assert torch.equal(s[idx], ws[idx])


def test_random_accuracy_gemm_and_head():
    g = torch.Generator(device=DEV).manual_seed(6)
    a = torch.randn(256, 4096, generator=g, device=DEV)
    b = torch.randn(512, 4096, generator=g, device=DEV)
    (aq, sa), (bq, sb) = ops.quantize_mxfp4(a), ops.quantize_mxfp4(b)
    want = _decode(aq, sa).double() @ _decode(bq, sb).double().t()
    got = ops.gemm_mxfp4_nt(aq, sa, bq, sb, out_fp32=True)
    rel = ((got - want).abs().max() / want.abs().max()).item()
    assert rel < 1e-3, rel
    b2 = torch.randn(512, generator=g, device=DEV)
    w3 = torch.randn(512, generator=g, device=DEV)
    y = ops.gemm_mxfp4_relu_dot(aq, sa, bq, sb, b2, w3)
    y_want = (torch.relu(want + b2.double()) @ w3.double()).float()
    torch.testing.assert_close(y, y_want, rtol=1e-3, atol=1e-2)


def _head_fp64(m, X):
    """(prediction, fp64 head on the operands the device itself emitted)."""
    yhat, (h1q, h1s), *_ = m._forward(X)
    h2 = torch.relu(_decode(h1q, h1s).double()
                    @ _decode(*m._w2_q4).double().t() + m.b2.double())
    return yhat, (h2 @ m.w3.double() + m.b3.double()).float()


#: twice the largest mean |fp4 - bf16 prediction| / mean |y| measured on an
#: MI355X over (hidden, seed, day) = (512, 1, 50), (512, 4, 120),
#: (1024, 2, 200); the values are in profiles/mx_fp4_scoring.md
FP4_PREDICTION_DEVIATION_BOUND = 0.0376


def test_mlp_fp4_scoring_task_parity():
    from bodywork_mlops_demo_amd.models import GPUMLPRegressor

    y, X = ops.datagen(200_000, 50, 42, device=DEV)
    m_bf = GPUMLPRegressor(hidden=512, device=DEV, seed=1)
    m_bf.fit(X, y, steps=30, batch_size=16384)
    m_f4 = GPUMLPRegressor(hidden=512, device=DEV, seed=1, fp4_scoring=True)
    assert m_f4.copy_weights_from(m_bf)
    Xe = X[:4096]
    p_bf, p_f4 = m_bf.predict(Xe), m_f4.predict(Xe)
    want = _head_fp64(m_f4, Xe)[1]
    torch.testing.assert_close(p_f4, want, rtol=1e-3, atol=1e-2)
    mape_bf = ops.score_label_metrics(p_bf, y[:4096])["MAPE"]
    mape_f4 = ops.score_label_metrics(p_f4, y[:4096])["MAPE"]
    dev = ((p_f4 - p_bf).abs().mean() / y.abs().mean()).item()
    print(f"fp4 parity: MAPE bf16 {mape_bf:.4f} fp4 {mape_f4:.4f} "
          f"deviation {dev:.5f}")
    assert abs(mape_f4 - mape_bf) < 0.05 * mape_bf + 0.01, (mape_bf, mape_f4)
    assert dev < FP4_PREDICTION_DEVIATION_BOUND, dev


def test_mlp_fp4_forward_at_an_odd_tile_count():
    """hidden = 768 is three K-tiles: the forward reaches the K-loop's third
    tail phase.  Untrained; only the forward pass is in question."""
    from bodywork_mlops_demo_amd.models import GPUMLPRegressor

    m = GPUMLPRegressor(hidden=768, device=DEV, seed=5, fp4_scoring=True)
    g = torch.Generator(device=DEV).manual_seed(14)
    X = torch.rand(512, generator=g, device=DEV) * 100
    got = m.predict(X)
    assert m._w2_q4 is not None  # the fp4 path ran
    torch.testing.assert_close(got, _head_fp64(m, X)[1], rtol=1e-3,
                               atol=1e-2)


def test_mlp_fp4_scorer_capture_and_hot_redeploy():
    """The fp4 path captures (no sync in a forward), replay equals eager,
    and a hot redeploy requantises codes and scales in place so the captured
    graph serves the NEW weights."""
    from bodywork_mlops_demo_amd.models import GPUMLPRegressor
    from bodywork_mlops_demo_amd.serving.scorer import BatchedScorer

    model = GPUMLPRegressor(hidden=512, device=DEV, seed=3, fp4_scoring=True)
    scorer = BatchedScorer(model, DEV, use_graphs=True)
    g = torch.Generator(device=DEV).manual_seed(10)
    X = torch.rand(4096, generator=g, device=DEV) * 100
    got = scorer.score_tensor(X)
    torch.testing.assert_close(got, model.predict(X), rtol=1e-3, atol=1e-3)

    new = GPUMLPRegressor(hidden=512, device=DEV, seed=77, fp4_scoring=True)
    assert scorer.update_model(new)
    got2 = scorer.score_tensor(X)
    torch.testing.assert_close(got2, new.predict(X), rtol=1e-3, atol=1e-2)
    torch.testing.assert_close(got2, _head_fp64(new, X)[1], rtol=1e-3,
                               atol=1e-2)
    assert (got2 - got).abs().max().item() > 1e-3  # actually changed
