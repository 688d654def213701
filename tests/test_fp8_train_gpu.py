"""Opt-in MX-fp8 training forward on hardware: mask-emitting MX epilogue,
dual-emit layer-1 expand, model wiring, captured-graph cache behaviour
and the end-of-training MAPE parity gate.

The exactness tests use integer operands in [-8, 8]: every value is
e4m3-representable and the fp32 accumulation over K <= 512 is exact, so
any deviation is a layout / epilogue bug, not rounding."""
import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.ops.reference import pack_relu_mask

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _randint(m, k, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-8, 9, (m, k), generator=g, device=DEV).float()


def _check_epilogue_exact(M, N, K):
    a = _randint(M, K, 100 + K)
    b = _randint(N, K, 200 + K)
    # integer bias that makes row 0 EXACTLY zero before the relu: its
    # mask bits must all be 0 (catches >= in place of >)
    bias = -(b @ a[0])
    a8 = ops.quantize_e4m3(a, 0)
    b8 = ops.quantize_e4m3(b, 0)
    out, mask = ops.gemm_mx8_relu_mask(a8, 0, b8, 0, bias)
    assert out.dtype == torch.bfloat16 and out.shape == (M, N)
    assert mask.dtype == torch.uint8 and mask.shape == (M, N // 8)
    same = ops.gemm_mx8_nt(a8, 0, b8, 0, bias=bias, relu=True,
                           out_fp32=False)
    assert torch.equal(out, same)
    want = torch.relu(a @ b.t() + bias)
    assert torch.equal(out, want.bfloat16())
    assert torch.equal(mask.cpu(), pack_relu_mask((out > 0).cpu()))
    assert torch.equal(mask.cpu(), pack_relu_mask((want > 0).cpu()))
    assert int(mask[0].sum()) == 0 and int(out[0].abs().sum()) == 0
    assert int(mask[1:].sum()) > 0
    # no-bias instantiation
    out0, mask0 = ops.gemm_mx8_relu_mask(a8, 0, b8, 0)
    want0 = torch.relu(a @ b.t())
    assert torch.equal(out0, want0.bfloat16())
    assert torch.equal(mask0.cpu(), pack_relu_mask((want0 > 0).cpu()))
    # ... and the plain GEMM's no-bias relu instantiation
    same0 = ops.gemm_mx8_nt(a8, 0, b8, 0, relu=True, out_fp32=False)
    assert torch.equal(same0, out0)
    # fp32 outputs of the plain GEMM's relu epilogue, with and without bias
    assert torch.equal(ops.gemm_mx8_nt(a8, 0, b8, 0, bias=bias, relu=True,
                                       out_fp32=True), want)
    assert torch.equal(ops.gemm_mx8_nt(a8, 0, b8, 0, relu=True,
                                       out_fp32=True), want0)


@pytest.mark.parametrize("M,N,K", [(256, 512, 512), (512, 256, 384),
                                   (256, 256, 128), (256, 256, 256)])
def test_mx8_relu_mask_epilogue_exact(M, N, K):
    _check_epilogue_exact(M, N, K)


@pytest.mark.parametrize("with_bias", [True, False])
def test_expand1d_bf16_e4m3_matches_single_output_kernels(with_bias):
    n, H, e = 257, 264, -3
    g = torch.Generator(device=DEV).manual_seed(31)
    x = ((torch.rand(n, generator=g, device=DEV) * 100) - 50.0) / 28.87
    w = (torch.randn(H, generator=g, device=DEV) * 1.4).bfloat16()
    b = (torch.randn(H, generator=g, device=DEV).bfloat16()
         if with_bias else None)
    h, m, q = ops.expand1d_bf16_e4m3(x, w, b, e)
    h_ref, m_ref = ops.expand1d_bf16(x, w, b, relu=True, emit_mask=True)
    assert h.dtype == torch.bfloat16 and torch.equal(h, h_ref)
    assert m.dtype == torch.uint8 and torch.equal(m, m_ref)
    assert q.dtype == torch.uint8 and q.shape == (n, H)
    assert torch.equal(q, ops.expand1d_e4m3(x, w, b, e))
    assert int(m.sum()) > 0


def test_model_fp8_training_forward():
    from bodywork_mlops_demo_amd.models import GPUMLPRegressor

    on = GPUMLPRegressor(hidden=512, device=DEV, seed=5, fp8_training=True)
    off = GPUMLPRegressor(hidden=512, device=DEV, seed=5,
                          fp8_training=False)
    g = torch.Generator(device=DEV).manual_seed(32)
    xb = torch.rand(512, generator=g, device=DEV) * 100
    _, h1, h2, xn, m1, m2 = on._forward(xb, want_masks=True)
    _, h1_r, h2_r, _, m1_r, _ = off._forward(xb, want_masks=True)
    assert torch.equal(h1, h1_r) and torch.equal(m1, m1_r)
    assert off._w2_q8_tr is None
    assert torch.equal(on._w2_q8_tr,
                       ops.quantize_e4m3(on.W2w_bf, on._e_w2_tr))
    h1_w, m1_w, h1q = ops.expand1d_bf16_e4m3(xn, on.w1_bf, on.b1_bf,
                                             on._e_h1_tr)
    h2_w, m2_w = ops.gemm_mx8_relu_mask(h1q, on._e_h1_tr, on._w2_q8_tr,
                                        on._e_w2_tr, on.b2)
    assert torch.equal(h1, h1_w) and torch.equal(m1, m1_w)
    assert torch.equal(h2, h2_w) and torch.equal(m2, m2_w)
    assert torch.equal(m2.cpu(), pack_relu_mask((h2 > 0).cpu()))
    # the project's quantisation bound (test_mx8_random_accuracy_...)
    rel = ((h2.float() - h2_r.float()).abs().mean()
           / h2_r.float().abs().mean()).item()
    print(f"fp8 vs bf16 h2 mean rel err: {rel:.5f}")
    assert rel < 0.05, rel
    assert not torch.equal(h2, h2_r)  # the MX kernel really ran


def _assert_no_saturation(m):
    assert m._fp8_train_saturated() == []
    assert m.W2.abs().max().item() <= 448.0 * 2.0 ** m._e_w2_tr
    h1_bound = (m._xn_max_tr * m.w1.abs().max().item()
                + m.b1.abs().max().item())
    assert h1_bound <= 448.0 * 2.0 ** m._e_h1_tr
    # the shadow the (captured) step maintains is the quantised W2w_bf
    assert torch.equal(m._w2_q8_tr,
                       ops.quantize_e4m3(m.W2w_bf, m._e_w2_tr))


def test_fp8_training_captured_fit_graph_cache():
    from bodywork_mlops_demo_amd.models import GPUMLPRegressor

    y, X = ops.datagen(20_000, 50, 42, device=DEV)
    m = GPUMLPRegressor(hidden=512, device=DEV, seed=7, fp8_training=True)
    w2_before = m.W2.clone()
    m.fit(X, y, steps=8, batch_size=4096)
    g0 = m._train_static["graph"]
    assert g0 is not None
    assert m._train_static["fp8_key"] == (True, m._e_w2_tr, m._e_h1_tr)
    assert not torch.equal(m.W2, w2_before)
    assert all(torch.isfinite(p).all() for p in m.parameters())
    _assert_no_saturation(m)
    shadow = m._w2_q8_tr

    # same weights + same data -> same exponents -> the graph is reused
    key = m._train_static["fp8_key"]
    m.reinit_(seed=7)
    m.fit(X, y, steps=8, batch_size=4096)
    assert m._train_static["fp8_key"] == key
    assert m._train_static["graph"] is g0
    assert m._w2_q8_tr is shadow
    _assert_no_saturation(m)

    # W2 x8 -> e_w2 moves by 3 -> a stale graph would bake the wrong
    # exponent: it must be rebuilt
    m.W2.mul_(8.0)
    m.W2wt_bf.copy_(m.W2.bfloat16())
    m.W2w_bf.copy_(ops.transpose_bf16(m.W2wt_bf))
    m._refresh_fp8_train()
    m.fit(X, y, steps=8, batch_size=4096)
    assert m._train_static["fp8_key"] != key
    assert m._train_static["fp8_key"][1] > key[1]
    assert m._train_static["graph"] is not None
    assert m._train_static["graph"] is not g0
    assert all(torch.isfinite(p).all() for p in m.parameters())
    _assert_no_saturation(m)


def test_fp8_training_shape_fallback():
    """A batch that is no tile multiple trains through the bf16 forward."""
    from bodywork_mlops_demo_amd.models import GPUMLPRegressor

    y, X = ops.datagen(20_000, 50, 42, device=DEV)
    m = GPUMLPRegressor(hidden=512, device=DEV, seed=7, fp8_training=True)
    assert not m._use_fp8_train(1000) and m._use_fp8_train(1024)
    m.fit(X, y, steps=8, batch_size=1000)
    assert m._train_static["graph"] is not None
    assert all(torch.isfinite(p).all() for p in m.parameters())


def test_fp8_training_end_of_training_parity():
    """MAPE parity gate: a model trained with the fp8 forward scores (in
    bf16, so only training differs) as well as its bf16-trained twin, to
    within the larger of the project's fp8 gate and twice the bf16
    model's own fit-seed-to-fit-seed MAPE spread."""
    from bodywork_mlops_demo_amd.models import GPUMLPRegressor

    y, X = ops.datagen(200_000, 50, 42, device=DEV)
    Xe, ye = X[:4096], y[:4096]

    def trained_mape(fp8, fit_seed):
        m = GPUMLPRegressor(hidden=512, device=DEV, seed=1,
                            fp8_scoring=False, fp8_training=fp8)
        m.fit(X, y, steps=30, batch_size=16384, seed=fit_seed)
        if fp8:
            _assert_no_saturation(m)
        return ops.score_label_metrics(m.predict(Xe), ye)["MAPE"]

    mape_bf = {s: trained_mape(False, s) for s in (42, 43, 44)}
    mape_f8 = trained_mape(True, 42)
    spread = max(mape_bf.values()) - min(mape_bf.values())
    tol = max(0.05 * mape_bf[42] + 0.01, 2.0 * spread)
    print(f"MAPE bf16-trained seeds 42/43/44: {mape_bf[42]:.6f} "
          f"{mape_bf[43]:.6f} {mape_bf[44]:.6f} (spread {spread:.6f}); "
          f"fp8-trained seed 42: {mape_f8:.6f}; "
          f"|diff| {abs(mape_f8 - mape_bf[42]):.6f} tol {tol:.6f}")
    assert abs(mape_f8 - mape_bf[42]) < tol, (mape_bf, mape_f8, tol)
