"""Opt-in MX-fp8 backward GEMMs on hardware: mixed e4m3/e5m2 operands,
mask-mul epilogue, device exponents, the e5m2 support kernels, the
model's backward against the oracle, captured-graph behaviour and the
end-of-training MAPE parity gate.

The exactness tests use integer operands in [-8, 8]: every value is
representable in e4m3 AND e5m2 (e5m2 holds every integer up to 8) and the
fp32 accumulation over K <= 512 is exact, so any deviation is a layout,
format or epilogue bug, not rounding."""
import math

import numpy as np
import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.ops import reference
from bodywork_mlops_demo_amd.ops.reference import (pack_relu_mask,
                                                   unpack_relu_mask)

pytestmark = pytest.mark.gpu

DEV = "cuda"
E5M2_MAX = 57344.0
_QUANT = {"e4m3": ops.quantize_e4m3, "e5m2": ops.quantize_e5m2}
_FMT_PAIRS = (("e5m2", "e4m3"), ("e4m3", "e5m2"), ("e4m3", "e4m3"),
              ("e5m2", "e5m2"))


def _randint(m, k, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-8, 9, (m, k), generator=g, device=DEV).float()


def _i32(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def _check_mixed_formats_exact(M, N, K):
    a = _randint(M, K, 300 + K)
    b = _randint(N, K, 400 + K)
    ea, eb = -2, 3
    want = (a @ b.t()) * 2.0 ** (ea + eb)
    for fa, fb in _FMT_PAIRS:
        a8, b8 = _QUANT[fa](a, 0), _QUANT[fb](b, 0)
        got = ops.gemm_mx8_nt_fmt(a8, ea, b8, eb, fa, fb, out_fp32=True)
        assert got.dtype == torch.float32 and torch.equal(got, want), (fa, fb)
        got16 = ops.gemm_mx8_nt_fmt(a8, ea, b8, eb, fa, fb)
        assert got16.dtype == torch.bfloat16
        assert torch.equal(got16, want.bfloat16()), (fa, fb)
        # the same bytes decoded with the formats swapped give another
        # matrix, so a swapped pair of immediates cannot pass the above
        # (a pair of equal formats has no swap to tell apart)
        if fa != fb:
            swapped = reference.gemm_mx8_nt_fmt_cpu(
                a8.cpu(), ea, b8.cpu(), eb, fb, fa, out_fp32=True)
            assert not torch.equal(swapped, want.cpu()), (fa, fb)
        # device exponents: same bits as the int form
        got_d = ops.gemm_mx8_nt_fmt(a8, _i32(ea), b8, _i32(eb), fa, fb,
                                    out_fp32=True)
        assert torch.equal(got_d, got), (fa, fb)
    # defaults: bit-identical to gemm_mx8_nt
    a8, b8 = ops.quantize_e4m3(a, 0), ops.quantize_e4m3(b, 0)
    for of in (True, False):
        assert torch.equal(ops.gemm_mx8_nt_fmt(a8, ea, b8, eb, out_fp32=of),
                           ops.gemm_mx8_nt(a8, ea, b8, eb, out_fp32=of))


def _check_mask_mul_exact(M, N, K):
    a = _randint(M, K, 500 + K)
    b = _randint(N, K, 600 + K)
    g = torch.Generator(device=DEV).manual_seed(7)
    active = torch.rand(M, N, generator=g, device=DEV) > 0.5
    active[3] = False   # one all-zero row
    active[M - 2] = True  # one all-ones row
    mask = pack_relu_mask(active.cpu()).to(DEV)
    assert torch.equal(unpack_relu_mask(mask.cpu(), N), active.cpu())
    want = (a @ b.t()) * unpack_relu_mask(mask.cpu(), N).to(DEV)
    for fa, fb in _FMT_PAIRS:
        a8, b8 = _QUANT[fa](a, 0), _QUANT[fb](b, 0)
        got = ops.gemm_mx8_nt_fmt(a8, 0, b8, 0, fa, fb, mask=mask)
        assert got.dtype == torch.bfloat16
        assert torch.equal(got, want.bfloat16()), (fa, fb)
        assert int(got[3].abs().sum()) == 0, (fa, fb)
        assert torch.equal(got[M - 2],
                           (a[M - 2] @ b.t()).bfloat16()), (fa, fb)
        got32 = ops.gemm_mx8_nt_fmt(a8, 0, b8, 0, fa, fb, mask=mask,
                                    out_fp32=True)
        assert torch.equal(got32, want), (fa, fb)


_EXACT_SHAPES = [(256, 512, 512), (512, 256, 384), (256, 256, 128),
                 (256, 256, 256)]


@pytest.mark.parametrize("M,N,K", _EXACT_SHAPES)
def test_mixed_formats_exact(M, N, K):
    _check_mixed_formats_exact(M, N, K)


@pytest.mark.parametrize("M,N,K", _EXACT_SHAPES)
def test_mask_mul_epilogue_exact(M, N, K):
    _check_mask_mul_exact(M, N, K)


def test_device_exponent_is_read_at_replay():
    a, b = _randint(256, 128, 11), _randint(256, 128, 12)
    a8, b8 = ops.quantize_e5m2(a, 0), ops.quantize_e4m3(b, 0)
    e_dev = _i32(0)
    # int form and tensor form of the same value: identical bits
    assert torch.equal(
        ops.gemm_mx8_nt_fmt(a8, 2, b8, -1, "e5m2", "e4m3", out_fp32=True),
        ops.gemm_mx8_nt_fmt(a8, _i32(2), b8, _i32(-1), "e5m2", "e4m3",
                            out_fp32=True))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.gemm_mx8_nt_fmt(a8, e_dev, b8, 0, "e5m2", "e4m3", out_fp32=True)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.gemm_mx8_nt_fmt(a8, e_dev, b8, 0, "e5m2", "e4m3",
                                  out_fp32=True)
    graph.replay()
    first = out.clone()
    assert torch.equal(first, a @ b.t())
    e_dev.fill_(3)
    graph.replay()
    assert torch.equal(out, first * 8.0)
    assert int(first.abs().sum()) > 0


def _next_up(v):
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def test_amax_exponent_e5m2_device():
    one = torch.ones(8, device=DEV).bfloat16()
    cases = ([E5M2_MAX * 2.0 ** k for k in (-20, 0, 9)]
             + [_next_up(E5M2_MAX * 2.0 ** k) for k in (-20, 0, 9)]
             + [0.0, math.inf, math.nan, 2.0 ** -140, 2.0 ** 127])
    for a in cases:
        e = ops.amax_exponent_e5m2(
            torch.tensor([a], dtype=torch.float32, device=DEV), one)
        assert e.dtype == torch.int32 and e.shape == (1,)
        assert int(e[0]) == ops.e5m2_exponent(a), a
    # upper clamp: the product leaves fp32's range only as inf (-> 0), so
    # reach +127 - 15 = 112 at the top of the range and -127 at the bottom
    assert ops.e5m2_exponent(2.0 ** 127) == 112
    assert ops.e5m2_exponent(2.0 ** -140) == -127
    # n, H no block multiples; maximum in the LAST element, negative
    n, H = 1000, 264
    g = torch.Generator(device=DEV).manual_seed(13)
    x = torch.randn(n, generator=g, device=DEV) * 1e-4
    w = torch.randn(H, generator=g, device=DEV).bfloat16()
    x[-1] = -0.37
    w[-1] = -5.0
    e = ops.amax_exponent_e5m2(x, w)
    a = (x.abs().max() * w.float().abs().max()).item()
    assert a == np.float32(0.37) * np.float32(5.0)
    assert int(e[0]) == ops.e5m2_exponent(a)
    assert int(e[0]) == int(ops.amax_exponent_e5m2(x.cpu(), w.cpu())[0])
    for _ in range(3):
        assert torch.equal(ops.amax_exponent_e5m2(x, w), e)
    # a nan anywhere is not dropped by the max
    x[17] = math.nan
    assert int(ops.amax_exponent_e5m2(x, w)[0]) == 0


def _quantiser_probe():
    """Every finite code value, every tie midpoint, values past the
    range, an odd length."""
    tab = reference._E5M2
    finite = np.array([tab[c] for c in range(256) if np.isfinite(tab[c])])
    mids = np.array([(tab[c] + tab[c + 1]) / 2 for c in range(0x7B)])
    beyond = np.array([E5M2_MAX * 1.0001, E5M2_MAX * 4, 1e30, 3e38])
    v = np.concatenate([finite, mids, -mids, beyond, -beyond, [0.3]])
    assert v.size % 2 == 1
    return torch.from_numpy(v).float()


@pytest.mark.parametrize("e", [0, -7, 6])
def test_quantize_e5m2_device_equals_oracle(e):
    x = _quantiser_probe() * 2.0 ** e   # exact power-of-two scaling
    want = reference.quantize_e5m2_cpu(x, e)
    got = ops.quantize_e5m2(x.to(DEV), e)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want)
    assert torch.equal(ops.quantize_e5m2(x.to(DEV), _i32(e)), got)
    assert int(((got & 0x7F) > 0x7B).sum()) == 0   # saturates, never inf
    # bf16 input (the values bf16 holds exactly: e5m2 has 2 mantissa bits)
    xb = x.bfloat16()
    assert torch.equal(ops.quantize_e5m2(xb.to(DEV), e).cpu(),
                       reference.quantize_e5m2_cpu(xb.float(), e))
    # even length too
    assert torch.equal(ops.quantize_e5m2(x[:-1].to(DEV), e).cpu(), want[:-1])


def test_expand1d_bf16_e5m2():
    n, H = 257, 264
    g = torch.Generator(device=DEV).manual_seed(31)
    x = torch.randn(n, generator=g, device=DEV) * 3e-5
    w = (torch.randn(H, generator=g, device=DEV) * 0.06).bfloat16()
    active = torch.rand(n, H, generator=g, device=DEV) > 0.5
    mask = pack_relu_mask(active.cpu()).to(DEV)
    e = ops.amax_exponent_e5m2(x, w)
    dz, dzq = ops.expand1d_bf16_e5m2(x, w, mask, e)
    assert dz.dtype == torch.bfloat16 and dz.shape == (n, H)
    assert dzq.dtype == torch.uint8 and dzq.shape == (n, H)
    assert torch.equal(dz, ops.expand1d_bf16(x, w, None, relu=False,
                                             mask=mask))
    assert torch.equal(dzq, ops.quantize_e5m2(dz, e))
    assert torch.equal(dzq.cpu(),
                       reference.quantize_e5m2_cpu(dz.float().cpu(), e))
    # the product bound keeps every element inside the finite range: no
    # inf/nan code and nothing clamped (0x7B itself is a legitimate
    # rounding target for a value in (53248, 57344] * 2^e)
    assert int(((dzq & 0x7F) > 0x7B).sum()) == 0
    assert dz.float().abs().max().item() <= E5M2_MAX * 2.0 ** int(e[0])
    assert int(dzq.max()) > 0
    assert int(dzq[~active].max()) == 0


@pytest.mark.parametrize("R,C", [(256, 384), (272, 80), (16, 16)])
def test_transpose_u8(R, C):
    g = torch.Generator(device=DEV).manual_seed(R + C)
    src = torch.randint(0, 256, (R, C), generator=g, device=DEV,
                        dtype=torch.uint8)
    out = ops.transpose_u8(src)
    assert out.shape == (C, R) and out.is_contiguous()
    assert torch.equal(out, src.t().contiguous())


def test_transpose_u8_rejects_odd_shapes():
    assert ops.hip_available()
    src = torch.zeros(10, 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):
        ops.transpose_u8(src)
    with pytest.raises(RuntimeError):
        torch.ops.bodywork_hip.transpose_u8(src)


# -- model ------------------------------------------------------------------

def _accum_bound(A, B, K):
    """Per-element bound on the difference of two fp32 accumulation
    orders of A @ B^T: K * 2^-23 * (|A| @ |B|^T)."""
    return K * 2.0 ** -23 * (A.abs().double() @ B.abs().double().t())


def dy_of(m, xb, yb):
    """The loss gradient _step_grads starts from."""
    yhat = m._forward(xb, want_masks=True)[0]
    return (2.0 / xb.shape[0]) * (yhat - yb.float())


def test_model_backward_against_oracle(monkeypatch):
    from bodywork_mlops_demo_amd.models import GPUMLPRegressor

    H = nb = 512
    on = GPUMLPRegressor(hidden=H, device=DEV, seed=5, fp8_backward=True)
    off = GPUMLPRegressor(hidden=H, device=DEV, seed=5, fp8_training=True)
    g = torch.Generator(device=DEV).manual_seed(33)
    xb = torch.rand(nb, generator=g, device=DEV) * 100
    yb = 1.0 + 0.5 * xb + torch.randn(nb, generator=g, device=DEV) * 10
    # record the operands and results of the two fp8 GEMM calls
    calls = []
    real = ops.gemm_mx8_nt_fmt

    def spy(a8, ea, b8, eb, *args, **kw):
        out = real(a8, ea, b8, eb, *args, **kw)
        calls.append((a8, ea, b8, eb, args, kw, out))
        return out

    monkeypatch.setattr(ops, "gemm_mx8_nt_fmt", spy)
    grads = on._step_grads(xb, yb)
    monkeypatch.undo()
    # the bf16 backward's dz1 is its only ops.linear_bf16 call
    dz1_calls = []
    real_lin = ops.linear_bf16

    def spy_lin(*args, **kw):
        out = real_lin(*args, **kw)
        dz1_calls.append((kw, out))
        return out

    monkeypatch.setattr(ops, "linear_bf16", spy_lin)
    base = off._step_grads(xb, yb)
    monkeypatch.undo()
    assert len(dz1_calls) == 1 and "mask" in dz1_calls[0][0]
    dz1_bf = dz1_calls[0][1]
    assert len(calls) == 2
    (wa, wea, wb, web, wargs, wkw, dW2), (da, dea, db, deb, dargs, dkw,
                                          dz1) = calls
    assert wargs == ("e4m3", "e5m2") and wkw == {"out_fp32": True}
    assert dargs == ("e5m2", "e4m3") and set(dkw) == {"mask"}
    assert torch.equal(dW2, grads[2]) and dW2.dtype == torch.float32
    assert dz1.dtype == torch.bfloat16
    e_g = int(dea[0])
    assert torch.equal(web, dea) and wea == on._e_h1_tr
    assert deb == on._e_w2_tr
    assert torch.equal(wa, ops.transpose_u8(on._h1q_tr))
    assert torch.equal(wb, ops.transpose_u8(da))
    assert torch.equal(db, ops.quantize_e4m3(on.W2wt_bf, on._e_w2_tr))

    # wgrad from the very bytes the GPU produced: only fp32 accumulation
    # order differs
    A = reference.e4m3_decode_cpu(wa.cpu(), wea)
    B = reference.e5m2_decode_cpu(wb.cpu(), e_g)
    want = A.double() @ B.double().t()
    err = (dW2.cpu().double() - want).abs()
    bound = _accum_bound(A, B, nb)
    assert bool((err <= bound).all()), float((err - bound).max())
    assert torch.equal(
        reference.gemm_mx8_nt_fmt_cpu(wa.cpu(), wea, wb.cpu(), web.cpu(),
                                      "e4m3", "e5m2", out_fp32=True),
        A @ B.t())
    # dgrad: same, plus one bf16 ulp for the bf16 output
    A = reference.e5m2_decode_cpu(da.cpu(), e_g)
    B = reference.e4m3_decode_cpu(db.cpu(), deb)
    m1 = unpack_relu_mask(dkw["mask"].cpu(), H)
    want = (A.double() @ B.double().t()) * m1
    bound = _accum_bound(A, B, H)
    # one bf16 ulp of a value v is at most 2^-7 * |v|
    bound = bound + 2.0 ** -7 * (want.abs() + bound)
    err = (dz1.cpu().double() - want).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    assert int(dz1[~m1.to(DEV)].abs().sum()) == 0

    # gradient error against the bf16 backward on the same batch (the
    # forward is the same fp8 forward in both): reported, not gated
    def rel(a, b):
        return ((a.float() - b.float()).abs().mean()
                / b.float().abs().mean()).item()

    print(f"fp8 vs bf16 backward mean rel err: dW2 {rel(dW2, base[2]):.5f} "
          f"dz1 {rel(dz1, dz1_bf):.5f} dw1 {rel(grads[0], base[0]):.5f}")
    for g_, b_ in zip(grads, base):
        assert g_.shape == b_.shape and bool(torch.isfinite(g_).all())
    # db2, dw3, db3 do not depend on the backward GEMMs: both models sum
    # the same nb terms per output, in an order the reduction kernels do
    # not fix, so they agree to nb * 2^-23 * sum|terms| (fp32 order bound)
    dz2 = ops.expand1d_bf16(
        dy_of(on, xb, yb), on.w3_bf, None, relu=False,
        mask=on._forward(xb, want_masks=True)[5]).float()
    h2 = on._forward(xb, want_masks=True)[2].float()
    dy = dy_of(on, xb, yb)
    eps = nb * 2.0 ** -23
    for i, terms in ((3, dz2.abs().sum(0)), (4, h2.abs().t() @ dy.abs()),
                     (5, dy.abs().sum().reshape(1))):
        assert bool(((grads[i] - base[i]).abs() <= eps * terms).all()), i


def test_captured_fit_with_fp8_backward():
    from bodywork_mlops_demo_amd.models import GPUMLPRegressor

    y, X = ops.datagen(20_000, 50, 42, device=DEV)
    m = GPUMLPRegressor(hidden=512, device=DEV, seed=7, fp8_backward=True)
    w2_before = m.W2.clone()
    m.fit(X, y, steps=8, batch_size=4096)
    g0 = m._train_static["graph"]
    assert g0 is not None
    assert m._train_static["fp8_key"] == (True, m._e_w2_tr, m._e_h1_tr)
    assert m._train_static["bwd_key"] == (True, ("dgrad", "wgrad"))
    assert not torch.equal(m.W2, w2_before)
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert torch.equal(m._w2_q8_tr, ops.quantize_e4m3(m.W2w_bf, m._e_w2_tr))
    assert torch.equal(m._w2t_q8_tr,
                       ops.quantize_e4m3(m.W2wt_bf, m._e_w2_tr))
    shadow = m._w2t_q8_tr

    # the gradient exponent lives on the device: a fresh fit reuses the
    # graph
    m.reinit_(seed=7)
    assert torch.equal(m._w2t_q8_tr,
                       ops.quantize_e4m3(m.W2wt_bf, m._e_w2_tr))
    m.fit(X, y, steps=8, batch_size=4096)
    assert m._train_static["graph"] is g0
    assert m._w2t_q8_tr is shadow
    assert torch.equal(m._w2t_q8_tr,
                       ops.quantize_e4m3(m.W2wt_bf, m._e_w2_tr))
    assert all(torch.isfinite(p).all() for p in m.parameters())

    # the A/B switch is part of the graph key
    m._fp8_bwd_parts = frozenset(("dgrad",))
    m.reinit_(seed=7)
    m.fit(X, y, steps=8, batch_size=4096)
    assert m._train_static["graph"] is not g0
    assert m._train_static["bwd_key"] == (True, ("dgrad",))
    assert all(torch.isfinite(p).all() for p in m.parameters())


def test_fp8_backward_shape_fallback():
    """A batch that is no tile multiple trains through the bf16 path."""
    from bodywork_mlops_demo_amd.models import GPUMLPRegressor

    y, X = ops.datagen(20_000, 50, 42, device=DEV)
    m = GPUMLPRegressor(hidden=512, device=DEV, seed=7, fp8_backward=True)
    assert not m._use_fp8_bwd(1000) and m._use_fp8_bwd(1024)
    w2_before = m.W2.clone()
    m.fit(X, y, steps=8, batch_size=1000)
    assert m._train_static["graph"] is not None
    assert not torch.equal(m.W2, w2_before)
    assert all(torch.isfinite(p).all() for p in m.parameters())


def test_fp8_backward_end_of_training_parity():
    """MAPE parity gate of test_fp8_training_end_of_training_parity,
    unchanged (data, hidden size, steps, batch, seeds, bf16 scoring), for
    a model trained with the fp8 forward AND both fp8 backward GEMMs.

    Measured on an MI355X: see profiles/fp8_train_backward.md."""
    from bodywork_mlops_demo_amd.models import GPUMLPRegressor

    y, X = ops.datagen(200_000, 50, 42, device=DEV)
    Xe, ye = X[:4096], y[:4096]

    def trained_mape(fp8, fit_seed):
        m = GPUMLPRegressor(hidden=512, device=DEV, seed=1,
                            fp8_scoring=False, fp8_training=fp8,
                            fp8_backward=fp8)
        m.fit(X, y, steps=30, batch_size=16384, seed=fit_seed)
        if fp8:
            assert m._use_fp8_bwd(16384)
            assert m._fp8_train_saturated() == []
        return ops.score_label_metrics(m.predict(Xe), ye)["MAPE"]

    mape_bf = {s: trained_mape(False, s) for s in (42, 43, 44)}
    mape_f8 = trained_mape(True, 42)
    spread = max(mape_bf.values()) - min(mape_bf.values())
    tol = max(0.05 * mape_bf[42] + 0.01, 2.0 * spread)
    print(f"MAPE bf16-trained seeds 42/43/44: {mape_bf[42]:.6f} "
          f"{mape_bf[43]:.6f} {mape_bf[44]:.6f} (spread {spread:.6f}); "
          f"fp8 fwd+bwd-trained seed 42: {mape_f8:.6f}; "
          f"|diff| {abs(mape_f8 - mape_bf[42]):.6f} tol {tol:.6f}")
    assert abs(mape_f8 - mape_bf[42]) < tol, (mape_bf, mape_f8, tol)
