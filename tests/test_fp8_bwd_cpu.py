"""Opt-in MX-fp8 backward GEMMs (e5m2 gradients): exponent rule, e5m2
quantiser and format-aware GEMM oracles, model wiring and flag plumbing
(runs anywhere; the hardware half lives in test_fp8_bwd_gpu.py)."""
import math

import numpy as np
import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.models import GPUMLPRegressor
from bodywork_mlops_demo_amd.ops import reference

E5M2_MAX = 57344.0


def _next_up(v: float) -> float:
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def _dev_exponent(a: float) -> int:
    """The "device" rule on CPU: product bound of x=[a] and w=[1]."""
    e = ops.amax_exponent_e5m2(torch.tensor([a], dtype=torch.float32),
                               torch.ones(1).bfloat16())
    assert e.dtype == torch.int32 and e.shape == (1,)
    return int(e[0])


# (amax, expected exponent): the boundary a = 57344 * 2^k is representable
# with e = k, the next fp32 above it needs e = k + 1
EXPONENT_CASES = (
    [(E5M2_MAX * 2.0 ** k, k) for k in (-20, 0, 9)]
    + [(_next_up(E5M2_MAX * 2.0 ** k), k + 1) for k in (-20, 0, 9)]
    + [(0.0, 0), (math.inf, 0), (math.nan, 0),
       (1e-38, -127), (2.0 ** 127, 127 - 15)]
)


@pytest.mark.parametrize("a,want", EXPONENT_CASES)
def test_e5m2_exponent_rule_host_and_device_agree(a, want):
    assert ops.e5m2_exponent(a) == want
    assert _dev_exponent(a) == want
    if math.isfinite(a) and a > 0 and -127 < want < 127:
        # smallest e with a / 2^e <= 57344
        assert a / 2.0 ** want <= E5M2_MAX < a / 2.0 ** (want - 1)


def test_e5m2_exponent_clamps():
    # below: 2^-140 would want e = -155; above: a python float past fp32
    assert ops.e5m2_exponent(2.0 ** -140) == -127
    assert ops.e5m2_exponent(2.0 ** 200) == 127
    assert _dev_exponent(2.0 ** -140) == -127
    # negative maxima count by magnitude, and the product is the bound
    e = ops.amax_exponent_e5m2(torch.tensor([1.0, -E5M2_MAX, 3.0]),
                               torch.tensor([0.5, -2.0]).bfloat16())
    assert int(e[0]) == 1


def test_e5m2_table_and_round_trip_of_every_finite_code():
    tab = reference._E5M2
    assert tab.shape == (256,)
    assert tab[0x7C] == math.inf and tab[0xFC] == -math.inf
    assert np.isnan(tab[0x7D:0x80]).all() and np.isnan(tab[0xFD:]).all()
    assert tab[0x7B] == E5M2_MAX and tab[0xFB] == -E5M2_MAX
    assert tab[0x01] == 2.0 ** -16 and tab[0x3C] == 1.0
    finite = [c for c in range(256) if np.isfinite(tab[c])]
    codes = torch.tensor(finite, dtype=torch.uint8)
    for e in (0, -3, 5):
        vals = reference.e5m2_decode_cpu(codes, e)
        assert torch.equal(reference.quantize_e5m2_cpu(vals, e), codes)
        assert torch.equal(ops.quantize_e5m2(vals, e), codes)


def test_quantize_e5m2_ties_saturation_and_sign():
    tab = reference._E5M2
    pos = [c for c in range(0x7B)]
    mids = torch.tensor([(tab[c] + tab[c + 1]) / 2 for c in pos],
                        dtype=torch.float64)
    want = torch.tensor([c if c % 2 == 0 else c + 1 for c in pos],
                        dtype=torch.uint8)
    assert torch.equal(reference.quantize_e5m2_cpu(mids, 0), want)
    assert torch.equal(reference.quantize_e5m2_cpu(-mids, 0), want | 0x80)
    # just off the midpoint goes to the nearer neighbour
    lo = torch.tensor([1.0 + 0.124, 1.0 + 0.126], dtype=torch.float64)
    assert reference.quantize_e5m2_cpu(lo, 0).tolist() == [0x3C, 0x3D]
    # saturation at +-57344 (never inf codes), scaled by the exponent
    big = torch.tensor([1e9, -1e9, math.inf, -math.inf, E5M2_MAX * 8.0001])
    assert reference.quantize_e5m2_cpu(big, 3).tolist() == [
        0x7B, 0xFB, 0x7B, 0xFB, 0x7B]
    assert reference.quantize_e5m2_cpu(torch.tensor([E5M2_MAX * 8]),
                                       3).tolist() == [0x7B]
    # sign preserved, zero's included (0x80 is -0, as the hardware
    # convert gives)
    q = reference.quantize_e5m2_cpu(
        torch.tensor([-1.5, 1.5, -0.0, 0.0, -1e-9]), 0)
    assert q.tolist() == [0xBE, 0x3E, 0x80, 0x00, 0x80]
    # the int32[1] tensor form of e is read
    x = torch.randn(33, generator=torch.Generator().manual_seed(1)) * 40
    assert torch.equal(ops.quantize_e5m2(x, -2),
                       ops.quantize_e5m2(x, torch.tensor([-2],
                                                         dtype=torch.int32)))


def _randint(m, k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (m, k), generator=g).float()


def test_gemm_mx8_nt_fmt_cpu_defaults_equal_gemm_mx8_nt():
    g = torch.Generator().manual_seed(2)
    a = torch.randn(64, 128, generator=g)
    b = torch.randn(32, 128, generator=g)
    a8, b8 = ops.quantize_e4m3(a, -5), ops.quantize_e4m3(b, -6)
    for of in (True, False):
        assert torch.equal(ops.gemm_mx8_nt_fmt(a8, -5, b8, -6, out_fp32=of),
                           ops.gemm_mx8_nt(a8, -5, b8, -6, out_fp32=of))
    e = torch.tensor([-5], dtype=torch.int32)
    assert torch.equal(ops.gemm_mx8_nt_fmt(a8, e, b8, -6, out_fp32=True),
                       ops.gemm_mx8_nt(a8, -5, b8, -6, out_fp32=True))


def test_gemm_mx8_nt_fmt_cpu_formats_and_mask_exact():
    a, b = _randint(32, 64, 3), _randint(48, 64, 4)
    a5, b4 = ops.quantize_e5m2(a, 0), ops.quantize_e4m3(b, 0)
    want = (a @ b.t()) * 2.0 ** (-2 + 3)
    got = ops.gemm_mx8_nt_fmt(a5, -2, b4, 3, "e5m2", "e4m3", out_fp32=True)
    assert torch.equal(got, want)
    # the same bytes read with the formats swapped mean something else
    swapped = ops.gemm_mx8_nt_fmt(a5, -2, b4, 3, "e4m3", "e5m2",
                                  out_fp32=True)
    assert not torch.equal(swapped, want)
    active = torch.rand(32, 48, generator=torch.Generator().manual_seed(5)) > .5
    active[0] = False
    mask = reference.pack_relu_mask(active)
    got = ops.gemm_mx8_nt_fmt(a5, -2, b4, 3, "e5m2", "e4m3", mask=mask)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got, (want * active).bfloat16())
    assert int(got[0].abs().sum()) == 0
    with pytest.raises(ValueError):
        ops.gemm_mx8_nt_fmt(a5, 0, b4, 0, "e3m4", "e4m3")


def test_transpose_u8_and_expand_cpu():
    g = torch.Generator().manual_seed(6)
    src = torch.randint(0, 256, (32, 48), generator=g, dtype=torch.uint8)
    assert torch.equal(ops.transpose_u8(src), src.t().contiguous())
    with pytest.raises(RuntimeError):
        ops.transpose_u8(src[:10, :16])
    n, H = 37, 72
    x = torch.randn(n, generator=g) * 1e-3
    w = torch.randn(H, generator=g).bfloat16()
    mask = reference.pack_relu_mask(torch.rand(n, H, generator=g) > 0.4)
    e = ops.amax_exponent_e5m2(x, w)
    dz, dzq = ops.expand1d_bf16_e5m2(x, w, mask, e)
    assert torch.equal(dz, ops.expand1d_bf16(x, w, None, relu=False,
                                             mask=mask))
    assert torch.equal(dzq, ops.quantize_e5m2(dz, e))
    # the product bound keeps every element inside the finite range: no
    # inf/nan code, and nothing was clamped (0x7B itself is a legitimate
    # rounding target for a value in (53248, 57344] * 2^e)
    assert int(((dzq & 0x7F) > 0x7B).sum()) == 0
    assert dz.float().abs().max().item() <= 57344.0 * 2.0 ** int(e[0])
    assert int(dzq.max()) > 0


# -- model ------------------------------------------------------------------

def _batch(n, seed):
    g = torch.Generator().manual_seed(seed)
    xb = torch.rand(n, generator=g) * 100
    yb = 1.0 + 0.5 * xb + torch.randn(n, generator=g) * 10
    return xb, yb


def _oracle_step_grads(m, xb, yb, parts=("dgrad", "wgrad")):
    """The fp8 backward written out by hand from the oracles."""
    nb = xb.shape[0]
    xn = (xb.float() - m.X_MU) / m.X_SIGMA
    h1, m1 = reference.expand1d_cpu(xn, m.w1_bf, m.b1_bf, relu=True,
                                    emit_mask=True)
    h1q = reference.quantize_e4m3_cpu(h1.float(), m._e_h1_tr)
    c = reference.gemm_mx8_nt_cpu(h1q, m._e_h1_tr, m._w2_q8_tr, m._e_w2_tr,
                                  m.b2, relu=True, out_fp32=True)
    h2, m2 = c.bfloat16(), reference.pack_relu_mask(c > 0)
    yhat = reference.rowdot_cpu(h2, m.w3_bf, float(m.b3[0]))
    dy = (2.0 / nb) * (yhat - yb.float())
    dw3 = reference.coldot_cpu(h2, dy)
    db3 = dy.sum().reshape(1)
    e_g = reference.e5m2_exponent(
        (dy.abs().max() * m.w3_bf.float().abs().max()).item())
    dz2 = reference.expand1d_cpu(dy, m.w3_bf, None, False, m2)
    dz2q = reference.quantize_e5m2_cpu(dz2.float(), e_g)
    if "wgrad" in parts:
        a = reference.e4m3_decode_cpu(h1q.t().contiguous(), m._e_h1_tr)
        b = reference.e5m2_decode_cpu(dz2q.t().contiguous(), e_g)
        dW2 = a @ b.t()
    else:
        dW2 = reference.gemm_tn_bf16_cpu(h1, dz2, out_fp32=True)
    db2 = reference.colsum_cpu(dz2)
    if "dgrad" in parts:
        w2t_q = reference.quantize_e4m3_cpu(m.W2wt_bf, m._e_w2_tr)
        d = (reference.e5m2_decode_cpu(dz2q, e_g)
             @ reference.e4m3_decode_cpu(w2t_q, m._e_w2_tr).t())
        dz1 = (d * reference.unpack_relu_mask(m1, m.hidden)).bfloat16()
    else:
        dz1 = reference.linear_bf16_cpu(dz2, m.W2wt_bf, mask=m1)
    dw1, db1 = reference.coldot_cpu(dz1, xn, also_colsum=True)
    return [dw1, db1, dW2, db2, dw3, db3]


@pytest.mark.parametrize("parts", [("dgrad", "wgrad"), ("dgrad",),
                                   ("wgrad",)])
def test_model_step_grads_equal_oracle_composition(parts):
    m = GPUMLPRegressor(hidden=64, device="cpu", seed=3, fp8_backward=True)
    assert m.fp8_training and m.fp8_backward
    m._fp8_bwd_parts = frozenset(parts)
    xb, yb = _batch(96, 11)
    assert m._use_fp8_bwd(96)
    got = m._step_grads(xb, yb)
    want = _oracle_step_grads(m, xb, yb, parts)
    for g_, w_ in zip(got, want):
        assert g_.dtype == w_.dtype and torch.equal(g_, w_)
    # and it is a different computation from the bf16 backward
    off = GPUMLPRegressor(hidden=64, device="cpu", seed=3, fp8_training=True)
    base = off._step_grads(xb, yb)
    assert not torch.equal(got[2], base[2]) or not torch.equal(got[0], base[0])
    assert torch.equal(m._w2t_q8_tr,
                       ops.quantize_e4m3(m.W2wt_bf, m._e_w2_tr))


def test_model_fit_cpu_stays_finite_and_refreshes_both_shadows():
    m = GPUMLPRegressor(hidden=64, device="cpu", seed=3, fp8_backward=True)
    X, y = _batch(960, 12)
    w2 = m.W2.clone()
    m.fit(X, y, steps=4, batch_size=96)
    assert not torch.equal(m.W2, w2)
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert torch.equal(m._w2_q8_tr, ops.quantize_e4m3(m.W2w_bf, m._e_w2_tr))
    assert torch.equal(m._w2t_q8_tr,
                       ops.quantize_e4m3(m.W2wt_bf, m._e_w2_tr))
    shadow = m._w2t_q8_tr
    m.reinit_(seed=3)
    assert m._w2t_q8_tr is shadow
    assert torch.equal(m._w2t_q8_tr,
                       ops.quantize_e4m3(m.W2wt_bf, m._e_w2_tr))
    other = GPUMLPRegressor(hidden=64, device="cpu", seed=9)
    assert m.copy_weights_from(other)
    assert m._w2t_q8_tr is shadow
    assert torch.equal(m._w2t_q8_tr,
                       ops.quantize_e4m3(m.W2wt_bf, m._e_w2_tr))
    # a batch that is no multiple of 16 takes the bf16 backward
    assert not m._use_fp8_bwd(90) and m._use_fp8_train(90)
    m.fit(X, y, steps=2, batch_size=90)
    assert all(torch.isfinite(p).all() for p in m.parameters())


def test_flag_and_environment_defaults(monkeypatch):
    monkeypatch.delenv("BODYWORK_MLP_FP8_BWD", raising=False)
    monkeypatch.delenv("BODYWORK_MLP_FP8_TRAIN", raising=False)
    m = GPUMLPRegressor(hidden=16)
    assert m.fp8_backward is False and m.fp8_training is False
    assert m._w2t_q8_tr is None and not m._use_fp8_bwd(256)
    assert m._fp8_bwd_parts == {"dgrad", "wgrad"}
    # forward-only flag leaves the backward in bf16
    m = GPUMLPRegressor(hidden=16, fp8_training=True)
    assert m.fp8_backward is False and not m._use_fp8_bwd(256)
    # the backward flag turns the forward on; an explicit False contradicts
    m = GPUMLPRegressor(hidden=16, fp8_backward=True)
    assert m.fp8_backward is True and m.fp8_training is True
    with pytest.raises(ValueError):
        GPUMLPRegressor(hidden=16, fp8_training=False, fp8_backward=True)
    monkeypatch.setenv("BODYWORK_MLP_FP8_BWD", "1")
    m = GPUMLPRegressor(hidden=16)
    assert m.fp8_backward is True and m.fp8_training is True
    assert GPUMLPRegressor(hidden=16, fp8_backward=False).fp8_backward is False
    # explicit arguments beat the environment
    m = GPUMLPRegressor(hidden=16, fp8_training=False)
    assert m.fp8_backward is False and m.fp8_training is False
    sk = GPUMLPRegressor(hidden=16, fp8_backward=False).to_sklearn()
    m = GPUMLPRegressor.from_sklearn(sk)
    assert m.fp8_backward is True and m.fp8_training is True
    monkeypatch.setenv("BODYWORK_MLP_FP8_BWD", "0")
    m = GPUMLPRegressor.from_sklearn(sk)
    assert m.fp8_backward is False and m.fp8_training is False


def test_resolve_model_name():
    from bodywork_mlops_demo_amd.pipeline.loop import resolve_model

    mt, env = resolve_model("mlp-fp8-train-bwd")
    mt0, env0 = resolve_model("mlp-fp8-train")
    assert mt == mt0 == "mlp"
    assert env == dict(env0, BODYWORK_MLP_FP8_BWD="1")
    assert "BODYWORK_MLP_FP8_BWD" not in env0
