"""The three bf16 GEMM kernels answer to one oracle, exactly.

``linear_bf16`` picks its kernel by shape (``BODYWORK_GEMM_8PHASE`` is read
once per process, so a test cannot toggle it); all three end in the same
wave-tile epilogue (ops/hip/mfma_tile.h):

    (200, 144,  96)  K % 64 != 0           -> register-staged fallback kernel
    (200, 144, 128)  K % 64 == 0           -> 128^2 glds kernel
    (256, 512, 256)  256-tiled, K >= 256   -> 8-phase kernel, two column tiles

N = 144 leaves the second column tile a 16-column stripe, so the mask-multiply
epilogue takes its byte-wise gather there (the whole-stripe u64 read
elsewhere); M = 200 leaves a partial row tile.

Operands are integers in [-3, 3], the bias integers in [-4, 4]: every partial
sum is an integer of magnitude <= 9*K + 4 <= 2308 < 2^24, so fp32 accumulation
is exact in any order, the bf16 results are one RNE rounding of the same fp32
value on both sides, and ``torch.equal`` is the comparison (-0.0 == 0.0 under
it, which the mask-multiply oracle's ``c * 0`` needs).

colsum/coldot: 130 rows x 264 columns of integers in [-3, 3] (two row chunks
of 65 = a 4-row unrolled part and a tail each; 264 columns = 33 of the
block's 256 threads); sums <= 390 and dots <= 1170 are exact.
"""
import functools

import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.ops import reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(200, 144, 96), (200, 144, 128), (256, 512, 256)]
# the shapes linear_relu_mask_bf16 accepts (K % 64 == 0 and N % 16 == 0)
EMIT_SHAPES = [s for s in SHAPES if s[2] % 64 == 0 and s[1] % 16 == 0]
MODES = ["plain", "bias_relu", "mask_mul"]


def _ints(shape, lo, hi, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).bfloat16()


def _id(shape):
    return "x".join(map(str, shape))


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Operands (host and device) and the relu mask of one shape; built once
    per shape and never modified."""
    M, N, K = shape
    x, w = _ints((M, K), -3, 3, 11), _ints((N, K), -3, 3, 12)
    bias = _ints((N,), -4, 4, 13)
    acc = x.float() @ w.float().t()
    assert acc.abs().max() + 4 < 2 ** 24
    mask = reference.pack_relu_mask(acc + bias.float() > 0)
    live = reference.unpack_relu_mask(mask, N)
    assert live.any() and not live.all()
    return {
        "x": x, "w": w, "bias": bias, "mask": mask,
        "xd": x.to(DEV), "wd": w.to(DEV), "biasd": bias.to(DEV),
        "maskd": mask.to(DEV),
    }


def _args(c, mode, dev):
    s = "d" if dev else ""
    if mode == "bias_relu":
        return {"bias": c["bias" + s], "relu": True}
    if mode == "mask_mul":
        return {"mask": c["mask" + s]}
    return {}


@pytest.mark.parametrize("out_fp32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_linear_bf16_exact(shape, mode, out_fp32):
    case = _case(shape)
    got = ops.linear_bf16(case["xd"], case["wd"], out_fp32=out_fp32,
                          **_args(case, mode, True))
    want = reference.linear_bf16_cpu(case["x"], case["w"], out_fp32=out_fp32,
                                     **_args(case, mode, False))
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("shape", EMIT_SHAPES, ids=_id)
def test_relu_mask_matches_bias_relu(shape):
    case = _case(shape)
    out, mask = ops.linear_relu_mask_bf16(case["xd"], case["wd"],
                                          case["biasd"])
    want, want_mask = reference.linear_relu_mask_cpu(case["x"], case["w"],
                                                     case["bias"])
    plain = ops.linear_bf16(case["xd"], case["wd"], case["biasd"], relu=True)
    assert torch.equal(out, plain)
    assert torch.equal(out.cpu(), want)
    assert torch.equal(mask.cpu(), reference.pack_relu_mask(out.cpu() > 0))
    assert torch.equal(mask.cpu(), want_mask)


@pytest.mark.parametrize("out_fp32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", EMIT_SHAPES, ids=_id)
def test_emitted_mask_fed_back(shape, out_fp32):
    case = _case(shape)
    out, mask = ops.linear_relu_mask_bf16(case["xd"], case["wd"],
                                          case["biasd"])
    got = ops.linear_bf16(case["xd"], case["wd"], mask=mask,
                          out_fp32=out_fp32)
    plain = ops.linear_bf16(case["xd"], case["wd"], out_fp32=out_fp32)
    assert torch.equal(got, torch.where(out > 0, plain,
                                        torch.zeros_like(plain)))


def test_colsum_equals_coldot_colsum_half():
    m = _ints((130, 264), -3, 3, 21)
    v = _ints((130,), -3, 3, 22).float()
    md, vd = m.to(DEV), v.to(DEV)
    cs = ops.colsum_bf16(md)
    dw, cs2 = ops.coldot_bf16(md, vd, also_colsum=True)
    assert torch.equal(cs, cs2)
    assert torch.equal(cs.cpu(), reference.colsum_cpu(m))
    assert torch.equal(dw.cpu(), reference.coldot_cpu(m, v))
    assert torch.equal(ops.coldot_bf16(md, vd), dw)
