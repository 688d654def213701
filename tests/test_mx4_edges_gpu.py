"""MXFP4 kernels at their edges: every K-loop path, the whole E8M0 range,
the quantiser's clamps and non-finite input, the expand and quantiser grid
strides, all six GEMM epilogues and the live-row boundaries.

K-loop coverage of gemm_mxfp4_nt_kernel (nt = K / 256 tiles; the steady loop
runs while t + 3 < nt, then one to three guarded tail phases):

| nt | K    | path                                               | tests  |
|----|------|----------------------------------------------------|--------|
| 1  | 256  | single tile, no B(1) staging, first wait vmcnt(0)  | k e    |
| 2  | 512  | no trip, two-tile tail                             | k (m)  |
| 3  | 768  | no trip, three-tile tail                           | k e p l m |
| 4  | 1024 | one trip + two-tile tail                           | (x)    |
| 5  | 1280 | one trip + three-tile tail after a slot rotation   | k e    |
| 6  | 1536 | two trips + two-tile tail                          | k      |
| 7  | 1792 | two trips + three-tile tail, odd rotation          | k e    |
| 16 | 4096 | seven trips + two-tile tail                        | (a)    |

k = test_kloop_paths_exact_*, e = test_e8m0_range_exact, p =
test_gemm_epilogues_exact, l = test_fused_head_live_row_boundaries; in
test_mx4_gpu.py: x = its exact tests, a = its approximate accuracy test, m =
its model tests (hidden 512; hidden 768 in
test_mlp_fp4_forward_at_an_odd_tile_count).

Every reference is fp64 numpy/torch on the logical operands, built on the
CPU by tests/mx4_data.py; tests/test_mx4_cpu.py checks there that the inputs
are exact in fp32 and that they see a dropped, a doubled and a mis-scaled
K-tile.  The grid inputs repeat their scale pattern every three tiles, so a
tile given the scales of the tile three before it would go unseen there; the
E8M0 inputs (independent exponents per block) at nt = 5 and 7 close that.
"""
import functools

import numpy as np
import pytest
import torch

import mx4_data as data
from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(pair):
    return tuple(t.to(DEV) for t in pair)


def _decode64(q, s):
    return ref.mxfp4_decode_cpu(q.cpu(), s.cpu(), q.shape[1] * 2,
                                dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _kloop_quantised(K):
    """the K-loop case's operands through the device quantiser, checked"""
    case = data.kloop_case(K)
    qa = ops.quantize_mxfp4(case["a"].to(DEV))
    qb = ops.quantize_mxfp4(case["b"].to(DEV))
    assert torch.equal(_decode64(*qa), case["a"].double())
    assert torch.equal(_decode64(*qb), case["b"].double())
    return qa, qb


# ---- 1. every K-loop path, exactly -----------------------------------------

@pytest.mark.parametrize("K", list(data.KLOOP_PATHS))
def test_kloop_paths_exact_512(K):
    """M = N = 512: m0 / n0 are non-zero in three of the four blocks, so the
    nt-dependent scale chunk stride is used at every nt."""
    case = data.kloop_case(K)
    (aq, sa), (bq, sb) = _kloop_quantised(K)
    got = ops.gemm_mxfp4_nt(aq, sa, bq, sb, out_fp32=True).cpu().double()
    assert torch.equal(got, case["c"]), (got - case["c"]).abs().max().item()
    y = ops.gemm_mxfp4_relu_dot(aq, sa, bq, sb, case["b2"].to(DEV),
                                case["w3"].to(DEV)).cpu().double()
    assert torch.equal(y, case["y"]), (y - case["y"]).abs().max().item()


@pytest.mark.parametrize("K", [256, 768])
def test_kloop_paths_exact_one_block(K):
    case = data.kloop_case(K)
    (aq, sa), (bq, sb) = _kloop_quantised(K)
    n = 256 * K // 32  # scale bytes of the first 256 rows: whole row groups
    got = ops.gemm_mxfp4_nt(aq[:256], sa[:n], bq[:256], sb[:n],
                            out_fp32=True).cpu().double()
    assert torch.equal(got, case["c"][:256, :256])
    c = case["c"][:256, :256]
    y_want = torch.relu(c + case["b2"][:256].double()) @ case["w3"][
        :256].double()
    y = ops.gemm_mxfp4_relu_dot(aq[:256], sa[:n], bq[:256], sb[:n],
                                case["b2"][:256].to(DEV),
                                case["w3"][:256].to(DEV)).cpu().double()
    assert torch.equal(y, y_want)


# ---- 2. the whole E8M0 range through the MFMA ------------------------------

@pytest.mark.parametrize("K, variant", [
    (256, "cancel"), (256, "spread"), (768, "cancel"), (768, "spread"),
    (1280, "free"), (1792, "free")])
def test_e8m0_range_exact(K, variant):
    """Operands packed from codes and exponents (no quantiser): scale bytes
    0 and 254 on both operands, a tiny scale against a huge one in one
    product (``cancel``), outputs over 2^+-80 (``spread``).  ``free`` at
    K = 1280 and 1792 has exponents independent per row and block, at the
    tile counts where the grid inputs repeat their scales."""
    case = data.e8m0_case(K, variant)
    (aq, sa), (bq, sb) = _dev(case["aq"]), _dev(case["bq"])
    got = ops.gemm_mxfp4_nt(aq, sa, bq, sb, out_fp32=True).cpu().double()
    bad = got != case["c"]
    print(f"e8m0 {variant} K={K}: {int(bad.sum())} of {bad.numel()} differ")
    assert torch.equal(got, case["c"]), (
        int(bad.sum()), got[bad][:4].tolist(), case["c"][bad][:4].tolist())


# ---- 3. device quantiser = oracle at the edges -----------------------------

@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantiser_edges_equal_oracle(dtype, K):
    x, where = data.edge_input(dtype, K)
    q, s = ops.quantize_mxfp4(x.to(DEV))
    q, s = q.cpu(), s.cpu()
    idx = ref.mxfp4_scale_index(64, K)
    for label, row, blk, pos, byte in where:
        got = int(s[idx[row, blk]])
        assert got == byte, (label, row, blk, got, byte)
    cq, cs = ref.quantize_mxfp4_cpu(x)
    assert torch.equal(s, cs)
    assert torch.equal(q, cq), (q != cq).nonzero()[:8].tolist()


@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantiser_nonfinite_blocks(dtype, K):
    """A block holding an inf or a NaN has scale byte 127, inf saturates to
    +-6, the NaN element follows the oracle's stated rule
    (``ref.E2M1_NAN_CODE``, sign kept), and the 31 finite neighbours get
    exactly the codes of a block whose e is 0 (the finite twin)."""
    x, twin, where = data.nonfinite_input(dtype, K)
    q, s = ops.quantize_mxfp4(x.to(DEV))
    q, s = q.cpu(), s.cpu()
    tq, ts = ref.quantize_mxfp4_cpu(twin)
    idx = ref.mxfp4_scale_index(64, K)
    seen = {}
    for kind, row, blk, pos in where:
        seen.setdefault(kind, set()).add(data.nibble(q, row, 32 * blk + pos))
    print(f"device codes of non-finite elements ({dtype}, K={K}):",
          {k: sorted(v) for k, v in seen.items()})
    for kind, row, blk, pos in where:
        assert int(s[idx[row, blk]]) == 127, (kind, row, blk)
        want = ((8 if kind[0] == "-" else 0)
                | (7 if "inf" in kind else ref.E2M1_NAN_CODE))
        assert data.nibble(q, row, 32 * blk + pos) == want, (kind, row, blk)
    finite = torch.isfinite(x.float())
    assert torch.equal(s, ts)
    assert torch.equal(data.unpack(q)[finite], data.unpack(tq)[finite])
    cq, cs = ref.quantize_mxfp4_cpu(x)
    assert torch.equal(q, cq) and torch.equal(s, cs)


def test_quantiser_second_grid_stride_trip():
    """8192 x 2304 fp32 is 2 359 296 eight-element chunks, more than the
    8192 x 256 threads of the capped grid: the threads of the first 262 144
    chunks take a second trip (from chunk 224 of row 7281 on).  nt = 9 is
    odd.  Compared with the oracle on a SAMPLE of 128 of the 8192 rows:
    the first, the last, rows 7280-7282 around the stride boundary, 64 drawn
    from all rows and 59 more from the second trip's rows."""
    R, K = 8192, 2304
    assert R * K // 8 > 8192 * 256
    boundary = 8192 * 256 // (K // 8)
    assert boundary == 7281 and 8192 * 256 % (K // 8) == 224
    g = torch.Generator(device=DEV).manual_seed(12)
    x = torch.randn(R, K, generator=g, device=DEV)
    x *= (2.0 ** torch.randint(-12, 12, (R, K // 32), generator=g,
                               device=DEV).float()).repeat_interleave(32, 1)
    q, s = ops.quantize_mxfp4(x)
    gc = torch.Generator().manual_seed(13)
    rows = [0, R - 1, boundary - 1, boundary, boundary + 1]
    rows += torch.randperm(R, generator=gc)[:64].tolist()
    rows += (boundary + 2 + torch.randperm(R - boundary - 3, generator=gc)[
        :59]).tolist()
    rows = torch.tensor(rows)
    assert len(rows) == 128
    cq, cs = ref.quantize_mxfp4_cpu(x[rows.to(DEV)].cpu())
    assert torch.equal(q[rows.to(DEV)].cpu(), cq)
    got_s = s.cpu()[ref.mxfp4_scale_index(R, K)[rows]]
    assert torch.equal(got_s, cs[ref.mxfp4_scale_index(128, K)])


# ---- 4. expand shell --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _expand_case(n, H, bias):
    """Exact-arithmetic inputs (x multiples of 1/8, w and b bf16-exact
    multiples of 1/4: fmaf and mul-then-add cannot differ) and the oracle's
    quantisation of the fp64 activation, which fp32 holds exactly."""
    g = torch.Generator().manual_seed(8 + H)
    x = torch.randint(-16, 17, (n,), generator=g) / 8.0
    w = (torch.randint(-16, 17, (H,), generator=g) / 4.0).bfloat16()
    b = (torch.randint(-16, 17, (H,), generator=g) / 4.0).bfloat16()
    h = x.double()[:, None] * w.double()[None, :]
    if bias:
        h = h + b.double()[None, :]
    # max(h, 0) with max(-0, +0) = +0, as IEEE maximum and the kernel's fmaxf
    # have it: without a bias 0 * w is -0 for a negative w, and a relu that
    # kept that sign would put the sign bit into the code
    h = torch.where(h > 0, h, torch.zeros_like(h))
    assert torch.equal(h.float().double(), h)
    return (x, w, (b if bias else None), h.float(),
            ref.quantize_mxfp4_cpu(h.float()))


@pytest.mark.parametrize("n, H, bias, n_dev", [
    (256, 256, True, None), (256, 768, True, None), (256, 256, False, None),
    (256, 768, False, 100), (256, 256, True, 0),
    # n * H / 8 = 786 432 chunks against 2048 x 256 threads: the loop strides
    (8192, 768, True, None), (8192, 768, True, 5000)])
def test_expand1d_shell_equals_oracle(n, H, bias, n_dev):
    x, w, b, h, (wq, ws) = _expand_case(n, H, bias)
    nd = None if n_dev is None else torch.tensor([n_dev], device=DEV)
    xd, wd = x.to(DEV), w.to(DEV)
    bd = None if b is None else b.to(DEV)
    # The op allocates its outputs.  Fill and release blocks of their sizes
    # first: where the allocator hands the same memory back, the dead rows
    # can be checked for being untouched; where it does not, only the live
    # rows and live scale bytes are compared, as in test_mx4_gpu.py.
    fill = [torch.full((size,), 0xA5, dtype=torch.uint8, device=DEV)
            for size in (n * H // 2, n * H // 32)]
    ptrs = [t.data_ptr() for t in fill]
    del fill
    q, s = ops.expand1d_mxfp4(xd, wd, bd, n_dev=nd)
    reused = [q.data_ptr(), s.data_ptr()] == ptrs
    q, s = q.cpu(), s.cpu()
    live = n if n_dev is None else n_dev
    index = ref.mxfp4_scale_index(n, H)
    idx = index[:live].reshape(-1)
    bad = data.unpack(q[:live]) != data.unpack(wq[:live])
    assert not bad.any(), (  # (row, column), activation, got, want
        bad.nonzero()[:4].tolist(), h[:live][bad][:4].tolist(),
        data.unpack(q[:live])[bad][:4].tolist(),
        data.unpack(wq[:live])[bad][:4].tolist())
    assert torch.equal(s[idx], ws[idx])
    print(f"expand n={n} H={H} n_dev={n_dev}: dead rows checked: {reused}")
    if reused:
        assert (q[live:] == 0xA5).all()
        assert (s[index[live:].reshape(-1)] == 0xA5).all()


# ---- 5. epilogues and live rows --------------------------------------------

@pytest.mark.parametrize("out_fp32", [True, False])
@pytest.mark.parametrize("epilogue", ["plain", "relu", "bias_relu"])
def test_gemm_epilogues_exact(epilogue, out_fp32):
    """256 x 256 x 768 on the K-loop inputs.  The fp32 value is exact, so a
    bf16 output is one RNE of the same number on both sides."""
    K = 768
    case = data.kloop_case(K)
    (aq, sa), (bq, sb) = _kloop_quantised(K)
    n = 256 * K // 32
    aq, sa, bq, sb = aq[:256], sa[:n], bq[:256], sb[:n]
    bias = case["b2"][:256] if epilogue == "bias_relu" else None
    relu = epilogue != "plain"
    pre = case["c"][:256, :256] + (0 if bias is None else bias.double())
    assert (pre < 0).any() and (pre > 0).any()  # relu clips and passes
    want64 = torch.relu(pre) if relu else pre
    want = want64.float() if out_fp32 else want64.float().bfloat16()
    oracle = ref.gemm_mxfp4_nt_cpu(aq.cpu(), sa.cpu(), bq.cpu(), sb.cpu(),
                                   bias, relu, out_fp32)
    assert torch.equal(oracle, want)
    got = ops.gemm_mxfp4_nt(aq, sa, bq, sb,
                            None if bias is None else bias.to(DEV), relu,
                            out_fp32)
    assert got.dtype == want.dtype
    assert torch.equal(got.cpu(), oracle)
    if relu:
        assert (got == 0).any() and (got > 0).any()


@pytest.mark.parametrize("n_dev", [1, 255, 256, 257, 511, 10_000])
def test_fused_head_live_row_boundaries(n_dev):
    """M = N = 512, K = 768: a single live row, either side of the 256-row
    tile boundary and the boundary itself (the second row tile returns at
    once), one short of M, and a count above M (clamped).  Dead rows hold
    all-ones codes and NaN scales."""
    K, M = 768, 512
    case = data.kloop_case(K)
    (aq, sa), (bq, sb) = _kloop_quantised(K)
    live = min(n_dev, M)
    aq, sa = aq.clone(), sa.clone()
    aq[live:] = 0xFF
    sa[ref.mxfp4_scale_index(M, K)[live:].reshape(-1).to(DEV)] = 0xFF
    got = ops.gemm_mxfp4_relu_dot(
        aq, sa, bq, sb, case["b2"].to(DEV), case["w3"].to(DEV),
        n_dev=torch.tensor([n_dev], device=DEV)).cpu().double()
    assert torch.equal(got[:live], case["y"][:live])
    assert (got[live:] == 0).all()
