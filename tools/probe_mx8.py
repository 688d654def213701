"""Check + bench the MX-fp8 (e4m3, K=128 scaled-MFMA) GEMM (gemm_mx8.hip).

`--check` validates layout/scale semantics EXACTLY with integer-valued
operands (every value e4m3-representable, dot products exact in fp32) and
measures quantisation accuracy on random data; `--bench` prints TFLOP/s
on the hot shapes next to the bf16 8-phase kernel for the A/B;
`--bench-train` / `--bench-bwd` time the fp8 training forward's and
backward's kernels against the bf16 calls they replace.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bodywork_mlops_demo_amd import ops  # noqa: E402


def _quant(x):
    e = ops.e4m3_exponent(x.abs().max().item())
    return ops.quantize_e4m3(x, e), e


def check() -> int:
    fails = []

    # 1. EXACT: small integers are e4m3-representable; with K=512 and
    # |v|<=8 the fp32 accumulation is exact, so any deviation is a
    # layout/scale bug (guide: A=I-check with ASYMMETRIC B).
    g = torch.Generator(device="cuda").manual_seed(7)
    for m, n, k in ((256, 256, 128), (256, 512, 512), (512, 256, 1024)):
        a = torch.randint(-8, 9, (m, k), generator=g,
                          device="cuda").float()
        b = torch.randint(-8, 9, (n, k), generator=g,
                          device="cuda").float()
        want = a @ b.t()
        # explicit e=0 so stored == value exactly
        a8 = ops.quantize_e4m3(a, 0)
        b8 = ops.quantize_e4m3(b, 0)
        got = ops.gemm_mx8_nt(a8, 0, b8, 0, out_fp32=True)
        if not torch.equal(got, want):
            d = (got - want).abs()
            fails.append(f"exact m{m} n{n} k{k}: {int((d > 0).sum())} wrong, "
                         f"maxdiff {d.max().item():.3e}")

    # 2. scale semantics: same integers scaled by 2^5 / 2^-3 through the
    # E8M0 operands must still be EXACT
    m, n, k = 256, 256, 512
    a = torch.randint(-8, 9, (m, k), generator=g, device="cuda").float()
    b = torch.randint(-8, 9, (n, k), generator=g, device="cuda").float()
    a8 = ops.quantize_e4m3(a * 32.0, 5)   # stored = value/2^5 = ints
    b8 = ops.quantize_e4m3(b * 0.125, -3)
    got = ops.gemm_mx8_nt(a8, 5, b8, -3, out_fp32=True)
    want = (a * 32.0) @ (b * 0.125).t()
    if not torch.equal(got, want):
        fails.append(f"scales: maxdiff {(got - want).abs().max().item():.3e}")

    # 3. quantiser matches the CPU oracle (decoded values)
    x = torch.randn(4096, generator=g, device="cuda") * 17.0
    e = ops.e4m3_exponent(x.abs().max().item())
    gq = ops.quantize_e4m3(x, e).cpu()
    cq = ops.quantize_e4m3(x.cpu(), e)
    agree = (gq == cq).float().mean().item()
    if agree < 0.999:  # RNE tie handling may differ on exact ties only
        fails.append(f"quantiser GPU-vs-oracle agreement {agree:.5f}")
    dg = ops.reference.e4m3_decode_cpu(gq, e)
    dc = ops.reference.e4m3_decode_cpu(cq, e)
    md = (dg - dc).abs().max().item()
    if md > 2.0 ** (e - 2):
        fails.append(f"quantiser decoded maxdiff {md:.3e}")

    # 4. random-data accuracy: vs fp32 matmul of the DEQUANTISED operands
    # (isolates MFMA-vs-torch accumulation, should be ~1e-3) and vs the
    # original operands (quantisation error, should be ~1%)
    m, n, k = 512, 512, 4096
    a = torch.randn(m, k, generator=g, device="cuda")
    b = torch.randn(n, k, generator=g, device="cuda")
    a8, ea = _quant(a)
    b8, eb = _quant(b)
    got = ops.gemm_mx8_nt(a8, ea, b8, eb, out_fp32=True)
    deq_a = ops.reference.e4m3_decode_cpu(a8.cpu(), ea).cuda()
    deq_b = ops.reference.e4m3_decode_cpu(b8.cpu(), eb).cuda()
    want_q = deq_a @ deq_b.t()
    rel_q = ((got - want_q).abs().max() /
             want_q.abs().max().clamp_min(1e-6)).item()
    if rel_q > 1e-3:
        fails.append(f"vs-dequantised rel {rel_q:.2e}")
    want = a @ b.t()
    rel = ((got - want).abs().mean() / want.abs().mean()).item()
    print(f"random-data mean rel err vs fp32: {rel:.4f} "
          f"(quantisation; k={k})")
    if rel > 0.05:
        fails.append(f"vs-fp32 mean rel {rel:.3f}")

    # 5. fused bias+relu epilogue
    bias = torch.randn(n, generator=g, device="cuda")
    got = ops.gemm_mx8_nt(a8, ea, b8, eb, bias=bias, relu=True,
                          out_fp32=True)
    want = torch.relu(want_q + bias)
    d = (got - want).abs().max().item()
    if d > 1e-2 * want.abs().max().item():
        fails.append(f"bias+relu maxdiff {d:.3e}")

    for f in fails:
        print("FAIL:", f)
    print("MX8 CHECK", "FAILED" if fails else "OK")
    return 1 if fails else 0


def _time_gemm(fn, iters=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench() -> None:
    g = torch.Generator(device="cuda").manual_seed(3)
    for m, n, k in ((4096, 4096, 4096), (8192, 8192, 8192),
                    (65536, 4096, 4096)):
        a = torch.randn(m, k, generator=g, device="cuda")
        b = torch.randn(n, k, generator=g, device="cuda")
        a8, ea = _quant(a)
        b8, eb = _quant(b)
        abf = a.bfloat16()
        bbf = b.bfloat16()
        fl = 2.0 * m * n * k
        t8 = _time_gemm(lambda: ops.gemm_mx8_nt(a8, ea, b8, eb))
        tb = _time_gemm(lambda: ops.linear_bf16(abf, bbf))
        tq = _time_gemm(lambda: ops.quantize_e4m3(a, ea))
        print(f"{m}x{n}x{k}: mx8 {fl / t8 / 1e12:7.0f} TF | "
              f"bf16 {fl / tb / 1e12:7.0f} TF | ratio {tb / t8:.2f}x | "
              f"quantize A {tq * 1e6:.0f} us ({a.numel() * 4 / tq / 1e9:.0f} "
              f"GB/s read)")


def bench_train_forward(m: int, n: int, k: int) -> None:
    """The fp8 TRAINING forward's h2 GEMM (bf16 out + 1-bit relu mask)
    against the bf16 kernel it replaces, same shape, plus the layer-1
    expand each path needs (dual-emit vs bf16+mask only)."""
    g = torch.Generator(device="cuda").manual_seed(3)
    a = torch.randn(m, k, generator=g, device="cuda").relu_()
    b = torch.randn(n, k, generator=g, device="cuda") * (2.0 / k) ** 0.5
    bias = torch.randn(n, generator=g, device="cuda") * 0.1
    a8, ea = _quant(a)
    b8, eb = _quant(b)
    abf, bbf, bias_bf = a.bfloat16(), b.bfloat16(), bias.bfloat16()
    fl = 2.0 * m * n * k
    t8 = _time_gemm(lambda: ops.gemm_mx8_relu_mask(a8, ea, b8, eb, bias))
    tb = _time_gemm(lambda: ops.linear_relu_mask_bf16(abf, bbf, bias_bf))
    print(f"train-forward {m}x{n}x{k}: gemm_mx8_relu_mask "
          f"{t8 * 1e3:.3f} ms ({fl / t8 / 1e12:.0f} TF) | "
          f"linear_relu_mask_bf16 {tb * 1e3:.3f} ms "
          f"({fl / tb / 1e12:.0f} TF) | ratio {tb / t8:.2f}x")
    x = torch.randn(m, generator=g, device="cuda")
    w1 = torch.randn(k, generator=g, device="cuda").bfloat16()
    b1 = torch.randn(k, generator=g, device="cuda").bfloat16()
    e1 = ops.e4m3_exponent(8.0)
    td = _time_gemm(lambda: ops.expand1d_bf16_e4m3(x, w1, b1, e1))
    te = _time_gemm(lambda: ops.expand1d_bf16(x, w1, b1, relu=True,
                                              emit_mask=True))
    print(f"layer-1 expand {m}x{k}: dual-emit {td * 1e3:.3f} ms | "
          f"bf16+mask {te * 1e3:.3f} ms | extra {(td - te) * 1e3:.3f} ms | "
          f"net forward saving {(tb - t8 - (td - te)) * 1e3:.3f} ms")


def bench_train_backward(m: int, n: int, k: int) -> None:
    """The fp8 TRAINING backward's kernels against the bf16 calls they
    replace, at batch m and hidden n == k: dgrad (e5m2 x e4m3, mask-mul
    epilogue, bf16 out) vs ``linear_bf16(mask=)``; wgrad (two byte
    transposes + e4m3 x e5m2, fp32 out) vs ``gemm_tn_bf16`` (which
    includes its two bf16 transposes); the dual-emit expand vs the bf16
    expand; and the per-step amax kernel."""
    assert n == k, "the backward GEMMs are H x H: pass MxHxH"
    g = torch.Generator(device="cuda").manual_seed(3)
    H = n
    dy = torch.randn(m, generator=g, device="cuda") * (2.0 / m)
    w3 = (torch.randn(H, generator=g, device="cuda")
          * (2.0 / H) ** 0.5).bfloat16()
    W2t = torch.randn(H, H, generator=g, device="cuda") * (2.0 / H) ** 0.5
    h1 = torch.randn(m, H, generator=g, device="cuda").relu_()
    mask1 = torch.randint(0, 256, (m, H // 8), generator=g, device="cuda",
                          dtype=torch.uint8)
    mask2 = torch.randint(0, 256, (m, H // 8), generator=g, device="cuda",
                          dtype=torch.uint8)
    w2q, e_w2 = _quant(W2t)
    h1q, e_h1 = _quant(h1)
    W2t_bf, h1_bf = W2t.bfloat16(), h1.bfloat16()
    fl = 2.0 * m * H * H

    t_amax = _time_gemm(lambda: ops.amax_exponent_e5m2(dy, w3))
    e_g = ops.amax_exponent_e5m2(dy, w3)
    t_ex8 = _time_gemm(lambda: ops.expand1d_bf16_e5m2(dy, w3, mask2, e_g))
    t_exb = _time_gemm(lambda: ops.expand1d_bf16(dy, w3, None, relu=False,
                                                 mask=mask2))
    dz2, dz2q = ops.expand1d_bf16_e5m2(dy, w3, mask2, e_g)
    print(f"amax_exponent_e5m2 n={m} H={H}: {t_amax * 1e3:.3f} ms")
    print(f"expand {m}x{H}: bf16+e5m2 dual emit {t_ex8 * 1e3:.3f} ms | "
          f"bf16 only {t_exb * 1e3:.3f} ms | extra "
          f"{(t_ex8 - t_exb) * 1e3:.3f} ms")

    t_d8 = _time_gemm(lambda: ops.gemm_mx8_nt_fmt(
        dz2q, e_g, w2q, e_w2, "e5m2", "e4m3", mask=mask1))
    t_db = _time_gemm(lambda: ops.linear_bf16(dz2, W2t_bf, mask=mask1))
    print(f"dgrad {m}x{H}x{H}: gemm_mx8_nt_fmt(e5m2,e4m3,mask) "
          f"{t_d8 * 1e3:.3f} ms ({fl / t_d8 / 1e12:.0f} TF) | "
          f"linear_bf16(mask) {t_db * 1e3:.3f} ms "
          f"({fl / t_db / 1e12:.0f} TF) | ratio {t_db / t_d8:.2f}x")

    t_t1 = _time_gemm(lambda: ops.transpose_u8(h1q))
    t_t2 = _time_gemm(lambda: ops.transpose_u8(dz2q))
    h1qt, dz2qt = ops.transpose_u8(h1q), ops.transpose_u8(dz2q)
    t_w8 = _time_gemm(lambda: ops.gemm_mx8_nt_fmt(
        h1qt, e_h1, dz2qt, e_g, "e4m3", "e5m2", out_fp32=True))
    t_wb = _time_gemm(lambda: ops.gemm_tn_bf16(h1_bf, dz2, out_fp32=True))
    t_tb = _time_gemm(lambda: ops.transpose_bf16(h1_bf))
    gb = m * H * 2 / 1e9  # bytes read + written by one byte transpose
    print(f"transpose_u8 {m}x{H}: {t_t1 * 1e3:.3f} ms, {t_t2 * 1e3:.3f} ms "
          f"({gb / t_t1:.0f} GB/s) | transpose_bf16 {t_tb * 1e3:.3f} ms "
          f"({2 * gb / t_tb:.0f} GB/s)")
    t_w8_all = t_w8 + t_t1 + t_t2
    print(f"wgrad {H}x{H}x{m}: gemm_mx8_nt_fmt(e4m3,e5m2,fp32) "
          f"{t_w8 * 1e3:.3f} ms ({fl / t_w8 / 1e12:.0f} TF), with its two "
          f"transposes {t_w8_all * 1e3:.3f} ms | gemm_tn_bf16 (incl. its "
          f"transposes) {t_wb * 1e3:.3f} ms | ratio {t_wb / t_w8_all:.2f}x")
    saved = (t_db - t_d8) + (t_wb - t_w8_all) - (t_ex8 - t_exb) - t_amax
    print(f"net backward saving per step (kernels only, without the second "
          f"W2 shadow's requantisation): {saved * 1e3:.3f} ms")


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--check", action="store_true")
    p.add_argument("--bench", action="store_true")
    p.add_argument("--bench-train", action="store_true",
                   help="time gemm_mx8_relu_mask against "
                        "linear_relu_mask_bf16 at --shape")
    p.add_argument("--bench-bwd", action="store_true",
                   help="time the fp8 backward's kernels (dgrad, wgrad + "
                        "byte transposes, dual-emit expand, amax) against "
                        "the bf16 calls they replace at --shape")
    p.add_argument("--shape", default="65536x4096x4096",
                   help="MxNxK for --bench-train / --bench-bwd")
    args = p.parse_args()
    rc = 0
    if args.check or not (args.bench or args.bench_train
                          or args.bench_bwd):
        rc = check()
    if args.bench:
        bench()
    if args.bench_train:
        bench_train_forward(*(int(v) for v in args.shape.split("x")))
    if args.bench_bwd:
        bench_train_backward(*(int(v) for v in args.shape.split("x")))
    raise SystemExit(rc)


if __name__ == "__main__":
    main()
