"""Time the fp8 and fp4 scoring kernels alternately (H = 4096).

Per M: the fused heads ``gemm_mx8_relu_dot`` / ``gemm_mxfp4_relu_dot`` and
the layer-1 expands ``expand1d_e4m3`` / ``expand1d_mxfp4``, torch events
around single launches after two warm-up calls, ``--reps`` rounds in which
the four take turns; prints median [min, max] ms and the heads' FLOP/s.

    python tools/probe_mx4.py --m 65536 1048576
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bodywork_mlops_demo_amd import ops  # noqa: E402

DEV = "cuda"
H = 4096


def alternate(fns, reps):
    res = {k: [] for k in fns}
    for f in fns.values():
        f()
        f()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, f in fns.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            res[k].append(a.elapsed_time(b))
    return res


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--m", type=int, nargs="+", default=[65536, 1 << 20])
    p.add_argument("--reps", type=int, default=7)
    args = p.parse_args()
    g = torch.Generator(device=DEV).manual_seed(0)
    w = torch.randn(H, generator=g, device=DEV).bfloat16()
    b = torch.randn(H, generator=g, device=DEV).bfloat16()
    W2 = (torch.randn(H, H, generator=g, device=DEV) * 0.02).bfloat16()
    b2 = torch.randn(H, generator=g, device=DEV)
    w3 = torch.randn(H, generator=g, device=DEV)
    w8, w4 = ops.quantize_e4m3(W2, -6), ops.quantize_mxfp4(W2)
    for M in args.m:
        x = torch.randn(M, generator=g, device=DEV)
        h8, h4 = ops.expand1d_e4m3(x, w, b, 3), ops.expand1d_mxfp4(x, w, b)
        res = alternate({
            "head fp8": lambda: ops.gemm_mx8_relu_dot(h8, 3, w8, -6, b2, w3),
            "head fp4": lambda: ops.gemm_mxfp4_relu_dot(*h4, *w4, b2, w3),
            "expand e4m3": lambda: ops.expand1d_e4m3(x, w, b, 3),
            "expand mxfp4": lambda: ops.expand1d_mxfp4(x, w, b),
        }, args.reps)
        for k, v in res.items():
            med = statistics.median(v)
            tf = (f" = {2.0 * M * H * H / (med * 1e-3) / 1e12:.0f} TF"
                  if k.startswith("head") else "")
            print(f"M={M} {k}: {med:.3f} [{min(v):.3f}, {max(v):.3f}] ms{tf}",
                  flush=True)


if __name__ == "__main__":
    main()
