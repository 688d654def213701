"""Replay time of the MLP scorer's 1- and 16-row buckets, skinny flag on
against off, in one process.

Two same-seed ``GPUMLPRegressor(hidden=H)``, one with ``skinny_scoring``,
a ``BatchedScorer`` over each, buckets 1 and 16 captured.  Per bucket the
two captured graphs are replayed in alternating blocks of ``--replays``
back-to-back replays, device events around each block, ``--rounds`` times;
per (bucket, variant) the microseconds per replay of every round are
printed, and for the skinny path the implied weight rate ``H*H*2 bytes /
time``.  Back-to-back replays re-read a weight matrix that fits in the
last-level cache: a hot steady state, not a cold HBM stream.

    python tools/skinny_latency.py [--hidden 4096] [--replays 2000]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--hidden", type=int, default=4096)
    p.add_argument("--replays", type=int, default=2000)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=200)
    args = p.parse_args()

    import torch

    from bodywork_mlops_demo_amd.models import GPUMLPRegressor
    from bodywork_mlops_demo_amd.serving.scorer import BatchedScorer

    assert torch.cuda.is_available(), "skinny_latency needs a GPU"
    dev = "cuda:0"
    g = torch.Generator(device="cpu").manual_seed(1)
    rows = (torch.rand(16, generator=g) * 100).to(dev)
    graphs: dict = {}
    outs: dict = {}
    for variant, flag in (("unfused", False), ("skinny", True)):
        model = GPUMLPRegressor(hidden=args.hidden, device=dev, seed=7,
                                skinny_scoring=flag)
        scorer = BatchedScorer(model, dev, use_graphs=True)
        for b in (1, 16):
            outs[b, variant] = scorer.score_tensor(rows[:b])
            assert scorer.use_graphs, "graph capture fell back"
            graphs[b, variant] = scorer._graphs[b][0]
        graphs[variant] = scorer  # keeps the static buffers alive
    for b in (1, 16):
        d = (outs[b, "skinny"] - outs[b, "unfused"]).abs().max().item()
        print(f"bucket {b}: max |skinny - unfused| = {d:.3e} "
              f"(max |y| {outs[b, 'unfused'].abs().max().item():.3f})")

    wbytes = args.hidden * args.hidden * 2
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    result = {"hidden": args.hidden, "replays": args.replays}
    for b in (1, 16):
        us = {"unfused": [], "skinny": []}
        for variant in us:
            for _ in range(args.warmup):
                graphs[b, variant].replay()
        for _ in range(args.rounds):
            for variant in us:
                graph = graphs[b, variant]
                start.record()
                for _ in range(args.replays):
                    graph.replay()
                stop.record()
                stop.synchronize()
                us[variant].append(
                    start.elapsed_time(stop) * 1e3 / args.replays)
        for variant, v in us.items():
            med = sorted(v)[len(v) // 2]
            line = (f"bucket {b:2d} {variant:8s} us/replay by round: "
                    + ", ".join(f"{t:.2f}" for t in v)
                    + f"  median {med:.2f}")
            if variant == "skinny":
                line += f"  weights {wbytes / med / 1e6:.2f} TB/s"
            print(line)
            result[f"b{b}_{variant}_us"] = [round(t, 3) for t in v]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
