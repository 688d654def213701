"""Replay time of the MLP scorer's small buckets, a one-kernel flag on
against off, in one process.

Two same-seed ``GPUMLPRegressor(hidden=H)``, one with ``--flag`` (``skinny``:
``skinny_scoring``, the 1- and 16-row buckets; ``mid``: ``mid_scoring``, the
256-row bucket; ``skinny_fp4``: ``skinny_fp4``, the same two buckets on the
MXFP4 weights, timed against the bf16 ``skinny`` variant instead of the
unfused path; ``mid_fp4``: ``mid_fp4``, the 256-row bucket on the MXFP4
weights, timed against both the bf16 ``mid`` variant and ``fp4_tile``, the
``fp4_scoring`` model's tile-gated path), a ``BatchedScorer`` over each.
``--cases`` lists
``bucket:live`` pairs: the bucket is captured by a request of ``live`` rows,
so the graph's device-side row count stays at ``live`` for the replays.
Per case the variants' captured graphs are replayed in alternating blocks of
``--replays`` back-to-back replays, device events around each block,
``--rounds`` times; per (case, variant) the microseconds per replay of every
round, their median and their spread are printed, and for the flagged path
the implied weight rate, ``H*H*2`` bytes (MXFP4: ``H*H*17/32``) over the
time.  Back-to-back replays re-read
a weight matrix that fits in the last-level cache: a hot steady state, not a
cold HBM stream.  Every (case, variant) has a model and a scorer of its own;
the figures in profiles/skinny_scoring.md were taken with an earlier
arrangement, one scorer per variant holding both buckets (the replayed
graphs are the same).

    python tools/skinny_latency.py [--hidden 4096] [--replays 2000]
    python tools/skinny_latency.py --flag mid [--cases 256:17,256:256]
    python tools/skinny_latency.py --flag skinny_fp4
    python tools/skinny_latency.py --flag mid_fp4
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEFAULT_CASES = {"skinny": "1:1,16:16",
                 "mid": "256:17,256:64,256:128,256:256",
                 "skinny_fp4": "1:1,16:16",
                 "mid_fp4": "256:17,256:64,256:128,256:256"}
#: variant -> the model flags it sets, and the bytes of W2 it streams per H*H
VARIANTS = {"unfused": ({}, None),
            "skinny": ({"skinny_scoring": True}, 2.0),
            "mid": ({"mid_scoring": True}, 2.0),
            "skinny_fp4": ({"skinny_fp4": True}, 17 / 32),
            "fp4_tile": ({"fp4_scoring": True}, None),
            "mid_fp4": ({"mid_fp4": True}, 17 / 32)}
#: what a flag is timed against (and its results compared with)
BASELINE = {"skinny": ("unfused",), "mid": ("unfused",),
            "skinny_fp4": ("skinny",), "mid_fp4": ("mid", "fp4_tile")}


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--flag", choices=sorted(DEFAULT_CASES), default="skinny")
    p.add_argument("--cases", default=None,
                   help="bucket:live pairs, e.g. 256:17,256:256")
    p.add_argument("--hidden", type=int, default=4096)
    p.add_argument("--replays", type=int, default=2000)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=200)
    args = p.parse_args()
    cases = [tuple(int(v) for v in c.split(":"))
             for c in (args.cases or DEFAULT_CASES[args.flag]).split(",")]

    import torch

    from bodywork_mlops_demo_amd.models import GPUMLPRegressor
    from bodywork_mlops_demo_amd.serving.scorer import BatchedScorer

    assert torch.cuda.is_available(), "skinny_latency needs a GPU"
    dev = "cuda:0"
    g = torch.Generator(device="cpu").manual_seed(1)
    rows = (torch.rand(max(b for b, _ in cases), generator=g) * 100).to(dev)
    variants = BASELINE[args.flag] + (args.flag,)
    graphs: dict = {}
    outs: dict = {}
    keep = []  # the scorers own the graphs' static buffers
    for b, live in cases:
        assert 1 <= live <= b, f"case {b}:{live}"
        for variant in variants:
            model = GPUMLPRegressor(hidden=args.hidden, device=dev, seed=7,
                                    **VARIANTS[variant][0])
            # one scorer per case: its bucket keeps this live count
            scorer = BatchedScorer(model, dev, use_graphs=True)
            outs[b, live, variant] = scorer.score_tensor(rows[:live])
            assert scorer.use_graphs, "graph capture fell back"
            assert sorted(scorer._graphs) == [b], (b, sorted(scorer._graphs))
            graphs[b, live, variant] = scorer._graphs[b][0]
            keep.append(scorer)
        for base in BASELINE[args.flag]:
            ref = outs[b, live, base]
            d = (outs[b, live, args.flag] - ref).abs().max().item()
            print(f"bucket {b} live {live}: max |{args.flag} - {base}| = "
                  f"{d:.3e} (max |y| {ref.abs().max().item():.3f})")

    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    result = {"hidden": args.hidden, "replays": args.replays,
              "flag": args.flag}
    for b, live in cases:
        us = {variant: [] for variant in variants}
        for variant in us:
            for _ in range(args.warmup):
                graphs[b, live, variant].replay()
        for _ in range(args.rounds):
            for variant in us:
                graph = graphs[b, live, variant]
                start.record()
                for _ in range(args.replays):
                    graph.replay()
                stop.record()
                stop.synchronize()
                us[variant].append(
                    start.elapsed_time(stop) * 1e3 / args.replays)
        for variant, v in us.items():
            med = sorted(v)[len(v) // 2]
            line = (f"bucket {b:3d} live {live:3d} {variant:10s} us/replay by "
                    "round: " + ", ".join(f"{t:.2f}" for t in v)
                    + f"  median {med:.2f}  spread {max(v) - min(v):.2f}")
            if VARIANTS[variant][1]:
                wbytes = args.hidden * args.hidden * VARIANTS[variant][1]
                line += f"  weights {wbytes / med / 1e6:.2f} TB/s"
            print(line)
            result[f"b{b}_n{live}_{variant}_us"] = [round(t, 3) for t in v]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
