"""Flagship benchmark — the driver contract.

Measures BASELINE.json's headline metric on MI355X: scoring rows/sec
through the stage-2 path with the full train->serve->drift->test cycle as
the step (`ms_per_step` = cycle wall-clock).  One step = one pipeline
"day" on `--rows` synthetic rows per GPU (weak scaling):

  stage 1  train on the day's rows (fused-stats OLS or MFMA-GEMM MLP,
           DP all-reduce over RCCL when N>1)
  stage 2  deploy: joblib artefact round-trip -> model into HBM,
           hipGraph-captured batch scoring
  stage 3  generate day t+1 on-GPU (philox drift kernel + compaction)
  stage 4  score day t+1 through the deployed scorer + fused metrics,
           persist test-metrics artefact

Launch (driver): python -m torch.distributed.run --nnodes=1
  --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...
Rank 0 prints ONE JSON line; `value` is whole-job rows/sec scored.

A plain run sets up, warms up, times `--steps` cycles and prints the
line.  `--dump-outputs DIR` additionally writes what the last timed cycle
computed as `DIR/<name>.npy` (inputs are seeded by date and rank, so two
builds run with the same arguments can be compared array for array; the
fp64 reductions use atomics, so metrics and fitted coefficients agree to
rounding, ~1e-13 relative, not bit for bit).  `--full` is where secondary
measurements belong; there are none at present.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import tempfile
from datetime import date
from time import perf_counter

import torch


DUMP_SAMPLE = 1 << 20  # elements kept per large array (4 MiB as float32)
METRIC_KEYS = ("MAPE", "r_squared", "max_residual")


def _dump_outputs(out_dir: str, result: dict, captured: dict) -> None:
    """Write what the last timed cycle computed as ``out_dir/<name>.npy``.

    ``X``/``labels`` are stage 3's day-t+1 rows, ``scores`` the deployed
    scorer's predictions for them, ``model_params`` the stage-1 fit and
    ``*_metrics`` the fused MAPE / r_squared / max_residual reductions
    (wall-clock fields are left out: they differ from run to run).  Arrays
    longer than DUMP_SAMPLE are written as a fixed seeded sample — the same
    indices for the three per-row arrays — so the dump stays a few MiB
    at any --rows."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)

    def sample(t: torch.Tensor) -> "np.ndarray":
        flat = t.detach().reshape(-1)
        if flat.numel() > DUMP_SAMPLE:
            idx = np.sort(np.random.default_rng(0).integers(
                0, flat.numel(), size=DUMP_SAMPLE))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        return flat.float().cpu().numpy()

    for name in ("X", "labels", "scores"):
        np.save(os.path.join(out_dir, f"{name}.npy"), sample(captured[name]))
    for name, metrics in (("online_metrics", result["online"]),
                          ("offline_metrics", result["offline"])):
        np.save(os.path.join(out_dir, f"{name}.npy"),
                np.array([metrics[k] for k in METRIC_KEYS], dtype=np.float64))
    model = captured.get("model")
    if hasattr(model, "intercept_"):  # linear: [intercept, coef]
        params = np.array([model.intercept_, model.coef_], dtype=np.float64)
    elif hasattr(model, "coef_t_"):  # polynomial ridge, normalised basis
        params = np.asarray(model.coef_t_, dtype=np.float64)
    elif model is not None:  # MLP: small vectors whole, W2 sampled
        params = np.concatenate([sample(t) for t in model.parameters()])
    else:
        return
    np.save(os.path.join(out_dir, "model_params.npy"), params)


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    # default timed region is ~20 cycles so external GPU-utilisation
    # samplers (the driver polls rocm-smi) can catch the run
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--rows", type=int, default=10_000_000,
                   help="synthetic rows per GPU per day (BASELINE config 2)")
    p.add_argument("--model", default="linear",
                   help="linear | poly[<degree>] | mlp | mlp-fp8 "
                        "(mlp = BASELINE config 5, 4096-d MFMA GEMM path; "
                        "mlp-fp8 adds the 2x-rate MX-fp8 scoring forward)")
    p.add_argument("--mlp-steps", type=int, default=50)
    p.add_argument("--mlp-batch", type=int, default=65536)
    p.add_argument("--no-graphs", action="store_true")
    p.add_argument("--store", default=None,
                   help="artefact store dir (default: fresh tmpdir)")
    p.add_argument("--serving", default="inprocess",
                   choices=["inprocess", "http"],
                   help="http = deploy a real uvicorn replica per rank and "
                        "drive stage 4 over the wire (mean_response_time "
                        "keeps its reference meaning, stage_4:105,111); "
                        "inprocess = resident BatchedScorer, no HTTP in "
                        "the timed region")
    p.add_argument("--http-mode", default="binary",
                   choices=["binary", "batch", "serial"],
                   help="wire format for --serving http")
    p.add_argument("--history", default="1",
                   help="training window in days, or 'all' for the "
                        "reference's read-all-accumulated-data semantics "
                        "(stage_1:59-71; history grows by --rows each step)")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="after the timed steps, write what the last timed "
                        "step computed (rank 0's shard) to DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements; a plain run "
                        "does only what the headline figure needs (there "
                        "are none at present: other models, sizes and "
                        "serving modes are runs of their own)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")
    history_days = None if args.history == "all" else int(args.history)

    # mlp-fp8: the MLP with MX-fp8 scoring forward (K=128 scaled MFMA,
    # measured 1.5-1.6x the bf16 GEMM rate).  The flag is an env var so
    # the DEPLOYED scorer model (reconstructed from the artefact in the
    # serving path) opts in too, not just the trainer.
    fp8_scoring = args.model == "mlp-fp8"
    if fp8_scoring:
        os.environ["BODYWORK_MLP_FP8"] = "1"
        args.model = "mlp"

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    if world > 1 and args.gpus != world:
        args.gpus = world

    use_cuda = torch.cuda.is_available()
    # modulo mapping lets world > device_count oversubscribe (e.g. the
    # world=2-on-one-GPU RCCL rehearsal for the 8-GPU scale run)
    dev_idx = local_rank % torch.cuda.device_count() if use_cuda else 0
    device = f"cuda:{dev_idx}" if use_cuda else "cpu"

    if use_cuda:
        # the HIP extension is the compute path — fail loudly if missing
        from bodywork_mlops_demo_amd import ops

        if not ops.hip_available():
            raise RuntimeError(
                "bench requires the in-tree _hipcore HIP extension on GPU; "
                "build with: PYTORCH_ROCM_ARCH=gfx950 python setup.py "
                "build_ext --inplace"
            )
        torch.cuda.set_device(dev_idx)

    pg = None
    if world > 1:
        import torch.distributed as dist

        from bodywork_mlops_demo_amd.parallel import init_distributed

        init_distributed()
        pg = dist.group.WORLD

    from bodywork_mlops_demo_amd.pipeline.cycle import CycleState, run_cycle
    from bodywork_mlops_demo_amd.store import LocalStore

    # shared store dir across ranks; the default is per user (another
    # user's leftover dir could not be cleared) and is removed at exit
    if args.store:
        store_dir = args.store
    else:
        store_dir = os.path.join(
            tempfile.gettempdir(),
            f"bodywork_bench_{os.getuid()}_"
            f"{os.environ.get('MASTER_PORT', 'solo')}",
        )
    if rank == 0:
        shutil.rmtree(store_dir, ignore_errors=True)
        os.makedirs(store_dir, exist_ok=True)
    if pg is not None:
        torch.distributed.barrier(pg)
    store = LocalStore(store_dir)

    state = CycleState(device, date(2026, 1, 1), rank=rank, world_size=world,
                       history_days=history_days)
    scorer_cache: dict = {}

    def one_cycle(capture=None):
        return run_cycle(
            state, store, args.rows, model_type=args.model,
            process_group=pg, persist_fmt="npy",
            mlp_steps=args.mlp_steps, mlp_batch_size=args.mlp_batch,
            use_graphs=not args.no_graphs and use_cuda,
            scorer_cache=scorer_cache,
            serving=args.serving, http_mode=args.http_mode,
            capture=capture,
        )

    def barrier_sync():
        if pg is not None:
            torch.distributed.barrier(pg)
        if use_cuda:
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        one_cycle()

    barrier_sync()
    t0 = perf_counter()
    rows_scored = 0
    last = None
    # the last timed step hands out references to its tensors (no copies,
    # no extra launches) so --dump-outputs can write them after the clock
    captured: dict | None = {} if args.dump_outputs and rank == 0 else None
    for i in range(args.steps):
        last = one_cycle(captured if i == args.steps - 1 else None)
        rows_scored += last["timings"]["rows_scored"]
    state.drain_io()  # async artefact writes are part of the timed work
    barrier_sync()
    elapsed = perf_counter() - t0

    # max elapsed over ranks, total rows over ranks
    if pg is not None:
        buf = torch.tensor([elapsed], dtype=torch.float64,
                           device=device if use_cuda else "cpu")
        torch.distributed.all_reduce(buf, op=torch.distributed.ReduceOp.MAX,
                                     group=pg)
        elapsed = float(buf.item())
        rbuf = torch.tensor([float(rows_scored)], dtype=torch.float64,
                            device=device if use_cuda else "cpu")
        torch.distributed.all_reduce(rbuf, group=pg)
        rows_scored = int(rbuf.item())

    replica = scorer_cache.get("http_replica")
    if replica is not None:
        replica.stop()

    if captured is not None:
        _dump_outputs(args.dump_outputs, last, captured)

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1000.0
        value = rows_scored / elapsed
        serving_desc = (
            f"1 uvicorn replica/GPU, {args.http_mode} wire over HTTP"
            if args.serving == "http"
            else "1 in-process replica/GPU, hipGraph-captured batches"
        )
        print(json.dumps({
            "metric": "rows/sec scored (stage_2 path, full "
                      "train-serve-drift-test cycle"
                      + (", over-the-wire HTTP serving)"
                         if args.serving == "http" else ")"),
            "value": value,
            "unit": "rows/s",
            "n_gpus": args.gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": ("bf16 train + fp8(e4m3) scoring" if fp8_scoring
                      else "bf16" if args.model == "mlp" else "fp32"),
            "data": "synthetic (on-GPU philox drift generator, "
                    f"{args.rows} rows/GPU/day, random-init weights"
                    + (", growing read-all training history"
                       if history_days is None else "") + ")",
            "config": {
                "model": ("mlp-4096x2-fp8scoring" if fp8_scoring
                          else {"linear": "linear-ols",
                                "mlp": "mlp-4096x2"}.get(args.model,
                                                         args.model)),
                "rows_per_gpu_per_day": args.rows,
                "history_days": args.history,
                "parallelism": f"dp{args.gpus}",
                "serving": serving_desc,
                "train_phase": ("adam bf16 MFMA GEMM, "
                                f"{args.mlp_steps}x{args.mlp_batch}"
                                if args.model == "mlp"
                                else "fused-stats closed-form OLS"),
                "online_mape": (last["online"]["MAPE"] if last else None),
                "phase_ms": {
                    k: round(v * 1000.0, 3)
                    for k, v in (last["timings"].items() if last else [])
                    if k.endswith("_s")
                },
            },
        }))

    if pg is not None:
        torch.distributed.barrier(pg)
        torch.distributed.destroy_process_group()
    if rank == 0 and not args.store:
        shutil.rmtree(store_dir, ignore_errors=True)


if __name__ == "__main__":
    main()
