#!/usr/bin/env python3
"""Serving/scoring throughput bench — the eval-side counterpart of bench.py.

The reference scores eval sets through the Java `Computable` one row at a
time (shifu-tensorflow-eval/.../TensorflowModel.java:52-94).  This measures
our ShifuScorer on an exported bundle — the headline Wide&Deep (default) or,
with --family mlp, the dense net the reference's eval side nearly always
serves (TrainParams default [50, 50] tanh):

  * compute()        — per-row latency (the Java call pattern)
  * compute_batch()  — batched scoring rows/s (CPU and, with --device cuda,
                       the GPU path the batch scorer `shifu_amd.score` uses)
  * --family mlp --device cuda also reports the device time of predict()
    alone (HIP events, resident input, median of --repeats)

--fused routes an MLP bundle through the single-kernel scoring path
(shifu_amd/ops/fused_mlp.py); without it the per-layer kernels run.
--ensemble M (with --family mlp) scores a bagged set of M such nets (seeds
11 .. 11+M-1, exported with export_ensemble); every line then carries "members".

Synthetic model + data (no network).  One JSON line per mode.
Usage: python tools/score_bench.py [--device cuda] [--batch 65536]
                                   [--family mlp [--fused] [--hidden 50,50]
                                    [--ensemble M]]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch


def _predict_device_time(sc, dense, batch, repeats, fused, model_desc,
                         extra):
    """Device time of model.predict on one resident batch: HIP events around
    predict alone, one warm-up, median of `repeats`."""
    x = torch.tensor(dense[:batch], device="cuda")
    sc.model.predict(x)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        sc.model.predict(x)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    times.sort()
    med = times[len(times) // 2]
    print(json.dumps({
        "metric": "predict_device_time_us", "value": med, "unit": "us/batch",
        "mode": "predict", "device": "cuda", "batch": int(x.shape[0]),
        "repeats": repeats, "min_us": times[0], "max_us": times[-1],
        "input_gb_per_s": x.numel() * 4 / (med * 1e-6) / 1e9,
        "higher_is_better": False, "fused": fused,
        "config": {"model": model_desc}, **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--n-cat", type=int, default=26)
    ap.add_argument("--n-dense", type=int, default=200)
    ap.add_argument("--vocab", type=int, default=100000)
    ap.add_argument("--embed-dim", type=int, default=64)
    ap.add_argument("--family", choices=["wide_deep", "mlp"], default="wide_deep")
    ap.add_argument("--hidden", default="50,50",
                    help="--family mlp: hidden layer widths (tanh)")
    ap.add_argument("--fused", action="store_true",
                    help="--family mlp: single-kernel scoring path")
    ap.add_argument("--ensemble", type=int, default=0, metavar="M",
                    help="--family mlp: a bagged set of M members (mean score)")
    ap.add_argument("--repeats", type=int, default=30,
                    help="--family mlp --device cuda: predict() timing repeats")
    args = ap.parse_args()

    from shifu_amd.models.wide_deep import WideDeep
    from shifu_amd.models.mlp import ShifuMLP
    from shifu_amd.train.export import export_ensemble, export_model
    from shifu_amd.serve import ShifuScorer

    mlp = args.family == "mlp"
    if args.fused and not mlp:
        ap.error("--fused needs --family mlp")
    if args.ensemble and not mlp:
        ap.error("--ensemble needs --family mlp")
    if args.ensemble < 0:
        ap.error("--ensemble must be >= 1")
    extra = {"members": args.ensemble} if args.ensemble else {}
    torch.manual_seed(11)
    if mlp:
        hidden = [int(h) for h in args.hidden.split(",") if h]
        model = ShifuMLP(args.n_dense, hidden, ["tanh"] * len(hidden), seed=11)
        model_desc = f"mlp[{args.n_dense}dense,hidden{hidden}]"
        if args.ensemble:
            members = [ShifuMLP(args.n_dense, hidden, ["tanh"] * len(hidden),
                                seed=11 + i) for i in range(args.ensemble)]
            model_desc = f"{args.ensemble}x{model_desc}"
    else:
        model = WideDeep(args.n_dense, [args.vocab] * args.n_cat, args.embed_dim,
                         [1024, 512, 256], ["relu"] * 3, seed=11)
        model_desc = (f"wide_deep[{args.n_cat}x{args.vocab}vocab"
                      f"*{args.embed_dim}d+{args.n_dense}dense,"
                      f"tower[1024, 512, 256]]")
    with tempfile.TemporaryDirectory() as td:
        if args.ensemble:
            export_ensemble(members, td)
        else:
            export_model(model, td)
        sc = ShifuScorer()
        sc.init(os.path.join(td, "GenericModelConfig.json"),
                device=args.device, fused=args.fused)

        rng = np.random.default_rng(3)
        dense = rng.standard_normal((args.rows, args.n_dense), dtype=np.float32)
        cats = None if mlp else rng.integers(0, args.vocab,
                                             (args.rows, args.n_cat),
                                             dtype=np.int64)

        def batch_of(s, e):
            return (dense[s:e],) if mlp else (dense[s:e], cats[s:e])

        # batched scoring
        n = 0
        # warmup
        sc.compute_batch(*batch_of(0, args.batch))
        if args.device == "cuda":
            torch.cuda.synchronize()
        t0 = time.time()
        for s in range(0, args.rows, args.batch):
            e = min(s + args.batch, args.rows)
            p = sc.compute_batch(*batch_of(s, e))
            n += len(p)
        if args.device == "cuda":
            torch.cuda.synchronize()
        dt = time.time() - t0
        print(json.dumps({
            "metric": "scoring_rows_per_sec", "value": n / dt, "unit": "rows/s",
            "mode": "compute_batch", "device": args.device,
            "batch": args.batch, "rows": n, "data": "synthetic",
            "fused": args.fused,
            "config": {"model": model_desc}, **extra}), flush=True)

        # per-row latency (Java Computable call pattern)
        k = 2000
        rows1 = [dense[i] if mlp else
                 np.concatenate([dense[i], cats[i].astype(np.float64)])
                 for i in range(k)]
        sc.compute(rows1[0])
        t0 = time.time()
        for i in range(k):
            sc.compute(rows1[i])
        dt = time.time() - t0
        print(json.dumps({
            "metric": "scoring_row_latency_us", "value": dt / k * 1e6,
            "unit": "us/row", "mode": "compute", "device": args.device,
            "rows": k, "higher_is_better": False,
            "fused": args.fused, **extra}), flush=True)

        if mlp and args.device == "cuda":
            _predict_device_time(sc, dense, args.batch, args.repeats,
                                 args.fused, model_desc, extra)


if __name__ == "__main__":
    main()
