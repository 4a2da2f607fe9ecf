#!/usr/bin/env python3
"""Flagship benchmark: Wide&Deep tabular training throughput (samples/sec,
whole node) — BASELINE.json headline config 3: 1M-vocab categorical
embeddings (26 features) + 200 dense numerics, bf16 compute on MI355X.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1
the driver launches via torch.distributed.run with one rank per GPU (RCCL).
W untimed warmup steps, then exactly K timed steps bracketed by
barrier+synchronize on both sides; elapsed is the MAX over ranks; rank 0
prints ONE JSON line.  Each timed step is a FULL training step: embedding
gather + fused GEMM tower forward, fused loss, backward GEMMs, bucketed
all-reduce (dense) + EP all-to-all or sparse allgather (embeddings), fused
optimizer update.
At world>1 the embeddings default to table-sharded EP (static all-to-all
routing); --emb-mode dp selects replicated arenas + sparse allgather.
Synthetic data (no network), random-init weights, weak scaling (per-GPU
batch fixed).

A plain run does only the above.  --dump-outputs DIR additionally writes,
after the timed loop, what the last timed step computed (see dump_outputs).
--full is the switch for every measurement beyond the headline figure; the
headline is all this script measures today, so it currently adds nothing.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from shifu_amd.config.model_config import ModelConfig
from shifu_amd.config.run_config import RunConfig
from shifu_amd.models.wide_deep import WideDeep
from shifu_amd.ops.flat import FlatParams, split_params
from shifu_amd.ops.loss import weighted_loss
from shifu_amd.ops.optim import FusedOptimizer
from shifu_amd.parallel.dist import (GradAggregator, destroy_distributed,
                                     init_distributed, is_distributed)

# headline model config (BASELINE.json config 3)
N_DENSE = 200
N_CAT = 26
VOCAB = 1_000_000
EMBED_DIM = 64
TOWER = [1024, 512, 256]
ACTS = ["relu", "relu", "relu"]
PER_GPU_BATCH = 32768
N_BATCHES = 8  # distinct resident batches cycled through the loop


def make_batches(device, batch, rank, dtype, vocab=VOCAB, n_cat=N_CAT):
    gen = torch.Generator(device="cpu").manual_seed(1234 + rank)
    batches = []
    for i in range(N_BATCHES):
        dense = torch.randn(batch, N_DENSE, generator=gen).to(device=device, dtype=dtype)
        cats = torch.randint(0, vocab, (batch, n_cat), generator=gen).to(device)
        target = (torch.rand(batch, generator=gen) > 0.5).float().to(device)
        weight = torch.ones(batch, device=device)
        batches.append((dense, cats, target, weight))
    return batches


DUMP_SAMPLES = 256      # samples of the last batch whose arena rows are dumped
DUMP_DENSE = 65536      # dense parameters dumped


def dump_outputs(out_dir, loss, logits, flat, model, cats):
    """Write what the last timed step computed as float32 <out_dir>/*.npy
    (~2.5 MB at the headline config):

      loss            [1]      what step() returns: the batch loss
      logits          [B]      the model's forward output for the last batch
      dense_index     [K]      positions of a fixed seeded sample of the flat
                               dense parameters (float64 ids)
      dense_params    [K]      their values after the update
      emb<k>_rows     [S*F]    arena rows looked up by a fixed seeded sample
                               of S samples of the last batch (float64 ids)
      emb<k>_weights  [S*F,.]  those rows after the update (unified arena:
                               the D deep columns + the wide column)
      emb<k>_adagrad  [S*F]    unified arena only: the rows' decoded in-row
                               rowwise-adagrad accumulators

    EP-sharded arenas (world>1) dump a seeded sample of local rows instead.

    Inputs and initial weights are seeded, and the CPU path repeats bit for
    bit.  On the GPU the update kernels accumulate with atomics (embedding
    scatter, bias grads): ONE step repeats to rounding, but bf16
    re-quantisation and Adam's normalisation grow that noise step by step,
    fastest while the resident batches are being memorised, so compare two
    builds against the spread between two runs of one build.  Measured
    spread between identical runs on one MI355X, max |a-b| (value range):

                       --steps 20 --warmup 5      --steps 50 --warmup 10
      loss             4.4e-5  (0.0192)           1.8e-6  (1.3e-5)
      logits           0.19    (-14..17)          2.1     (-31..34)
      dense_params     4.5e-3  (-0.15..0.10)      5.9e-3  (-0.15..0.11)
      emb0_weights     7.8e-3  (-1.25..1.25)      7.8e-3  (-1.3..1.24)
      emb0_adagrad     7.3e-12 (0..2.8e-10)       1.9e-11 (0..3.6e-10)

    (three runs each, largest pairwise difference; the mean differences are
    10-100x smaller: logits 0.017 / 0.12, dense_params 2.6e-4 / 3.3e-4.)
    The spread keeps growing with the step count, and the loss falls towards
    zero as the 8 resident batches are memorised (1e-5 after 60 steps, 1e-6
    after ~200), so its RELATIVE spread grows too (0.2% at 25 steps, 14% at
    60): compare the loss absolutely, and prefer few steps for comparing."""
    os.makedirs(out_dir, exist_ok=True)

    def save(name, t, dtype=np.float32):
        a = t.detach().to("cpu", torch.float64).numpy().astype(dtype)
        np.save(os.path.join(out_dir, name + ".npy"), a)

    save("loss", loss.reshape(1))
    save("logits", logits.reshape(-1))
    gen = torch.Generator(device="cpu").manual_seed(4321)
    n = flat.flat.numel()
    didx = torch.randperm(n, generator=gen)[:DUMP_DENSE].sort().values
    save("dense_index", didx, np.float64)
    save("dense_params", flat.flat[didx.to(flat.flat.device)])
    pick = torch.randperm(cats.shape[0], generator=gen)[:DUMP_SAMPLES]
    k = 0
    for _, m in sorted(model.named_modules(), key=lambda kv: kv[0]):
        arena = getattr(m, "arena", None)
        if not getattr(arena, "_is_embedding_arena", False):
            continue
        offsets = getattr(m, "offsets", None)
        sizes = getattr(m, "sizes", None)
        if (offsets is not None and sizes is not None
                and offsets.numel() == cats.shape[1]
                and int(sizes.sum()) == arena.shape[0]):
            ids = cats[pick.to(cats.device)]
            rows = (ids.clamp(min=0) % sizes + offsets).reshape(-1)
        else:
            nr = min(arena.shape[0], DUMP_SAMPLES * cats.shape[1])
            rows = torch.randperm(arena.shape[0], generator=gen)[:nr].to(arena.device)
        vals = arena.data[rows]
        save(f"emb{k}_rows", rows, np.float64)
        if getattr(arena, "_acc_in_arena", False):
            D = arena._unified_split
            save(f"emb{k}_weights", vals[:, :D + 1])
            if vals.dtype == torch.bfloat16:
                acc = vals[:, D + 2:D + 4].contiguous().view(torch.float32)
            else:
                acc = vals[:, D + 2]
            save(f"emb{k}_adagrad", acc.reshape(-1))
        else:
            save(f"emb{k}_weights", vals)
        k += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=PER_GPU_BATCH)
    ap.add_argument("--bucket-mb", type=int, default=128)
    ap.add_argument("--embed-dim", type=int, default=EMBED_DIM)
    ap.add_argument("--vocab", type=int, default=VOCAB,
                    help="per-feature vocab (reduce for CPU smoke only)")
    ap.add_argument("--n-cat", type=int, default=N_CAT)
    ap.add_argument("--graphs", choices=["auto", "on", "off"], default="auto",
                    help="hipGraph-capture the whole training step")
    ap.add_argument("--arena", choices=["unified", "split"], default="unified",
                    help="wide+deep weights in ONE [R,D+2] arena (one gather/"
                         "scatter/EP-exchange) or two separate arenas")
    ap.add_argument("--emb-mode", choices=["auto", "dp", "ep", "ep_row"],
                    default="auto",
                    help="embedding parallelism: replicated+sparse-allgather "
                         "(dp), feature-sharded static all-to-all (ep, the "
                         "default at world>1), or row%%world sharding "
                         "(ep_row)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed "
                         "step computed as DIR/<name>.npy (rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beyond the headline "
                         "figure (none today: the plain run is the whole "
                         "benchmark)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    rank, world, device = init_distributed()
    if args.gpus != 1 and args.gpus != world:
        # never over-claim GPUs: a single process with --gpus 8 would report
        # 8x inflated samples/s.  The driver launches N>1 via torchrun, so
        # world (the rank count actually doing work) is the only truth.
        print(f"bench.py: --gpus {args.gpus} but world_size is {world}; "
              f"launch N>1 via torch.distributed.run (one rank per GPU)",
              file=sys.stderr, flush=True)
        sys.exit(2)
    n_gpus = world
    on_gpu = device.type == "cuda"
    dtype = torch.bfloat16 if on_gpu else torch.float32

    torch.manual_seed(777)
    mode = args.emb_mode
    if mode == "auto":
        mode = "ep" if world > 1 else "dp"
    sharded = {"ep": "table", "ep_row": "row", "dp": False}[mode]
    use_ep = bool(sharded)
    model = WideDeep(N_DENSE, [args.vocab] * args.n_cat, args.embed_dim, TOWER, ACTS,
                     seed=777, sharded_embeddings=sharded, world=world,
                     rank=rank, emb_fast_init=True,
                     unified=(args.arena == "unified")).to(device)
    if on_gpu:
        # keep embedding arenas bf16 (HBM-resident, gathered by the HIP kernel)
        for p in model.parameters():
            if getattr(p, "_is_embedding_arena", False):
                p.data = p.data.to(torch.bfloat16)
    if world == 1:
        from shifu_amd.ops.embedding import UnifiedMultiEmbedding
        for m in model.modules():
            if isinstance(m, UnifiedMultiEmbedding):
                m.defer_grads = True   # unpacked-grad fast path

    dense_params, emb_params = split_params(model)
    from shifu_amd.ops.flat import bind_mirrors
    flat = FlatParams(dense_params, mirror_bf16=on_gpu)
    bind_mirrors(model, flat)
    agg = GradAggregator(flat, emb_params, bucket_mb=args.bucket_mb, overlap=True)
    opt = FusedOptimizer(flat, emb_params, optimizer="adam", lr=1e-3,
                         l2_reg=0.0, emb_optimizer="adagrad", emb_lr=0.01)

    batches = make_batches(device, args.batch, rank, dtype, args.vocab, args.n_cat)

    use_graphs = (args.graphs == "on" or
                  (args.graphs == "auto" and on_gpu and world == 1))
    last = {}  # logits of the most recent step (a static buffer under graphs)

    if use_graphs:
        # static input buffers; per step we copy the rotating batch in and
        # replay ONE hipGraph covering fwd+loss+bwd+optimizer
        from shifu_amd.train.graph import GraphedStep
        sdense, scats, starget, sweight = [t.clone() for t in batches[0]]

        def graph_body():
            logits = model(sdense, scats)
            last["logits"] = logits.detach()
            loss = weighted_loss(logits, starget, sweight, "sigmoid_ce")
            loss.backward()
            agg.finish()
            opt.step()
            opt.zero_grad()
            return loss

        stepper = GraphedStep(graph_body, warmup=3)
        try:
            stepper.capture()
        except Exception as e:  # robust on fresh boxes: fall back to eager
            print(f"# hipGraph capture failed ({e}); falling back to eager",
                  flush=True)
            use_graphs = False

        def step(i):
            dense, cats, target, weight = batches[i % N_BATCHES]
            sdense.copy_(dense)
            scats.copy_(cats)
            starget.copy_(target)
            sweight.copy_(weight)
            return stepper.run()
    if not use_graphs:
        def step(i):
            dense, cats, target, weight = batches[i % N_BATCHES]
            logits = model(dense, cats)
            last["logits"] = logits.detach()
            loss = weighted_loss(logits, target, weight, "sigmoid_ce")
            loss.backward()
            agg.finish()
            opt.step()
            opt.zero_grad()
            return loss

    for i in range(args.warmup):
        step(i)

    if is_distributed():
        torch.distributed.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.time()
    for i in range(args.steps):
        loss = step(args.warmup + i)
    if on_gpu:
        torch.cuda.synchronize()
    if is_distributed():
        torch.distributed.barrier()
    elapsed = time.time() - t0

    # max elapsed over ranks (+ min, for the straggler spread)
    elapsed_min = elapsed
    if is_distributed():
        t = torch.tensor([elapsed], device=device if on_gpu else "cpu")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        tmin = torch.tensor([elapsed], device=device if on_gpu else "cpu")
        torch.distributed.all_reduce(tmin, op=torch.distributed.ReduceOp.MIN)
        elapsed, elapsed_min = float(t), float(tmin)

    if rank == 0:
        samples = n_gpus * args.batch * args.steps
        out = {
            "metric": "samples_per_sec_wide_deep",
            "value": samples / elapsed,
            "unit": "samples/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "rank_spread_ms": (elapsed - elapsed_min) * 1000.0,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # reference publishes no numbers
            "dtype": "bf16" if on_gpu else "fp32",
            "data": "synthetic",
            "config": {
                "model": f"wide_deep[{args.n_cat}x{args.vocab}vocab*{args.embed_dim}d+{N_DENSE}dense,tower{TOWER}]",
                "global_batch": n_gpus * args.batch,
                "per_gpu_batch": args.batch,
                "seq_len": None,
                "parallelism": (f"dp{n_gpus}+ep{n_gpus}(emb:{sharded})"
                                if use_ep else f"dp{n_gpus}"),
                "optimizer": "adam+rowwise_adagrad(emb)",
                "loss": "sigmoid_ce",
                "hipgraphs": use_graphs,
                "arena": args.arena,
            },
        }
        if args.dump_outputs:
            last_cats = batches[(args.warmup + args.steps - 1) % N_BATCHES][1]
            dump_outputs(args.dump_outputs, loss, last["logits"], flat, model,
                         last_cats)
        print(json.dumps(out), flush=True)
    destroy_distributed()


if __name__ == "__main__":
    main()
