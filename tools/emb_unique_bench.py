"""Unified embedding update chain, old (emb_update_unified: accsq + scatter,
all atomics) against new (emb_update_unified_spans: duplicate flags + fused
plain pass + atomic duplicate tail), on the same inputs at the bench's n.

Ids are drawn per feature as floor(V * u**alpha), u uniform: alpha = 1 is
the bench's uniform draw, larger alpha skews the draw towards low ids so
more entries sit on rows that are hit more than once.

    python tools/emb_unique_bench.py                       # alpha sweep
    python tools/emb_unique_bench.py --flags-only --vocab 8000000
    SHIFU_EMB_SPAN_LOG2=16 python tools/emb_unique_bench.py --alphas 1

Prints one JSON line per alpha: once-hit share of the entries, microseconds
per call of both ops (device events, alternating) and of emb_dup_flags
alone."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shifu_amd.ops.dispatch import hip_ops  # noqa: E402


def draw_ids(B, F, V, alpha, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = torch.rand(B, F, generator=g, dtype=torch.float64)
    local = (u.pow(alpha) * V).long().clamp_(max=V - 1)
    return local + torch.arange(F, dtype=torch.int64) * V


def time_us(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--n-cat", type=int, default=26)
    ap.add_argument("--vocab", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--dense", type=int, default=32)
    ap.add_argument("--alphas", type=float, nargs="+",
                    default=[1.0, 2.0, 3.0, 4.0, 6.0, 8.0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--flags-only", action="store_true",
                    help="time emb_dup_flags alone (no arena is allocated)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ext = hip_ops()
    B, F, V, D, nd = args.batch, args.n_cat, args.vocab, args.dim, args.dense
    DP, n, R = D + 4, B * F, F * V
    lo = torch.arange(F, dtype=torch.int64) * V
    spans = torch.stack([lo, lo + V], dim=1).contiguous()
    span = int(ext.emb_dup_span())
    wgs = F * ((V + span - 1) // span)
    if not args.flags_only:
        arena = (torch.rand(R, DP, device="cuda", dtype=torch.float32) * 0.2 - 0.1
                 ).to(torch.bfloat16)
        arena[:, D + 1:] = 0
        dgrad = (torch.randn(B, nd + F * D, device="cuda") * 1e-3).to(torch.bfloat16)
        wide = (torch.randn(B, F, device="cuda") * 1e-3).to(torch.bfloat16)
        acc = torch.empty(0, device="cuda")
    for alpha in args.alphas:
        ids = draw_ids(B, F, V, alpha, 1234)
        rows_cpu = ids.reshape(-1)
        cnt = torch.bincount(rows_cpu, minlength=R)
        once_share = float((cnt[rows_cpu] == 1).double().mean())
        del cnt
        rows = rows_cpu.cuda()
        out = {"alpha": alpha, "n": n, "once_hit_share": round(once_share, 4),
               "span": span, "flag_workgroups": wgs}

        def flags():
            ext.emb_dup_flags(rows, F, spans)

        def old():
            ext.emb_update_unified(arena, acc, rows, dgrad, nd, wide, 1, F,
                                   0.01, 1e-8, True, True)

        def new():
            ext.emb_update_unified_spans(arena, acc, rows, dgrad, nd, wide, 1, F,
                                         0.01, 1e-8, True, True, spans)

        fns = {"flags_us": flags}
        if not args.flags_only:
            fns.update({"old_us": old, "new_us": new})
        for fn in fns.values():
            time_us(fn, 3)                                  # warm up
        best = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                best[k].append(time_us(fn, args.iters))
        for k, v in best.items():
            out[k] = [round(x, 1) for x in v]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
