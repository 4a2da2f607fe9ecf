"""The training engine: per-rank epoch loop.

Successor of the reference's worker hot loop (reference: ssgd_monitor.py
main():147-345 — build graph, MonitoredTrainingSession, per-epoch batch loop
feeding np.array_split slices, valid pass, metric line, chief-side
checkpoint + export), redesigned MI355X-first:

* the whole rank shard lives on the GPU (288 GB HBM3E holds every BASELINE
  config short of the 100M-row one); batches are views, no host staging in
  the hot loop;
* forward/backward run bf16 through the fused HIP ops; gradient aggregation
  is the GradAggregator's bucketed RCCL all-reduce overlapped with backward;
* optimizer is one fused kernel over the flat arena;
* per-epoch: train pass -> weighted valid loss (+AUC) -> metric emission ->
  rank-0 checkpoint; final rank-0 export in the eval-compatible layout.
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np
import torch

from shifu_amd.config.model_config import ModelConfig
from shifu_amd.config.run_config import RunConfig
from shifu_amd.data.csv_loader import TabularDataset
from shifu_amd.ops.flat import FlatParams, split_params
from shifu_amd.ops.loss import weighted_loss
from shifu_amd.ops.optim import FusedOptimizer
from shifu_amd.parallel.dist import GradAggregator, is_distributed
from shifu_amd.train import checkpoint as ckpt
from shifu_amd.train.export import export_model
from shifu_amd.train.metrics import TrainingIntermediateResult


def auc_score(scores: np.ndarray, labels: np.ndarray) -> float:
    """Rank-based AUC (no sklearn dependency in the hot path)."""
    order = np.argsort(scores, kind="mergesort")
    ranks = np.empty_like(order, dtype=np.float64)
    ranks[order] = np.arange(1, len(scores) + 1)
    # average ties
    s_sorted = scores[order]
    i = 0
    while i < len(s_sorted):
        j = i
        while j + 1 < len(s_sorted) and s_sorted[j + 1] == s_sorted[i]:
            j += 1
        if j > i:
            ranks[order[i:j + 1]] = (i + 1 + j + 1) / 2.0
        i = j + 1
    pos = labels >= 0.5
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    if n_pos == 0 or n_neg == 0:
        return 0.5
    return float((ranks[pos].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def _arena_offset_rows(p: torch.nn.Parameter, model: torch.nn.Module) -> torch.Tensor:
    """LOCAL rows of an embedding arena hit by all-zero ids (graph-capture
    warmup seeds): the owning module knows its own layout."""
    for mod in model.modules():
        if getattr(mod, "arena", None) is p:
            if hasattr(mod, "capture_touch_rows"):
                return mod.capture_touch_rows().to(p.device)
            return mod.offsets.to(p.device)
    return torch.zeros(1, dtype=torch.int64, device=p.device)


@dataclass
class DeviceData:
    dense: torch.Tensor   # [N, Fn] (bf16 on GPU, f32 on CPU)
    cats: torch.Tensor    # [N, Fc] int64 (may be empty second dim)
    target: torch.Tensor  # [N] f32
    weight: torch.Tensor  # [N] f32

    @classmethod
    def from_dataset(cls, ds: TabularDataset, device: torch.device,
                     dense_dtype: torch.dtype) -> "DeviceData":
        return cls(
            dense=torch.from_numpy(ds.dense).to(device=device, dtype=dense_dtype),
            cats=torch.from_numpy(ds.cats).to(device=device),
            target=torch.from_numpy(ds.target).to(device=device),
            weight=torch.from_numpy(ds.weight).to(device=device),
        )

    def __len__(self):
        return self.target.shape[0]

    def slice(self, idx: torch.Tensor) -> "DeviceData":
        return DeviceData(self.dense[idx], self.cats[idx],
                          self.target[idx], self.weight[idx])


class StreamingData:
    """Out-of-core residency (ROADMAP item 5): the shard stays in host RAM
    (pinned when the target is a GPU) and only the current batch crosses PCIe.
    Use when the per-rank shard exceeds what you want resident in the 288 GB
    HBM (RunConfig.data_residency="stream").  Same interface as DeviceData;
    `slice(idx)` takes HOST indices and returns a device-resident batch
    (async H2D from pinned memory)."""

    index_device = "cpu"     # epoch permutations index host-side

    def __init__(self, ds: TabularDataset, device: torch.device,
                 dense_dtype: torch.dtype):
        self.device = device
        pin = device.type == "cuda"

        def host(t: torch.Tensor) -> torch.Tensor:
            return t.pin_memory() if pin and t.numel() else t

        self.dense = host(torch.from_numpy(ds.dense).to(dense_dtype))
        self.cats = host(torch.from_numpy(ds.cats))
        self.target = host(torch.from_numpy(ds.target))
        self.weight = host(torch.from_numpy(ds.weight))

    @classmethod
    def from_dataset(cls, ds: TabularDataset, device: torch.device,
                     dense_dtype: torch.dtype) -> "StreamingData":
        return cls(ds, device, dense_dtype)

    def __len__(self):
        return self.target.shape[0]

    def slice(self, idx) -> DeviceData:
        dev = self.device
        nb = dev.type == "cuda"
        return DeviceData(self.dense[idx].to(dev, non_blocking=nb),
                          self.cats[idx].to(dev, non_blocking=nb),
                          self.target[idx].to(dev, non_blocking=nb),
                          self.weight[idx].to(dev, non_blocking=nb))


class StreamPrefetcher:
    """Double-buffered H2D prefetch for StreamingData (ROADMAP item 5 /
    VERDICT item 6): batch i+1's pinned-host gather + async copy run on a
    side stream while the compute stream works on batch i, hiding the PCIe
    transfer under compute."""

    def __init__(self, data):
        self.data = data
        self.stream = torch.cuda.Stream()
        self.pending = None

    def start(self, idx) -> None:
        with torch.cuda.stream(self.stream):
            b = self.data.slice(idx)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.pending = (b, ev)

    def get(self) -> "DeviceData":
        b, ev = self.pending
        self.pending = None
        cur = torch.cuda.current_stream()
        cur.wait_event(ev)
        for t in (b.dense, b.cats, b.target, b.weight):
            if t.is_cuda:
                t.record_stream(cur)   # allocator: tensor born on the side stream
        return b


class Trainer:
    def __init__(self, model: torch.nn.Module, mc: ModelConfig, rc: RunConfig,
                 train_data: TabularDataset, valid_data: TabularDataset,
                 rank: int = 0, world_size: int = 1,
                 device: Optional[torch.device] = None,
                 metric_sink: Optional[Callable[[TrainingIntermediateResult], None]] = None,
                 heartbeat: Optional[Callable[[], None]] = None):
        self.mc, self.rc = mc, rc
        self.rank, self.world = rank, world_size
        self.device = device or torch.device(rc.resolved_device())
        self.is_chief = (rank == 0)  # chief semantics (TensorflowSession.java:443-450)
        self.metric_sink = metric_sink
        # liveness: successor of the executor heartbeat loop
        # (TensorflowApplicationMaster.java:63-112); called at least every
        # heartbeat_interval_s from inside the epoch step loop
        self.heartbeat = heartbeat
        self._hb_interval = float(rc.heartbeat_interval_s)
        self._hb_last = time.time()
        self._ckpt_secs = float(getattr(rc, "checkpoint_every_secs", 0.0))
        self._ckpt_last = time.time()
        self._has_sharded = False  # set after model construction below

        self.model = model.to(self.device)
        dense_dtype = torch.bfloat16 if (self.device.type == "cuda"
                                         and rc.dtype == "bf16") else torch.float32
        if dense_dtype == torch.bfloat16:
            # embedding arenas live bf16 in HBM (the HIP gather path);
            # dense params stay fp32 masters (FusedLinear casts per step)
            for p in self.model.parameters():
                if getattr(p, "_is_embedding_arena", False):
                    p.data = p.data.to(torch.bfloat16)
        self.dense_dtype = dense_dtype
        residency = getattr(rc, "data_residency", "auto")
        container = (StreamingData if residency == "stream" else DeviceData)

        def wrap(ds):
            # prebuilt containers (a 100M-row stream built chunk-wise without
            # an fp32 numpy intermediate — tools/config5_stream.py) pass
            # through untouched
            if hasattr(ds, "slice") and not isinstance(ds, TabularDataset):
                return ds
            return container.from_dataset(ds, self.device, dense_dtype)

        self.train_data = wrap(train_data)
        self.valid_data = wrap(valid_data)

        self._has_sharded = any(getattr(p, "_is_ep_sharded", False)
                                for p in self.model.parameters())
        if self._ckpt_secs > 0 and self._has_sharded:
            # time-based triggers are rank-local clocks; EP shards saved at
            # different steps would be mutually inconsistent.  Epoch-cadence
            # saves (rank-synchronized) still run.
            if self.is_chief:
                print("shifu_amd: checkpoint_every_secs is disabled for "
                      "EP-sharded embeddings (epoch-cadence saves only)",
                      flush=True)
            self._ckpt_secs = 0.0

        dense_params, emb_params = split_params(self.model)
        from shifu_amd.ops.flat import bind_mirrors
        self.flat = FlatParams(dense_params,
                               mirror_bf16=(dense_dtype == torch.bfloat16))
        bind_mirrors(self.model, self.flat)
        self.emb_params = emb_params
        self.aggregator = GradAggregator(self.flat, emb_params,
                                         bucket_mb=rc.bucket_mb,
                                         overlap=rc.overlap_allreduce,
                                         quorum_ratio=rc.quorum_ratio)
        p = mc.params
        self.optimizer = FusedOptimizer(
            self.flat, emb_params, optimizer=p.optimizer, lr=p.learning_rate,
            l2_reg=p.l2_reg, emb_lr=p.learning_rate)
        self.loss_kind = p.loss
        self.batch_size = int(rc.batch_size or p.batch_size)
        self.update_window = max(int(p.update_window), 1)
        if world_size == 1 and self.update_window == 1:
            # unified arenas: hand unpacked grads straight to the optimizer
            # (no [n, D+2] packing); needs single-rank, no window accumulation
            from shifu_amd.ops.embedding import UnifiedMultiEmbedding
            for m in self.model.modules():
                if isinstance(m, UnifiedMultiEmbedding):
                    m.defer_grads = True
        self.epochs = int(rc.epochs or mc.num_train_epochs)
        self.global_step = 0
        self.start_epoch = 0
        self._rng = np.random.default_rng(rc.seed + rank)
        # Uniform stepping at world>1: every rank takes the SAME number of
        # steps per epoch with FULL-SIZE batches, padding tails with
        # weight-0 rows.  Shards differ by up to one row, so without this
        # (a) ranks could take different step counts (mismatched collectives
        # = deadlock) and (b) tail batch sizes could differ across ranks,
        # which the static-split table-EP all-to-all cannot tolerate.
        # Weight-0 rows are exact no-ops: the loss normalizes by the
        # nonzero-weight count and their gradients are identically zero.
        self._uniform_steps = None
        if world_size > 1 and is_distributed():
            if len(self.train_data) == 0:
                # an empty TRAIN shard cannot pad batches (no row to repeat);
                # it means the sharding itself is wrong — fail loudly
                raise ValueError(
                    f"rank {rank}: empty train shard at world={world_size} — "
                    "check data sharding (fewer rows than ranks?)")
            import math as _math
            t = torch.tensor([_math.ceil(len(self.train_data) / self.batch_size)],
                             device=self.device if self.device.type == "cuda"
                             else "cpu")
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            self._uniform_steps = int(t)
        from shifu_amd.utils.trace import StepTracer
        self.tracer = StepTracer(enabled=rc.enable_trace,
                                 use_gpu_events=(self.device.type == "cuda"))
        # hipGraph-captured steps (full-size batches only; tail batches and
        # window mode run eager; capture failure falls back silently)
        g = getattr(rc, "graphs", "auto")
        self.use_graphs = ((g == "on" or (g == "auto" and
                                          self.device.type == "cuda" and
                                          world_size == 1 and
                                          self.update_window == 1 and
                                          not rc.enable_trace))
                           and not isinstance(self.train_data, StreamingData))
        self._graph = None
        self._gb: Optional[DeviceData] = None
        # one-kernel forward+loss+backward for LDS-resident MLPs
        self._fused_step = bool(getattr(rc, "fused_mlp_step", False))
        if self._fused_step:
            from shifu_amd.ops.fused_mlp import fused_grad_eligible
            ok, why = fused_grad_eligible(self.model)
            if ok and world_size != 1:
                ok, why = False, f"world size {world_size} != 1"
            if not ok:
                raise ValueError(f"fused_mlp_step is set but the model cannot "
                                 f"use the fused training step: {why}")

        # loss + score histograms accumulated on the device (ops/eval_hist.py)
        self._device_eval = bool(getattr(rc, "device_eval", False))
        if self._device_eval:
            from shifu_amd.ops.eval_hist import _check_bins
            self._eval_bins = _check_bins(getattr(rc, "device_eval_bins", 1024))
            if world_size != 1:
                raise ValueError(
                    f"device_eval is set but world size {world_size} != 1: the "
                    f"per-rank evaluation states are not all-reduced yet")

    # ------------------------------------------------------------------ steps
    def train_step(self, batch: DeviceData, sync: bool = True) -> torch.Tensor:
        """One forward/backward/(all-reduce)/update step; returns the loss as
        a device scalar (call .item() only at epoch granularity — a per-step
        host readback would stall the pipeline)."""
        tr = self.tracer
        self.aggregator.set_sync(sync)
        if self._fused_step:
            with tr.phase("fwd"):
                loss = self.model.fused_loss(batch.dense, batch.target,
                                             batch.weight, self.loss_kind)
        else:
            with tr.phase("fwd"):
                logits = self.model(batch.dense, batch.cats)
            with tr.phase("loss"):
                loss = weighted_loss(logits, batch.target, batch.weight, self.loss_kind)
        with tr.phase("bwd"):
            loss.backward()
        if sync:
            with tr.phase("comm"):
                self.aggregator.finish()
            with tr.phase("opt"):
                self.optimizer.step()
                self.optimizer.zero_grad()
        self.global_step += 1
        return loss.detach()  # device scalar: no per-step host sync

    # ------------------------------------------------------------- graph mode
    def _ensure_graph(self) -> bool:
        if self._graph is not None:
            return True
        B = self.batch_size
        self._gb = DeviceData(
            dense=torch.empty(B, self.train_data.dense.shape[1],
                              device=self.device, dtype=self.train_data.dense.dtype),
            cats=torch.empty(B, self.train_data.cats.shape[1],
                             device=self.device, dtype=torch.int64),
            target=torch.empty(B, device=self.device),
            weight=torch.empty(B, device=self.device),
        )
        gb = self._gb

        def body():
            if self._fused_step:
                loss = self.model.fused_loss(gb.dense, gb.target, gb.weight,
                                             self.loss_kind)
            else:
                logits = self.model(gb.dense, gb.cats)
                loss = weighted_loss(logits, gb.target, gb.weight, self.loss_kind)
            loss.backward()
            self.aggregator.finish()
            self.optimizer.step()
            self.optimizer.zero_grad()
            return loss

        from shifu_amd.train.graph import GraphedStep
        try:
            # Warmup + capture run REAL steps; training semantics require the
            # model to be unchanged afterwards.  Seed with all-zero ids so
            # each arena touches only its F offset rows, snapshot the dense
            # state + those rows, and restore after capture.
            gb.dense.normal_()
            gb.cats.zero_()
            gb.target.fill_(0.5)
            gb.weight.fill_(1.0)
            snap = {
                "flat": self.flat.flat.clone(),
                "m": None if self.optimizer.m is None else self.optimizer.m.clone(),
                "v": None if self.optimizer.v is None else self.optimizer.v.clone(),
                "step_count": self.optimizer.step_count,
                "emb": [], "emb_state": [],
            }
            for i, p in enumerate(self.emb_params):
                rows = _arena_offset_rows(p, self.model)
                snap["emb"].append((rows, p.data[rows].clone()))
                acc = self.optimizer.emb_state.get(i)
                snap["emb_state"].append(None if acc is None else acc[rows].clone())

            stepper = GraphedStep(body, warmup=3)
            stepper.capture()

            # restore pre-capture training state
            self.flat.flat.copy_(snap["flat"])
            if snap["m"] is not None:
                self.optimizer.m.copy_(snap["m"])
            if snap["v"] is not None:
                self.optimizer.v.copy_(snap["v"])
            self.optimizer.step_count = snap["step_count"]
            if hasattr(self.optimizer, "_step_buf"):
                self.optimizer._step_buf.fill_(float(snap["step_count"]))
            for i, p in enumerate(self.emb_params):
                rows, vals = snap["emb"][i]
                p.data[rows] = vals
                if snap["emb_state"][i] is not None:
                    self.optimizer.emb_state[i][rows] = snap["emb_state"][i]
            self.flat.refresh_mirror()
            self._graph = stepper
            return True
        except Exception:
            self.use_graphs = False
            return False

    def _graphed_step(self, idx: torch.Tensor, k_valid: int) -> torch.Tensor:
        gb = self._gb
        torch.index_select(self.train_data.dense, 0, idx, out=gb.dense)
        torch.index_select(self.train_data.cats, 0, idx, out=gb.cats)
        torch.index_select(self.train_data.target, 0, idx, out=gb.target)
        torch.index_select(self.train_data.weight, 0, idx, out=gb.weight)
        if k_valid < idx.shape[0]:          # outside the captured graph
            gb.weight[k_valid:] = 0.0
        loss = self._graph.run()
        self.global_step += 1
        return loss.detach().clone()

    @torch.no_grad()
    def evaluate(self, data: DeviceData, batch_size: int = 65536) -> dict:
        """Weighted loss + AUC over a dataset (the reference's per-epoch valid
        pass, ssgd_monitor.py:281-284).

        At world>1 the forward may contain EP collectives, so every rank runs
        the SAME number of batches with the SAME batch size — ranks with
        fewer local rows pad with weight-0 repeats of row 0 (no-ops in the
        metrics)."""
        if self._device_eval:
            return self._evaluate_device(data, batch_size)
        self.model.eval()
        n = len(data)
        steps = (n + batch_size - 1) // batch_size
        eb = batch_size
        if self._uniform_steps is not None:
            t = torch.tensor([n], device=self.device
                             if self.device.type == "cuda" else "cpu")
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            gmax = int(t)
            eb = max(min(batch_size, gmax), 1)
            steps = max((gmax + eb - 1) // eb, 1)
        if steps == 0 or (n == 0 and self._uniform_steps is None):
            self.model.train()
            return {"loss": 0.0, "auc": 0.5, "n": 0}
        idx_dev = ("cpu" if getattr(data, "index_device", "device") == "cpu"
                   else self.device)
        total, wtot = 0.0, 0.0
        scores = []
        for si in range(steps):
            s = si * eb
            k = max(min(s + eb, n) - s, 0)
            if n == 0:
                # empty local shard but peers still run collectives: join
                # with an all-padding batch
                b = DeviceData(
                    dense=torch.zeros(eb, self.train_data.dense.shape[1],
                                      device=self.device, dtype=self.dense_dtype),
                    cats=torch.zeros(eb, self.train_data.cats.shape[1],
                                     device=self.device, dtype=torch.int64),
                    target=torch.zeros(eb, device=self.device),
                    weight=torch.zeros(eb, device=self.device))
            else:
                idx = torch.arange(s, s + k, device=idx_dev)
                if self._uniform_steps is not None and k < eb:
                    idx = torch.cat([idx, idx.new_zeros(eb - k)])
                b = data.slice(idx)
            logits = self.model(b.dense, b.cats).float().reshape(-1)
            p = torch.sigmoid(logits)[:k]
            w = b.weight.float()[:k]
            y = b.target.float()[:k]
            if self.loss_kind in ("sigmoid_ce", "ce", "bce"):
                per = w * torch.nn.functional.binary_cross_entropy_with_logits(
                    logits[:k], y, reduction="none")
            else:
                per = w * (p - y) ** 2
            total += float(per.sum())
            wtot += float((w != 0).sum())  # SUM_BY_NONZERO_WEIGHTS (ops/loss.py)
            scores.append(p.cpu().numpy())
        self.model.train()
        scores = np.concatenate(scores)
        labels = data.target.cpu().numpy()[:len(scores)]
        return {"loss": total / max(wtot, 1e-12),
                "auc": auc_score(scores, labels), "n": n}

    @torch.no_grad()
    def _evaluate_device(self, data: DeviceData, batch_size: int) -> dict:
        """evaluate() with RunConfig.device_eval: the same batches, but loss and
        score histograms accumulate on the device and the host reads one small
        tensor at the end.  `auc` is the AUC of the bin-quantised scores; the
        dict also carries ks, wauc, wks and the raw histograms."""
        from shifu_amd.ops.eval_hist import EvalAccumulator, eval_eligible
        from shifu_amd.ops.fused_mlp import pack_mlp
        n = len(data)
        acc = EvalAccumulator(self._eval_bins, self.device)
        kind = 1 if self.loss_kind in ("sigmoid_ce", "ce", "bce") else 0
        self.model.eval()
        # an eligible MLP is packed once from the live parameters and runs
        # forward + loss + histogram as one kernel per batch
        packed = (pack_mlp(self.model)
                  if eval_eligible(self.model, self._eval_bins)[0] else None)
        idx_dev = ("cpu" if getattr(data, "index_device", "device") == "cpu"
                   else self.device)
        for s in range(0, n, batch_size):
            b = data.slice(torch.arange(s, min(s + batch_size, n), device=idx_dev))
            if packed is not None:
                acc.add_mlp(packed, b.dense, b.target, b.weight, kind)
            else:
                acc.add_scores(self.model(b.dense, b.cats), b.target, b.weight, kind)
        self.model.train()
        return acc.result()

    # ------------------------------------------------------------------ epochs
    def run_epoch(self, epoch: int) -> TrainingIntermediateResult:
        t0 = time.time()
        n = len(self.train_data)
        # snapshot the RNG state and step count BEFORE drawing this epoch's
        # permutation: a mid-epoch checkpoint (tagged epoch-1) must let the
        # resumed run redraw the SAME permutation and recount from the
        # epoch-start step
        rng_pre = self._rng.bit_generator.state
        step_pre = self.global_step
        B = self.batch_size
        n_steps = self._uniform_steps or max((n + B - 1) // B, 1)
        # block shuffle (beyond-HBM streams, tools/config5_stream.py): permute
        # BATCH-SIZED blocks and read each contiguously — a random row gather
        # over a 40 GB pinned host block is CPU-cache-miss bound (measured
        # 1.9M rows/s vs >20M with contiguous slices), and a 100M-row
        # permutation array alone is 800 MB
        block_mode = bool(getattr(self.train_data, "block_shuffle", False))
        if block_mode:
            bperm = self._rng.permutation(max((n + B - 1) // B, 1))
        else:
            perm = torch.from_numpy(self._rng.permutation(n))
            if getattr(self.train_data, "index_device", "device") != "cpu":
                perm = perm.to(self.device)
        losses = []

        def make_idx(si):
            if block_mode:
                s = int(bperm[si % len(bperm)]) * B
                idx = torch.arange(s, min(s + B, n))
            else:
                s = si * B
                idx = perm[s:min(s + B, n)]
            k = idx.shape[0]             # valid rows; the rest are padding
            if self._uniform_steps and k < B:
                idx = torch.cat([idx, idx.new_zeros(B - k)])
            return idx, k

        prefetch = None
        if (isinstance(self.train_data, StreamingData)
                and self.device.type == "cuda" and not self.use_graphs):
            prefetch = StreamPrefetcher(self.train_data)
            prefetch.start(make_idx(0)[0])

        for si in range(n_steps):
            idx, k = make_idx(si)
            sync = ((si + 1) % self.update_window == 0) or (si == n_steps - 1)
            if (self.use_graphs and sync and idx.shape[0] == self.batch_size
                    and self._ensure_graph()):
                losses.append(self._graphed_step(idx, k))
            else:
                if prefetch is not None:
                    batch = prefetch.get()
                    if si + 1 < n_steps:
                        prefetch.start(make_idx(si + 1)[0])
                else:
                    batch = self.train_data.slice(idx)
                if k < idx.shape[0]:
                    batch.weight = batch.weight.clone()
                    batch.weight[k:] = 0.0   # padding rows are exact no-ops
                # window mode: only every update_window-th (or last) step
                # syncs+updates
                losses.append(self.train_step(batch, sync=sync))
            if self.heartbeat and time.time() - self._hb_last >= self._hb_interval:
                self.heartbeat()
                self._hb_last = time.time()
            if (self._ckpt_secs > 0
                    and time.time() - self._ckpt_last >= self._ckpt_secs):
                # mid-epoch time-based save, tagged as the last COMPLETE epoch
                # (epoch-1 == -1 resumes epoch 0 correctly) with the pre-epoch
                # RNG/step snapshot so resume replays this epoch from its start
                self._save_checkpoint(epoch - 1, global_step=step_pre,
                                      np_rng=rng_pre)
                self._ckpt_last = time.time()
            ces = int(getattr(self.rc, "checkpoint_every_steps", 0))
            if ces > 0 and sync and (si + 1) % ces == 0 and si + 1 < n_steps:
                # step-cadence save: si is identical on every rank (uniform
                # stepping), so EP shards stay mutually consistent; the stamp
                # lets resume DETECT a crash that interleaved two save points
                self._save_checkpoint(epoch - 1, global_step=step_pre,
                                      np_rng=rng_pre, stamp=self.global_step)
                if is_distributed():
                    torch.distributed.barrier()
        mean_loss = float(torch.stack(losses).float().mean()) if losses else 0.0
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        train_time = time.time() - t0

        t1 = time.time()
        val = self.evaluate(self.valid_data)
        valid_time = time.time() - t1

        return TrainingIntermediateResult(
            worker_index=self.rank,
            current_epoch=epoch,
            current_epoch_time=train_time,
            current_epoch_valid_time=valid_time,
            training_error=mean_loss,
            valid_error=val["loss"],
            container_id=f"rank-{self.rank}",
        )

    def _save_checkpoint(self, epoch: int, global_step: Optional[int] = None,
                         np_rng=None, stamp: Optional[int] = None) -> None:
        """EP-aware save: every rank writes its shard, rank 0 the main file
        (train/checkpoint.py layout).  `stamp` disambiguates repeated saves
        under the same epoch tag (step-cadence mid-epoch saves)."""
        gs = self.global_step if global_step is None else global_step
        rng = self._rng.bit_generator.state if np_rng is None else np_rng
        if stamp is None:
            # (step, launcher attempt): equal across ranks of ONE save, and
            # different across a crash+restart retraining the same epoch —
            # load_checkpoint then detects mixed shard generations
            stamp = (self.global_step << 8) | (
                int(os.environ.get("SHIFU_RUN_ATTEMPT", "0")) & 0xFF)
        ckpt.save_checkpoint(self.rc.tmp_model_path, epoch, gs,
                             self.model, self.optimizer,
                             extra={"np_rng": rng},
                             rank=self.rank, world=self.world, stamp=stamp)

    def maybe_resume(self) -> None:
        path = ckpt.latest_checkpoint(self.rc.tmp_model_path, world=self.world)
        if path:
            info = ckpt.load_checkpoint(path, self.model, self.optimizer,
                                        self.device, rank=self.rank,
                                        world=self.world)
            self.flat.refresh_mirror()
            self.start_epoch = int(info["epoch"]) + 1
            self.global_step = int(info["global_step"])
            np_rng = (info.get("extra") or {}).get("np_rng")
            if np_rng is not None and self.rank == 0:
                self._rng.bit_generator.state = np_rng
            else:
                # Non-chief ranks (the checkpoint stores only rank 0's stream)
                # and old checkpoints: fast-forward by the permutations already
                # consumed, so the resumed run draws the same epoch orderings
                # an uninterrupted run would have.
                for _ in range(self.start_epoch):
                    self._rng.permutation(len(self.train_data))

    def fit(self) -> List[TrainingIntermediateResult]:
        self.maybe_resume()
        results = []
        for epoch in range(self.start_epoch, self.epochs):
            r = self.run_epoch(epoch)
            results.append(r)
            if self.metric_sink:
                self.metric_sink(r)
            if (epoch + 1) % self.rc.checkpoint_every_epochs == 0:
                # all ranks: EP shards are per-rank; non-chief without shards
                # is a no-op inside save_checkpoint
                self._save_checkpoint(epoch)
            if is_distributed():
                torch.distributed.barrier()
        if self.tracer.enabled:
            self.tracer.export_chrome_trace(
                os.path.join(self.rc.log_dir, f"trace-rank{self.rank}.json"))
            if self.is_chief:
                print(self.tracer.summary_line(), flush=True)
        swapped = self._consolidate_sharded_for_export()  # collective when EP
        if self.is_chief:
            try:
                export_model(self.model, self.rc.final_model_path,
                             model_name=self.mc.model_name, algorithm=self.mc.algorithm,
                             selected_columns=(self.rc.selected_numeric_columns +
                                               self.rc.selected_categorical_columns))
            finally:
                for name, orig in swapped.items():
                    parent = self.model
                    parts = name.split(".")
                    for part in parts[:-1]:
                        parent = getattr(parent, part)
                    setattr(parent, parts[-1], orig)
        return results

    def _consolidate_sharded_for_export(self) -> dict:
        """EP models: all-gather each sharded arena (row%world or by-feature
        — the module's merge_shards knows its own topology) and temporarily
        swap a full replicated MultiEmbedding into the chief's model so the
        export is self-contained.  A collective — EVERY rank must call this;
        returns {module_name: original} on the chief (for restore), {}
        elsewhere."""
        sharded = [(n, m) for n, m in self.model.named_modules()
                   if hasattr(m, "merge_shards")
                   and getattr(getattr(m, "arena", None), "_is_ep_sharded", False)]
        if not sharded:
            return {}
        import torch.distributed as dist
        from shifu_amd.ops.embedding import MultiEmbedding
        swapped = {}
        for name, mod in sharded:
            shard = mod.arena.data
            world = mod.world
            counts = [mod.shard_rows(r) for r in range(world)]
            pad = shard.new_zeros(max(counts), mod.dim)
            pad[:shard.shape[0]] = shard
            outs = [torch.empty_like(pad) for _ in range(world)]
            dist.all_gather(outs, pad)
            if not self.is_chief:
                continue
            full = mod.merge_shards([o[:c] for o, c in zip(outs, counts)])
            rep = MultiEmbedding(mod.vocab_sizes, mod.dim, empty_init=True,
                                 dtype=shard.dtype).to(shard.device)
            rep.arena.data = full
            if hasattr(mod.arena, "_unified_split"):
                # unified EP arena: the export splits it wide/deep
                rep.arena._unified_split = mod.arena._unified_split
            parent = self.model
            parts = name.split(".")
            for part in parts[:-1]:
                parent = getattr(parent, part)
            swapped[name] = getattr(parent, parts[-1])
            setattr(parent, parts[-1], rep)
        return swapped
