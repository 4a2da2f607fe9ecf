"""Device-side evaluation pass: weighted loss + score histograms, AUC and KS.

`EvalAccumulator` collects, over any number of batches, the statistic the
kernels of ops/hip/eval_hist.hip compute:

    p    = fp32 sigmoid of the fp32 logit
    bin  = min(NB - 1, int(p * NB)), NB a power of two; a NaN p goes to bin 0
    cls  = target >= 0.5                       (auc_score's rule)
    count[cls][bin] += 1,  wsum[cls][bin] += weight
    loss_sum += weight * (p - y)^2  or  weight * bce_with_logits
    nonzero  += weight != 0                    (SUM_BY_NONZERO_WEIGHTS)

and `result()` turns it into loss, AUC, KS and their weighted forms.  AUC is
the average-tie rank AUC of the bin-quantised scores,
sum_b neg_b * (pos_above_b + pos_b / 2) / (P * N); KS is the largest gap
between the two classes' cumulative shares over the bin edges.

On the GPU the state lives in one int64 tensor that every `add_*` call adds
to on the device; `result()` is the only device-to-host read.  Counts and
everything derived from them are bitwise reproducible.  The weight sums are
accumulated with fp32 LDS atomics inside a block, so their last bits depend
on the order in which lanes arrive and are NOT bitwise reproducible.

Dispatch follows ops/dispatch.py: CPU tensors run the float64 emulation, GPU
tensors run the HIP kernels, a GPU tensor without the extension is an error.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from shifu_amd.ops.dispatch import require_hip
from shifu_amd.ops.fused_mlp import (WAVES, PackedMLP, _blob_bytes, _ceil_to,
                                     _shapes_of, fused_eligible, unpack_mlp)
from shifu_amd.ops.linear import _act_fwd_ref

MIN_BINS, MAX_BINS = 32, 4096
EVAL_LDS_LIMIT = 160 * 1024   # all of a gfx950 CU's LDS
_EVAL_TAIL = 8 * WAVES        # per-wave loss / nonzero-count scratch
_OUT = 8                      # loss, auc, ks, wauc, wks, n, P, N
_FIELDS = ("loss", "auc", "ks", "wauc", "wks", "n", "pos", "neg")


def _check_bins(n_bins: int) -> int:
    n_bins = int(n_bins)
    if not (MIN_BINS <= n_bins <= MAX_BINS and n_bins & (n_bins - 1) == 0):
        raise ValueError(f"n_bins must be a power of two in [{MIN_BINS}, "
                         f"{MAX_BINS}], got {n_bins}")
    return n_bins


def _eval_lds_bytes(shapes, n_bins: int) -> int:
    """LDS of one mlp_eval_fused_kernel block for layers [(N, K), ...]: the
    blob, 8 x 2 activation buffers, 16 * NB bytes of histogram and the
    reduction scratch — the launcher derives the same map and checks it again."""
    max_kpad = max([32] + [_ceil_to(k, 32) for _, k in shapes[1:]])
    return (_blob_bytes(shapes) + 2 * WAVES * 32 * max_kpad + 16 * n_bins
            + _EVAL_TAIL)


def eval_eligible(model, n_bins: int) -> Tuple[bool, str]:
    """(True, "") when `model` can be evaluated by the fused forward + loss +
    histogram kernel with `n_bins` bins, else (False, reason)."""
    ok, why = fused_eligible(model)
    if not ok:
        return ok, why
    lds = _eval_lds_bytes(_shapes_of(model), _check_bins(n_bins))
    if lds > EVAL_LDS_LIMIT:
        return False, (f"packed weights + activation buffers + {n_bins}-bin "
                       f"histogram need {lds} B of LDS > {EVAL_LDS_LIMIT}")
    return True, ""


def _finish(counts: np.ndarray, wsum: np.ndarray, loss_sum: float,
            nonzero: int) -> dict:
    """The finish kernel in float64 numpy; counts, wsum are [2, NB]."""
    def auc_ks(h):
        neg, pos = h[0].astype(np.float64), h[1].astype(np.float64)
        P, N = pos.sum(), neg.sum()
        if not (P > 0 and N > 0):
            return 0.5, 0.0
        above = np.cumsum(pos[::-1])[::-1]              # pos in bins >= b
        area = float((neg * (above - 0.5 * pos)).sum())
        gap = np.abs(above / P - np.cumsum(neg[::-1])[::-1] / N)
        return area / (P * N), float(gap.max())

    auc, ks = auc_ks(counts)
    wauc, wks = auc_ks(wsum)
    pos, neg = int(counts[1].sum()), int(counts[0].sum())
    return {"loss": loss_sum / max(float(nonzero), 1e-12), "auc": auc, "ks": ks,
            "wauc": wauc, "wks": wks, "n": pos + neg, "pos": pos, "neg": neg}


def _emulate_logits(packed: PackedMLP, dense: torch.Tensor) -> torch.Tensor:
    """fp32 head logits with the fused kernels' rounding points (fused_mlp._emulate
    without the final sigmoid)."""
    x = dense.detach().float().cpu().to(torch.bfloat16).float()
    layers = unpack_mlp(packed)
    for w, b, act in layers[:-1]:
        x = _act_fwd_ref(x @ w.float().t() + b, act).to(torch.bfloat16).float()
    w, b, _ = layers[-1]
    return (x @ w.float().t() + b).reshape(-1)


class EvalAccumulator:
    def __init__(self, n_bins: int = 1024, device="cpu"):
        self.n_bins = _check_bins(n_bins)
        self.device = torch.device(device)
        # GPU state needs the extension (an error if absent, see dispatch.py)
        self._ext = require_hip() if self.device.type == "cuda" else None
        self.reset()

    def reset(self) -> None:
        nb = self.n_bins
        if self._ext is not None:
            # int64 words: 2NB counts | 2NB fp64 weight sums | fp64 loss sum |
            # nonzero count | the finish kernel's 8 fp64 results
            self._state = torch.zeros(4 * nb + 2 + _OUT, dtype=torch.int64,
                                      device=self.device)
        else:
            self._counts = np.zeros((2, nb), dtype=np.int64)
            self._wsum = np.zeros((2, nb), dtype=np.float64)
            self._loss_sum, self._nonzero = 0.0, 0

    # ------------------------------------------------------------------ CPU
    def _emulate(self, logits, target, weight, kind: int) -> None:
        z32 = logits.detach().float().cpu().reshape(-1)
        y = target.detach().double().cpu().numpy()
        w = weight.detach().float().cpu().double().numpy()
        nb = self.n_bins
        s = (torch.sigmoid(z32) * nb).numpy()           # fp32; x NB is exact
        bins = np.where(np.isnan(s), 0, np.minimum(nb - 1, np.nan_to_num(s))
                        ).astype(np.int64)
        slot = (y >= 0.5) * nb + bins
        self._counts += np.bincount(slot, minlength=2 * nb).reshape(2, nb)
        self._wsum += np.bincount(slot, weights=w, minlength=2 * nb).reshape(2, nb)
        z = z32.double()
        yt = torch.from_numpy(y)
        if kind == 0:
            per = (torch.sigmoid(z) - yt) ** 2
        else:
            per = torch.nn.functional.binary_cross_entropy_with_logits(
                z, yt, reduction="none")
        self._loss_sum += float((torch.from_numpy(w) * per).sum())
        self._nonzero += int((w != 0).sum())

    # --------------------------------------------------------------- public
    @torch.no_grad()
    def add_scores(self, logits: torch.Tensor, target: torch.Tensor,
                   weight: torch.Tensor, kind: int = 0, replicas: int = 0,
                   max_blocks: int = 0) -> None:
        """Add a batch of logits [B] (any model's).  replicas > 0 overrides the
        number of LDS copies of the histogram (measurements); max_blocks > 0
        caps the grid (tests)."""
        logits = logits.detach().reshape(-1)
        if self._ext is None:      # CPU state, or the explicit eager A/B opt-in
            return self._emulate(logits, target, weight, kind)
        if logits.dtype not in (torch.float32, torch.bfloat16):
            logits = logits.float()
        self._ext.eval_hist_scores(
            logits.contiguous(), target.detach().float().contiguous(),
            weight.detach().float().contiguous(), self._state, self.n_bins, kind,
            replicas, max_blocks)

    @torch.no_grad()
    def add_mlp(self, packed: PackedMLP, dense: torch.Tensor,
                target: torch.Tensor, weight: torch.Tensor, kind: int = 0,
                max_blocks: int = 0) -> None:
        """Add a batch of rows [B, num_features] scored by the packed MLP:
        forward, loss and histogram in one kernel, no logits in memory."""
        if dense.dim() != 2 or dense.shape[1] != packed.num_features:
            raise ValueError(f"expected dense [B, {packed.num_features}], got "
                             f"{tuple(dense.shape)}")
        if self._ext is None:
            return self._emulate(_emulate_logits(packed, dense), target, weight, kind)
        if packed.blob.device != dense.device:
            raise ValueError(f"packed weights are on {packed.blob.device} but the "
                             f"rows are on {dense.device}")
        x = dense.detach()
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        self._ext.eval_hist_mlp(
            x.contiguous(), target.detach().float().contiguous(),
            weight.detach().float().contiguous(), packed.blob, packed.table,
            self._state, self.n_bins, kind, max_blocks)

    def result(self) -> dict:
        """loss, auc, ks, wauc, wks, n, pos, neg, nonzero, loss_sum and the raw
        [2, NB] histograms `counts` (int64) and `wsum` (float64); row 0 is the
        negative class.  One device-to-host read on the GPU."""
        nb = self.n_bins
        if self._ext is None:
            out = _finish(self._counts, self._wsum, self._loss_sum, self._nonzero)
            out.update(nonzero=self._nonzero, loss_sum=self._loss_sum,
                       counts=self._counts.copy(), wsum=self._wsum.copy())
            return out
        self._ext.eval_hist_finish(self._state, nb)
        host = self._state.cpu().numpy()
        f64 = host.view(np.float64)
        out = dict(zip(_FIELDS, f64[4 * nb + 2:].tolist()))
        for k in ("n", "pos", "neg"):
            out[k] = int(out[k])
        out.update(nonzero=int(host[4 * nb + 1]), loss_sum=float(f64[4 * nb]),
                   counts=host[:2 * nb].reshape(2, nb).copy(),
                   wsum=f64[2 * nb:4 * nb].reshape(2, nb).copy())
        return out
