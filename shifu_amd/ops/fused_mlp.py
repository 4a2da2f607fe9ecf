"""Fused whole-network scoring for exported ShifuMLP models.

The serving-side counterpart of the per-layer training kernels: the complete
weight set of a typical Shifu MLP (TrainParams default [50, 50] tanh, ~25 KB)
is packed ONCE at model load into a single device blob, and
`mlp_score_fused` (ops/hip/fused_mlp.hip) keeps it resident in LDS while rows
stream through MFMA — one launch, fp32 rows in, fp32 scores out.

Packed blob, per layer (head included), back to back:
  * bf16 W zero-padded to [Npad = ceil16(N), Kpad = ceil32(K)], stored in the
    16x16x32 MFMA fragment order (`_to_fragment_order`), so the in-LDS operand
    read is a contiguous, bank-conflict-free 16 bytes per lane;
  * fp32 bias zero-padded to Npad.
The layer table is a CPU int32 [L, 4]: byte offset, N, K, activation id.

Rounding points (kernel and CPU emulation alike): bf16 input, bf16 weights,
fp32 accumulate + fp32 bias + fp32 activation, bf16 between layers, fp32 head
logit, sigmoid.

Dispatch follows ops/dispatch.py: CPU tensors run the pure-torch emulation,
GPU tensors run the HIP kernel, and a GPU tensor without the extension is a
loud error — never a silent fallback.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import torch

from shifu_amd.ops.dispatch import require_hip
from shifu_amd.ops.linear import _act_fwd_ref

MAX_LAYERS = 8
LDS_LIMIT = 128 * 1024        # same ceiling the v4 GEMM uses (V4_LDS_BYTES)
WAVES = 8                     # waves per block sharing one weight copy
MAX_INPUT = 1024              # layer-0 fragments live in registers (32 k-steps)


def _ceil_to(v: int, a: int) -> int:
    return (v + a - 1) // a * a


def _to_fragment_order(wp: torch.Tensor) -> torch.Tensor:
    """[Npad, Kpad] -> flat fragment order: for n-tile nt and k-step ks the 64
    lanes' 8-element fragments are contiguous, lane = (k%32//8)*16 + n%16."""
    npad, kpad = wp.shape
    return (wp.reshape(npad // 16, 16, kpad // 32, 4, 8)
              .permute(0, 2, 3, 1, 4).contiguous().reshape(-1))


def _from_fragment_order(flat: torch.Tensor, npad: int, kpad: int) -> torch.Tensor:
    return (flat.reshape(npad // 16, kpad // 32, 4, 16, 8)
                .permute(0, 3, 1, 2, 4).contiguous().reshape(npad, kpad))


def _layers_of(model) -> list:
    return list(model.hidden) + [model.shifu_output_0]


def _lds_bytes(shapes: List[Tuple[int, int]]) -> int:
    """LDS the kernel needs for layers [(N, K), ...]: the blob plus two
    ping-pong bf16 activation buffers (16 rows x widest hidden Kpad) per wave."""
    blob = sum(_ceil_to(n, 16) * _ceil_to(k, 32) * 2 + _ceil_to(n, 16) * 4
               for n, k in shapes)
    max_kpad = max([32] + [_ceil_to(k, 32) for _, k in shapes[1:]])
    return blob + 2 * WAVES * 32 * max_kpad


def fused_eligible(model) -> Tuple[bool, str]:
    """(True, "") when `model` can run through the fused kernel, else
    (False, reason)."""
    from shifu_amd.models.mlp import ShifuMLP
    if not isinstance(model, ShifuMLP):
        return False, (f"{type(model).__name__} is not a ShifuMLP (the fused "
                       f"scoring kernel covers dense MLP bundles only)")
    layers = _layers_of(model)
    if len(layers) > MAX_LAYERS:
        return False, (f"{len(layers)} layers (head included) > {MAX_LAYERS}")
    if layers[-1].out_features != 1:
        return False, f"head width {layers[-1].out_features} != 1"
    lds = _lds_bytes([(l.out_features, l.in_features) for l in layers])
    if lds > LDS_LIMIT:
        return False, (f"packed weights + activation buffers need {lds} B of "
                       f"LDS > {LDS_LIMIT}")
    if layers[0].in_features > MAX_INPUT:
        return False, f"input width {layers[0].in_features} > {MAX_INPUT}"
    return True, ""


@dataclass
class PackedMLP:
    blob: torch.Tensor        # uint8 [blob_bytes], on the model's device
    table: torch.Tensor       # CPU int32 [L, 4]: byte offset, N, K, act id
    lds_bytes: int
    num_features: int


def pack_mlp(model) -> PackedMLP:
    ok, why = fused_eligible(model)
    if not ok:
        raise ValueError(f"model is not eligible for fused scoring: {why}")
    layers = _layers_of(model)
    parts, rows, off = [], [], 0
    for l in layers:
        n, k = l.out_features, l.in_features
        npad, kpad = _ceil_to(n, 16), _ceil_to(k, 32)
        wp = torch.zeros(npad, kpad, dtype=torch.bfloat16)
        wp[:n, :k] = l.weight.detach().float().cpu().to(torch.bfloat16)
        bp = torch.zeros(npad, dtype=torch.float32)
        bp[:n] = l.bias.detach().float().cpu()
        parts.append(_to_fragment_order(wp).view(torch.uint8))
        parts.append(bp.view(torch.uint8))
        rows.append([off, n, k, l._act])
        off += npad * kpad * 2 + npad * 4
    blob = torch.cat(parts).contiguous()
    device = layers[0].weight.device
    return PackedMLP(blob=blob.to(device),
                     table=torch.tensor(rows, dtype=torch.int32),
                     lds_bytes=_lds_bytes([(r[1], r[2]) for r in rows]),
                     num_features=layers[0].in_features)


def unpack_mlp(packed: PackedMLP, padded: bool = False):
    """[(W bf16 [N, K], bias fp32 [N], act id), ...] recovered from the blob;
    padded=True returns the full zero-padded [Npad, Kpad] / [Npad] arrays."""
    blob = packed.blob.cpu()
    out = []
    for off, n, k, act in packed.table.tolist():
        npad, kpad = _ceil_to(n, 16), _ceil_to(k, 32)
        wb = npad * kpad * 2
        w = _from_fragment_order(blob[off:off + wb].view(torch.bfloat16), npad, kpad)
        b = blob[off + wb:off + wb + npad * 4].view(torch.float32).clone()
        out.append((w, b, act) if padded else (w[:n, :k].clone(), b[:n], act))
    return out


def _emulate(packed: PackedMLP, dense: torch.Tensor) -> torch.Tensor:
    """Pure-torch forward pass with exactly the kernel's rounding points."""
    layers = unpack_mlp(packed)
    x = dense.detach().float().cpu().to(torch.bfloat16).float()
    for i, (w, b, act) in enumerate(layers):
        z = x @ w.float().t() + b
        if i == len(layers) - 1:
            return torch.sigmoid(z.reshape(-1)).to(dense.device)
        x = _act_fwd_ref(z, act).to(torch.bfloat16).float()
    raise AssertionError("unreachable")


@torch.no_grad()
def fused_predict(packed: PackedMLP, dense: torch.Tensor,
                  max_blocks: int = 0, waves: int = WAVES) -> torch.Tensor:
    """Scores fp32 [B] for dense [B, num_features]."""
    if dense.dim() != 2 or dense.shape[1] != packed.num_features:
        raise ValueError(f"expected dense [B, {packed.num_features}], got "
                         f"{tuple(dense.shape)}")
    if not dense.is_cuda:
        return _emulate(packed, dense)
    ext = require_hip()
    if ext is None:            # explicit eager A/B opt-in only (dispatch.py)
        return _emulate(packed, dense)
    if packed.blob.device != dense.device:
        raise ValueError(f"packed weights are on {packed.blob.device} but the "
                         f"rows are on {dense.device}")
    x = dense.detach().float().contiguous()
    return ext.mlp_score_fused(x, packed.blob, packed.table, max_blocks, waves)


def attach_fused(model) -> PackedMLP:
    """Pack `model` and route its predict() through the fused path."""
    packed = pack_mlp(model)
    model._fused_packed = packed
    model.predict = lambda dense, cats=None: fused_predict(packed, dense)
    return packed


# ---------------------------------------------------------------------------
# Bagged ensembles (Shifu train.baggingNum -> model0 .. modelN-1, mean score).
#
# `mlp_score_fused_ensemble` keeps the packed images of a whole GROUP of
# member networks in LDS, loads each 16-row tile's layer-0 fragments once and
# runs every member on them: M members cost one read of the rows and one
# launch.  Members that do not fit one block's LDS together are split
# greedily, in member order, into consecutive groups (one launch each); the
# running fp32 sum is carried from launch to launch in the output buffer and
# scaled once at the end, so the result does not depend on the grouping.

MAX_ENSEMBLE = 64             # members over all groups
MAX_GROUP_MEMBERS = 8         # members resident in LDS per launch
MAX_GROUP_LAYERS = 32         # layers (heads included) per launch
MAX_ENSEMBLE_INPUT = 512      # layer-0 fragments stay live across all members


def _shapes_of(model) -> List[Tuple[int, int]]:
    return [(l.out_features, l.in_features) for l in _layers_of(model)]


def _blob_bytes(shapes: List[Tuple[int, int]]) -> int:
    return sum(_ceil_to(n, 16) * _ceil_to(k, 32) * 2 + _ceil_to(n, 16) * 4
               for n, k in shapes)


def _group_lds_bytes(group_shapes: List[List[Tuple[int, int]]],
                     max_kpad: int) -> int:
    """`_lds_bytes` arithmetic for a group: the members' blobs back to back
    plus the 8 waves' ping-pong buffers at the ensemble-wide hidden Kpad."""
    return sum(_blob_bytes(s) for s in group_shapes) + 2 * WAVES * 32 * max_kpad


def _ensemble_max_kpad(all_shapes: List[List[Tuple[int, int]]]) -> int:
    return max([32] + [_ceil_to(k, 32) for s in all_shapes for _, k in s[1:]])


def ensemble_eligible(models) -> Tuple[bool, str]:
    """(True, "") when `models` can run as one fused ensemble, else
    (False, reason)."""
    models = list(models)
    if not 1 <= len(models) <= MAX_ENSEMBLE:
        return False, (f"{len(models)} members, the fused ensemble kernel "
                       f"takes 1..{MAX_ENSEMBLE}")
    for i, m in enumerate(models):
        ok, why = fused_eligible(m)
        if not ok:
            return False, f"member {i}: {why}"
    widths = [_layers_of(m)[0].in_features for m in models]
    if len(set(widths)) != 1:
        return False, (f"members disagree on the input width: {widths} (one "
                       f"set of layer-0 fragments feeds every member)")
    if widths[0] > MAX_ENSEMBLE_INPUT:
        return False, (f"input width {widths[0]} > {MAX_ENSEMBLE_INPUT} (the "
                       f"layer-0 fragments stay in registers across all members)")
    shapes = [_shapes_of(m) for m in models]
    max_kpad = _ensemble_max_kpad(shapes)
    for i, s in enumerate(shapes):
        lds = _group_lds_bytes([s], max_kpad)
        if lds > LDS_LIMIT:
            return False, (f"member {i}: packed weights + the ensemble's "
                           f"activation buffers need {lds} B of LDS > {LDS_LIMIT}")
    return True, ""


@dataclass
class PackedEnsemble:
    blobs: List[torch.Tensor]   # per group: uint8, the members' images back to back
    tables: List[torch.Tensor]  # per group: CPU int32 [Lg, 5]: member index in
                                # the group, byte offset, N, K, act id
    group_sizes: List[int]      # members per group, in member order
    group_lds_bytes: List[int]  # LDS of each group's 8-wave block
    num_features: int
    num_members: int


def pack_ensemble(models, max_group_bytes: int = LDS_LIMIT) -> PackedEnsemble:
    """Pack `models` (member order = summation order) into LDS-sized groups.
    max_group_bytes lowers the per-group LDS budget (tests force more groups)."""
    models = list(models)
    ok, why = ensemble_eligible(models)
    if not ok:
        raise ValueError(f"models are not eligible for fused ensemble scoring: {why}")
    budget = min(int(max_group_bytes), LDS_LIMIT)
    shapes = [_shapes_of(m) for m in models]
    max_kpad = _ensemble_max_kpad(shapes)

    groups: List[List[int]] = [[]]
    for i, s in enumerate(shapes):
        if _group_lds_bytes([s], max_kpad) > budget:
            raise ValueError(f"member {i} alone needs "
                             f"{_group_lds_bytes([s], max_kpad)} B of LDS > "
                             f"max_group_bytes={budget}")
        cur = groups[-1]
        trial = [shapes[j] for j in cur] + [s]
        if cur and (len(trial) > MAX_GROUP_MEMBERS
                    or sum(len(t) for t in trial) > MAX_GROUP_LAYERS
                    or _group_lds_bytes(trial, max_kpad) > budget):
            groups.append([i])
        else:
            cur.append(i)

    device = _layers_of(models[0])[0].weight.device
    blobs, tables, lds = [], [], []
    for g in groups:
        parts, rows, off = [], [], 0
        for mi, i in enumerate(g):
            pm = pack_mlp(models[i])
            parts.append(pm.blob.cpu())
            for o, n, k, act in pm.table.tolist():
                rows.append([mi, off + o, n, k, act])
            off += pm.blob.numel()
        blobs.append(torch.cat(parts).contiguous().to(device))
        tables.append(torch.tensor(rows, dtype=torch.int32))
        lds.append(_group_lds_bytes([shapes[i] for i in g], max_kpad))
    return PackedEnsemble(blobs=blobs, tables=tables,
                          group_sizes=[len(g) for g in groups],
                          group_lds_bytes=lds,
                          num_features=_layers_of(models[0])[0].in_features,
                          num_members=len(models))


def ensemble_members(packed: PackedEnsemble) -> List[PackedMLP]:
    """Each member as a stand-alone PackedMLP cut out of its group's blob
    (CPU), in member order — the per-model layout `pack_mlp` builds."""
    out = []
    for blob, table in zip(packed.blobs, packed.tables):
        blob = blob.cpu()
        rows = table.tolist()
        for mi in range(rows[-1][0] + 1):
            mine = [r[1:] for r in rows if r[0] == mi]
            base = mine[0][0]
            end = base + _blob_bytes([(n, k) for _, n, k, _ in mine])
            out.append(PackedMLP(
                blob=blob[base:end].clone(),
                table=torch.tensor([[o - base, n, k, a] for o, n, k, a in mine],
                                   dtype=torch.int32),
                lds_bytes=_lds_bytes([(n, k) for _, n, k, _ in mine]),
                num_features=packed.num_features))
    return out


def _emulate_ensemble(packed: PackedEnsemble, dense: torch.Tensor):
    """(mean [B], members [B, M]) with the kernel's arithmetic: per-member
    `_emulate`, fp32 left-to-right sum in member order, times float32(1/M)."""
    cols = [_emulate(pm, dense).float() for pm in ensemble_members(packed)]
    total = torch.zeros_like(cols[0])
    for c in cols:
        total = total + c
    scale = torch.tensor(1.0 / packed.num_members, dtype=torch.float32)
    return total * scale.to(total.device), torch.stack(cols, dim=1)


@torch.no_grad()
def fused_ensemble_predict(packed: PackedEnsemble, dense: torch.Tensor,
                           return_members: bool = False, max_blocks: int = 0,
                           waves: int = WAVES):
    """Mean score fp32 [B] over the members for dense [B, num_features]; with
    return_members=True, (mean [B], per-member scores [B, M])."""
    if dense.dim() != 2 or dense.shape[1] != packed.num_features:
        raise ValueError(f"expected dense [B, {packed.num_features}], got "
                         f"{tuple(dense.shape)}")
    ext = require_hip() if dense.is_cuda else None
    if ext is None:            # CPU rows, or the explicit eager A/B opt-in
        mean, members = _emulate_ensemble(packed, dense)
        return (mean, members) if return_members else mean
    if any(b.device != dense.device for b in packed.blobs):
        raise ValueError(f"packed weights are on {packed.blobs[0].device} but "
                         f"the rows are on {dense.device}")
    x = dense.detach().float().contiguous()
    res = ext.mlp_score_fused_ensemble(x, packed.blobs, packed.tables,
                                       return_members, max_blocks, waves)
    return (res[0], res[1]) if return_members else res[0]


def attach_fused_ensemble(model) -> PackedEnsemble:
    """Pack an EnsembleModel's members and route its predict() and
    predict_members() through the fused ensemble path."""
    packed = pack_ensemble(list(model.members))
    model._fused_packed = packed
    model.predict = lambda dense, cats=None: fused_ensemble_predict(packed, dense)
    model.predict_members = lambda dense, cats=None: fused_ensemble_predict(
        packed, dense, return_members=True)[1]
    return packed
