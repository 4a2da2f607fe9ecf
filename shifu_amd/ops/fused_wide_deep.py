"""Fused single-kernel scoring for exported Wide&Deep bundles.

`wd_score_stream` (ops/hip/fused_wide_deep.hip) scores a batch in one launch:
it folds the categorical ids, gathers the embedding rows straight into the
tower's LDS input tile next to the dense features, computes the wide term,
runs the tower through the streamed-weight layer loop of `mlp_score_stream`
and adds the wide term to the head logit before the sigmoid.  The layer path
takes about ten launches for the same work.

Packed once at model load:
  * the tower in `pack_mlp`'s blob layout (ops/fused_mlp.py), K0 = nd + F * D;
  * a bf16 (RNE) copy of the deep arena [R, D] and an fp32 copy of the wide
    arena [R];
  * the fp32 wide-dense weights [nd] and bias;
  * the per-feature (offset, size) table, on the host for the launcher's
    bounds check and on the device for the kernel.

Rounding points (kernel and CPU emulation alike): the tower's are
`mlp_score_stream`'s with the gathered rows taken from the bf16 arena; the
wide term is fp32 throughout, from the dense values as given (fp32 rows
unrounded) and is added to the unrounded fp32 head logit.

This path has its own opt-in switch, `fused_wd` (load_exported,
ShifuScorer.init, score.py --fused-wd).  `fused=` keeps refusing Wide&Deep.
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Tuple

import torch

from shifu_amd.ops.dispatch import require_hip
from shifu_amd.ops.fused_mlp import (MAX_LAYERS, STREAM_LDS_LIMIT,
                                     STREAM_MAX_WIDTH, STREAM_ROW_TILES,
                                     _emulate_logit, _pack_layers, _shapes_of,
                                     _stream_lds_bytes)

MAX_ARENA_ROWS = 2 ** 31 - 1      # the kernel keeps folded row indices as int32


def _tower_of(model):
    """The tower and head under the names `_pack_layers` reads."""
    return SimpleNamespace(hidden=model.tower, shifu_output_0=model.shifu_output_0)


def _wd_lds_bytes(shapes, num_cat: int, row_tile: int) -> int:
    """LDS of one block at a `row_tile`-row tile: the streamed kernel's two
    activation buffers, row_tile fp32 wide terms and row_tile x F int32 row
    indices — the launcher re-derives it."""
    return _stream_lds_bytes(shapes, row_tile) + row_tile * 4 + row_tile * num_cat * 4


def wd_eligible(model) -> Tuple[bool, str]:
    """(True, "") when `model` can run through the fused Wide&Deep kernel, else
    (False, reason)."""
    from shifu_amd.models.wide_deep import WideDeep
    from shifu_amd.ops.embedding import MultiEmbedding
    if not isinstance(model, WideDeep):
        return False, (f"{type(model).__name__} is not a WideDeep (the fused "
                       f"Wide&Deep scoring kernel covers Wide&Deep bundles only)")
    if model.unified:
        return False, ("unified wide+deep arena (the kernel reads the split "
                       "layout exported bundles reload as)")
    for name in ("wide_cat", "embeddings"):
        if type(getattr(model, name)) is not MultiEmbedding:
            return False, (f"{name} is a {type(getattr(model, name)).__name__}, "
                           f"not a replicated MultiEmbedding")
    if model.num_dense < 1:
        return False, "no dense features (the kernel needs num_dense >= 1)"
    if not model.vocab_sizes:
        return False, "no categorical features"
    rows = model.embeddings.total_rows
    if rows > MAX_ARENA_ROWS:
        return False, f"{rows} arena rows > {MAX_ARENA_ROWS}"
    shapes = _shapes_of(_tower_of(model))
    if len(shapes) > MAX_LAYERS:
        return False, f"{len(shapes)} tower layers (head included) > {MAX_LAYERS}"
    if shapes[-1][0] != 1:
        return False, f"head width {shapes[-1][0]} != 1"
    widest = max([shapes[0][1]] + [n for n, _ in shapes])
    if widest > STREAM_MAX_WIDTH:
        return False, f"width {widest} > {STREAM_MAX_WIDTH}"
    lds = _wd_lds_bytes(shapes, len(model.vocab_sizes), STREAM_ROW_TILES[0])
    if lds > STREAM_LDS_LIMIT:
        return False, (f"a {STREAM_ROW_TILES[0]}-row tile needs {lds} B of LDS "
                       f"> {STREAM_LDS_LIMIT}")
    return True, ""


@dataclass
class PackedWideDeep:
    blob: torch.Tensor            # uint8 tower image, pack_mlp's layout
    table: torch.Tensor           # CPU int32 [L, 4]: byte offset, N, K, act id
    arena: torch.Tensor           # bf16 [R, D] deep arena
    wide_vec: torch.Tensor        # fp32 [R] wide arena
    wide_dense_w: torch.Tensor    # fp32 [nd]
    wide_bias: float
    feat_table: torch.Tensor      # CPU int64 [F, 2]: (offset, size) per feature
    feat_table_dev: torch.Tensor  # the same table on the model's device
    num_dense: int
    num_cat: int
    embed_dim: int
    lds_bytes: int                # one block's LDS at the smallest row tile


def pack_wide_deep(model) -> PackedWideDeep:
    ok, why = wd_eligible(model)
    if not ok:
        raise ValueError(f"model is not eligible for fused Wide&Deep scoring: {why}")
    tower = _tower_of(model)
    blob, table = _pack_layers(tower)
    emb = model.embeddings
    feat = torch.stack([emb.offsets.cpu(), emb.sizes.cpu()], dim=1).contiguous()
    return PackedWideDeep(
        blob=blob, table=table,
        arena=emb.arena.detach().float().to(torch.bfloat16).contiguous(),
        wide_vec=model.wide_cat.arena.detach().float().reshape(-1).contiguous(),
        wide_dense_w=model.wide_dense.weight.detach().float().reshape(-1).contiguous(),
        wide_bias=float(model.wide_dense.bias.detach().float().reshape(-1)[0]),
        feat_table=feat, feat_table_dev=feat.to(blob.device),
        num_dense=model.num_dense, num_cat=len(model.vocab_sizes),
        embed_dim=model.embed_dim,
        lds_bytes=_wd_lds_bytes(_shapes_of(tower), len(model.vocab_sizes),
                                STREAM_ROW_TILES[0]))


def _emulate_wd(packed: PackedWideDeep, dense: torch.Tensor,
                cats: torch.Tensor) -> torch.Tensor:
    """Pure-torch forward pass with exactly the kernel's rounding points."""
    d = dense.detach().cpu()
    if d.dtype != torch.bfloat16:
        d = d.float()
    offsets, sizes = packed.feat_table[:, 0], packed.feat_table[:, 1]
    rows = cats.detach().cpu().long().clamp(min=0) % sizes + offsets    # [B, F]
    emb = packed.arena.cpu()[rows.reshape(-1)].reshape(d.shape[0], -1)
    x = torch.cat([d.to(torch.bfloat16), emb], dim=1)
    wide = (d.float() @ packed.wide_dense_w.cpu() + packed.wide_vec.cpu()[rows].sum(dim=1)
            + torch.tensor(packed.wide_bias, dtype=torch.float32))
    return torch.sigmoid(_emulate_logit(packed, x) + wide).to(dense.device)


@torch.no_grad()
def wd_predict(packed: PackedWideDeep, dense: torch.Tensor, cats: torch.Tensor,
               max_blocks: int = 0, row_tile: int = 0) -> torch.Tensor:
    """Scores fp32 [B] for dense [B, num_dense] (fp32 or bf16 rows) and
    per-feature local ids cats [B, num_cat] (int64 or int32, any value: they
    are folded as MultiEmbedding.forward folds them).  row_tile 0 lets the
    launcher choose the block tile; 16, 32 or 64 forces it.  Scores do not
    depend on either launch argument."""
    if dense.dim() != 2 or dense.shape[1] != packed.num_dense:
        raise ValueError(f"expected dense [B, {packed.num_dense}], got "
                         f"{tuple(dense.shape)}")
    if cats.dim() != 2 or tuple(cats.shape) != (dense.shape[0], packed.num_cat):
        raise ValueError(f"expected cats [{dense.shape[0]}, {packed.num_cat}], "
                         f"got {tuple(cats.shape)}")
    if row_tile not in (0,) + STREAM_ROW_TILES:
        raise ValueError(f"row_tile must be 0 or one of {STREAM_ROW_TILES}, "
                         f"got {row_tile}")
    if not dense.is_cuda:
        return _emulate_wd(packed, dense, cats)
    ext = require_hip()
    if ext is None:            # explicit eager A/B opt-in only (dispatch.py)
        return _emulate_wd(packed, dense, cats)
    if packed.blob.device != dense.device or cats.device != dense.device:
        raise ValueError(f"packed weights are on {packed.blob.device}, the ids "
                         f"on {cats.device} but the rows are on {dense.device}")
    x = dense.detach()
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    ids = cats.detach()
    if ids.dtype not in (torch.int64, torch.int32):
        ids = ids.long()
    return ext.wd_score_stream(x.contiguous(), ids.contiguous(), packed.arena,
                               packed.wide_vec, packed.wide_dense_w,
                               packed.wide_bias, packed.feat_table,
                               packed.feat_table_dev, packed.blob, packed.table,
                               max_blocks, row_tile)


def attach_fused_wd(model) -> PackedWideDeep:
    """Pack `model` and route its predict(dense, cats) through `wd_predict`."""
    packed = pack_wide_deep(model)
    model.predict = lambda dense, cats: wd_predict(packed, dense, cats)
    model._fused_wd_packed = packed
    return packed
