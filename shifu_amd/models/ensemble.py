"""Bagged model set: the mean score of N member models.

Shifu's `train.baggingNum` produces `model0 .. modelN-1`, and the eval side
scores each row through all of them and reports the mean.  `EnsembleModel` is
that combination over any member family (the layer path, CPU or GPU); MLP
ensembles can additionally be routed through the single-kernel path
(ops/fused_mlp.py::attach_fused_ensemble).

The mean is defined the same way on every path: the fp32 left-to-right sum of
the members' scores, in member order, times float32(1/M).
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch


def _layout(model) -> tuple:
    num_dense = getattr(model, "num_dense", None)
    if num_dense is None:
        num_dense = model.num_features
    return int(num_dense), list(getattr(model, "vocab_sizes", []) or [])


class EnsembleModel(torch.nn.Module):
    def __init__(self, members: Sequence[torch.nn.Module]):
        super().__init__()
        members = list(members)
        if not members:
            raise ValueError("an ensemble needs at least one member")
        self.num_dense, self.vocab_sizes = _layout(members[0])
        for i, m in enumerate(members[1:], 1):
            nd, vs = _layout(m)
            if nd != self.num_dense or vs != self.vocab_sizes:
                raise ValueError(
                    f"member {i} expects {nd} dense + vocab sizes {vs}, member 0 "
                    f"{self.num_dense} dense + vocab sizes {self.vocab_sizes}")
        self.members = torch.nn.ModuleList(members)

    def _member_scores(self, dense, cats):
        if self.vocab_sizes:
            return [m.predict(dense, cats).float().reshape(-1) for m in self.members]
        return [m.predict(dense).float().reshape(-1) for m in self.members]

    @torch.no_grad()
    def predict_members(self, dense: torch.Tensor,
                        cats: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per-member scores fp32 [B, M]."""
        return torch.stack(self._member_scores(dense, cats), dim=1)

    @torch.no_grad()
    def predict(self, dense: torch.Tensor,
                cats: Optional[torch.Tensor] = None) -> torch.Tensor:
        cols = self._member_scores(dense, cats)
        total = torch.zeros_like(cols[0])
        for c in cols:
            total = total + c
        scale = torch.tensor(1.0 / len(cols), dtype=torch.float32,
                             device=total.device)
        return total * scale
