"""Inputs, references and checks shared by tests/test_eval_hist_{cpu,gpu}.py.

Score cases are built so that a row's bin cannot depend on the device's exp:
draw a bin and an offset u in [0.25, 0.75], set p = (bin + u) / NB and
logit = log(p / (1 - p)) in float64, then cast.  For bf16 logits the bin is
recomputed in float64 from the rounded logit and rows within 0.05 bin of an
edge are dropped (bf16 rounding moves a score by <= 0.04 bin at NB = 64, so
none are in practice; the 10 % cap is asserted).  Weights are half-integers,
so fp32 sums of them are exact in any order.
"""
import functools

import numpy as np
import torch

from shifu_amd.train.trainer import auc_score
from test_fused_mlp_gpu import TOL, _build, _ref64

WEIGHTS = np.array([0.0, 0.5, 1.0, 1.5, 2.0], dtype=np.float32)
NETS = {"h50x2": ([50, 50], ["tanh", "tanh"]),
        "h33_17": ([33, 17], ["sigmoid", "leakyrelu"])}
SCORE_KINDS = [(64, torch.float32), (4096, torch.float32), (64, torch.bfloat16)]
MLP_BINS = 32
MLP_ROWS = 471


def labels_weights(rng, n):
    return (rng.integers(0, 2, n).astype(np.float32),
            WEIGHTS[rng.integers(0, len(WEIGHTS), n)])


def scores_case(nb, n, dtype, one_bin=False, seed=0):
    """(logits tensor, labels, weights, reference bins) as numpy but the logits."""
    rng = np.random.default_rng(seed + nb + n)
    bins = np.full(n, nb // 3) if one_bin else rng.integers(0, nb, n)
    p = (bins + rng.uniform(0.25, 0.75, n)) / nb
    z = torch.from_numpy(np.log(p / (1.0 - p))).to(dtype)
    if dtype == torch.bfloat16:
        s = torch.sigmoid(z.double()).numpy() * nb
        bins = np.floor(s).astype(np.int64)
        keep = np.abs(s - np.round(s)) >= 0.05
        assert keep.mean() >= 0.9
        z, bins = z[torch.from_numpy(keep)], bins[keep]
    y, w = labels_weights(rng, len(bins))
    return z, y, w, bins


def scan(h):
    """(auc, ks) of a [2, NB] histogram by a float64 scan from the top bin."""
    neg, pos = h[0].astype(np.float64), h[1].astype(np.float64)
    P, N = pos.sum(), neg.sum()
    if P == 0 or N == 0:
        return 0.5, 0.0
    area = ks = cp = cn = 0.0
    for b in range(len(pos) - 1, -1, -1):
        area += neg[b] * (cp + 0.5 * pos[b])
        cp += pos[b]
        cn += neg[b]
        ks = max(ks, abs(cp / P - cn / N))
    return area / (P * N), ks


def check(res, nb, bins, y, w, finish=True):
    """Histograms and counts exact against numpy.bincount; AUC against
    auc_score of the bin indices, the rest against `scan`, to 1e-12."""
    slot = (y >= 0.5) * nb + bins
    assert np.array_equal(res["counts"].ravel(), np.bincount(slot, minlength=2 * nb))
    assert np.array_equal(res["wsum"].ravel(),
                          np.bincount(slot, weights=w.astype(np.float64),
                                      minlength=2 * nb))
    pos = int((y >= 0.5).sum())
    assert (res["n"], res["pos"], res["neg"]) == (len(y), pos, len(y) - pos)
    assert res["nonzero"] == int((w != 0).sum())
    if finish:
        assert abs(res["auc"] - auc_score(bins.astype(np.float64), y)) <= 1e-12
        (_, ks), (wauc, wks) = scan(res["counts"]), scan(res["wsum"])
        for k, ref in (("ks", ks), ("wauc", wauc), ("wks", wks)):
            assert abs(res[k] - ref) <= 1e-12, (k, res[k], ref)


def loss_ref(z, y, w, kind):
    """float64 loss sum from float64 logits (numpy)."""
    z, y = torch.from_numpy(z), torch.from_numpy(y.astype(np.float64))
    per = ((torch.sigmoid(z) - y) ** 2 if kind == 0 else
           torch.nn.functional.binary_cross_entropy_with_logits(z, y, reduction="none"))
    return float((torch.from_numpy(w.astype(np.float64)) * per).sum())


@functools.lru_cache(maxsize=None)
def mlp_case(k0, hkey):
    """(cpu model, x fp32 [471, k0], float64 reference scores, labels, weights)."""
    model = _build(k0, *NETS[hkey])
    # seed k0 + 14: the first of k0 + 5, k0 + 6, ... for which every (net, K0, B)
    # case keeps >= 75 % of its rows (worst case keeps 82 %)
    x = torch.randn(MLP_ROWS, k0, generator=torch.Generator().manual_seed(k0 + 14))
    y, w = labels_weights(np.random.default_rng(k0), MLP_ROWS)
    return model, x, _ref64(model, x, rounded=True).numpy(), y, w


def mlp_rows(k0, hkey, B):
    """The first B rows minus those whose reference score lies within TOL of a
    bin edge: (model, x[keep], reference bins, float64 logits, labels, weights)."""
    model, x, ref, y, w = mlp_case(k0, hkey)
    s = ref[:B] * MLP_BINS
    keep = np.abs(s - np.round(s)) >= TOL * MLP_BINS
    assert keep.mean() >= 0.75, f"{(~keep).sum()} of {B} rows near a bin edge"
    p = ref[:B][keep]
    return (model, x[:B][torch.from_numpy(keep)].contiguous(),
            np.floor(s[keep]).astype(np.int64), np.log(p / (1.0 - p)),
            y[:B][keep], w[:B][keep])


def check_mlp(res, bins, z, y, w, kind):
    check(res, MLP_BINS, bins, y, w, finish=False)
    ref = loss_ref(z, y, w, kind)
    # the gate tests/test_ops_gpu.py::test_weighted_loss puts on the loss sum
    assert abs(res["loss_sum"] - ref) <= 1e-2 * max(ref, 1.0), (res["loss_sum"], ref)
