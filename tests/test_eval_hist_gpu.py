"""The evaluation kernels of ops/hip/eval_hist.hip on the GPU, against the
exact references of tests/eval_hist_cases.py: histograms and counts bitwise,
AUC / KS to 1e-12, the fused MLP path on rows whose reference score is at
least TOL away from a bin edge."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_hist_cases as ec  # noqa: E402
from shifu_amd.ops.dispatch import hip_available  # noqa: E402
from shifu_amd.ops.eval_hist import EvalAccumulator  # noqa: E402
from shifu_amd.ops.fused_mlp import pack_mlp  # noqa: E402
from test_eval_hist_cpu import check_on_off, trainer_on_off  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    assert torch.cuda.is_available(), "GPU test requires a GPU"
    assert hip_available(), "HIP extension must be built (native code not loaded!)"


def _gpu(*arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


# n = 70001 makes the CU-capped grid loop; (70001, True) puts every row in ONE
# bin (the replicated-histogram scheme); odd n take the partial last piece
@pytest.mark.parametrize("n,one_bin", [(1, False), (63, False), (1000, False),
                                       (70001, False), (70001, True)])
@pytest.mark.parametrize("nb,dtype", ec.SCORE_KINDS)
def test_scores_histogram_and_finish(nb, dtype, n, one_bin):
    z, y, w, bins = ec.scores_case(nb, n, dtype, one_bin)
    acc = EvalAccumulator(nb, "cuda")
    acc.add_scores(z.cuda(), *_gpu(y, w), kind=1)
    res = acc.result()
    ec.check(res, nb, bins, y, w)
    ref = ec.loss_ref(z.double().numpy(), y, w, 1)
    assert abs(res["loss_sum"] - ref) <= 1e-2 * max(ref, 1.0)

    # two calls (the second from an unaligned view: the dword-load variant)
    # accumulate to the single-call histogram; reset() clears the state
    acc.reset()
    h = len(bins) // 2 + 1
    zg, yg, wg = z.cuda(), *_gpu(y, w)
    for sl in (slice(0, h), slice(h, None)):
        acc.add_scores(zg[sl], yg[sl], wg[sl], kind=1)
    two = acc.result()
    assert np.array_equal(two["counts"], res["counts"])
    assert np.array_equal(two["wsum"], res["wsum"])
    assert (two["auc"], two["ks"], two["nonzero"]) == (res["auc"], res["ks"], res["nonzero"])


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_empty_class(label):
    z, y, w, bins = ec.scores_case(64, 1000, torch.float32)
    y = np.full_like(y, label)
    acc = EvalAccumulator(64, "cuda")
    acc.add_scores(z.cuda(), *_gpu(y, w))
    res = acc.result()
    ec.check(res, 64, bins, y, w)
    assert res["auc"] == 0.5 and res["ks"] == 0.0


def _mlp(hkey, k0, B, dtype, kind, max_blocks=0):
    model, x, bins, z, y, w = ec.mlp_rows(k0, hkey, B)
    acc = EvalAccumulator(ec.MLP_BINS, "cuda")
    acc.add_mlp(pack_mlp(copy.deepcopy(model).cuda()), x.cuda().to(dtype),
                *_gpu(y, w), kind=kind, max_blocks=max_blocks)
    ec.check_mlp(acc.result(), bins, z, y, w, kind)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 17, 259])
@pytest.mark.parametrize("k0", [5, 37, 200])
@pytest.mark.parametrize("hkey", list(ec.NETS))
def test_mlp_fused(hkey, k0, B, dtype, kind):
    _mlp(hkey, k0, B, dtype, kind)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mlp_fused_single_block_wraps(dtype):
    """One block walks all the tiles of B = 471: its 8 waves wrap."""
    _mlp("h50x2", 200, ec.MLP_ROWS, dtype, 0, max_blocks=1)


def test_trainer_device_eval():
    """9 layers: the add_scores route, fed the model's bf16 logits."""
    on, off = trainer_on_off([4] * 8, "cuda")
    check_on_off(on, off, same_scores=True)
