"""Fused ensemble scoring kernel (ops/hip/fused_mlp.hip,
mlp_score_fused_ensemble) on the GPU.

Exactness: every member column must be bitwise the single-model fused kernel's
score of that member, and the mean must be bitwise the fp32 left-to-right sum
of those columns times float32(1/M) — however the members are split into
launches.  Numerics: the mean against the mean of the members' fp64 references
with the kernel's rounding points, same 2e-3 absolute bound per row the
single-model tests use (the mean of M values each within the bound is within
the bound; the fp32 sum and scale add < 1e-6).
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from shifu_amd.models.ensemble import EnsembleModel
from shifu_amd.models.mlp import ShifuMLP
from shifu_amd.ops.dispatch import hip_available, hip_ops
from shifu_amd.ops.fused_mlp import (fused_ensemble_predict, fused_predict,
                                     pack_ensemble, pack_mlp)
from shifu_amd.ops.linear import LEAKY_SLOPE

TOL = 2e-3
MIN_STD = 0.02
BMAX = 259
# Member i is built from seed SEED0 + i.  With 42 + i the fp64 reference of
# h16x7 (seed 43) has std 0.0146 and of h33_17_5 (seed 43) 0.0185 over the 259
# rows at K0 = 5, under the MIN_STD guard; from 44 every member of every case
# below has std >= 0.029 (checked on the CPU).
SEED0 = 44


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    assert torch.cuda.is_available(), "GPU test requires a GPU"
    assert hip_available(), "HIP extension must be built (native code not loaded!)"


HIDDEN = {
    "h7": ([7], ["leakyrelu"]),
    "h50x2": ([50, 50], ["tanh", "tanh"]),
    "h33_17_5": ([33, 17, 5], ["tanh", "relu", "sigmoid"]),
    # 8 layers counting the head: the per-member limit
    "h16x7": ([16] * 7, ["tanh", "leakyrelu", "tanh", "tanh", "leakyrelu",
                         "tanh", "tanh"]),
}
SETS = {
    "one": ["h7"],
    "pair": ["h50x2", "h50x2"],
    "mixed": ["h7", "h33_17_5", "h50x2"],
    # 40 layers > 32 per launch: two groups [4, 1] with a carried partial sum
    "deep5": ["h16x7"] * 5,
}
K0S = [5, 37, 200]
BS = [1, 15, 16, 17, 259]


def _build(k0, hidden, acts, seed=42):
    """Project xavier init (fixed seed), biases randn*0.1; CPU model."""
    m = ShifuMLP(k0, hidden, acts, seed=seed)
    g = torch.Generator().manual_seed(seed + 77)
    with torch.no_grad():
        for l in list(m.hidden) + [m.shifu_output_0]:
            l.bias.copy_(torch.randn(l.bias.shape, generator=g) * 0.1)
    return m.eval()


def _members(k0, skey):
    """Members of set `skey` at input width k0, seeds SEED0 + i; CPU models."""
    return [_build(k0, *HIDDEN[h], seed=SEED0 + i)
            for i, h in enumerate(SETS[skey])]


def _act64(z, name):
    if name == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-z))
    if name == "tanh":
        return torch.tanh(z)
    if name == "relu":
        return torch.clamp(z, min=0.0)
    if name == "leakyrelu":
        return torch.where(z > 0, z, LEAKY_SLOPE * z)
    return z


def _ref64(model, x):
    """fp64 CPU forward pass with the kernel's bf16 rounding points."""
    def bf(t):
        return t.float().to(torch.bfloat16).double()

    h = bf(x)
    for l in model.hidden:
        z = h @ bf(l.weight.detach()).t() + l.bias.detach().double()
        h = bf(_act64(z, l.activation))
    hd = model.shifu_output_0
    z = h @ bf(hd.weight.detach()).t() + hd.bias.detach().double()
    return (1.0 / (1.0 + torch.exp(-z))).reshape(-1)


def _sum_scale(members):
    """fp32 left-to-right sum of the columns of [B, M], times float32(1/M)."""
    total = torch.zeros_like(members[:, 0])
    for i in range(members.shape[1]):
        total = total + members[:, i]
    scale = torch.tensor(1.0 / members.shape[1], dtype=torch.float32,
                         device=members.device)
    return total * scale


@functools.lru_cache(maxsize=None)
def _case(k0, skey):
    """(cpu members, ensemble packed on GPU, per-member packs on GPU,
    x cpu [259, k0], x gpu, per-member fp64 references)."""
    models = _members(k0, skey)
    x = torch.randn(BMAX, k0, generator=torch.Generator().manual_seed(k0 + 5))
    refs = [_ref64(m, x) for m in models]
    gpu = [m.cuda() for m in _members(k0, skey)]
    return models, pack_ensemble(gpu), [pack_mlp(m) for m in gpu], x, x.cuda(), refs


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("skey", list(SETS))
@pytest.mark.parametrize("k0", K0S)
def test_member_exactness(k0, skey, B):
    _, packed, singles, _, xg, _ = _case(k0, skey)
    xb = xg[:B].contiguous()
    mean, members = fused_ensemble_predict(packed, xb, return_members=True)
    M = len(singles)
    assert mean.shape == (B,) and mean.dtype == torch.float32 and mean.is_cuda
    assert members.shape == (B, M) and members.dtype == torch.float32
    for i, single in enumerate(singles):
        assert torch.equal(members[:, i], fused_predict(single, xb)), f"member {i}"
    assert torch.equal(mean, _sum_scale(members))
    assert torch.equal(mean.cpu(), _sum_scale(members.cpu()))
    # without the member columns: the same mean
    assert torch.equal(fused_ensemble_predict(packed, xb), mean)


def test_member_without_hidden_layers():
    """A member that is only a head (K0 -> 1) computes its score straight from
    the shared layer-0 registers, between members that use the LDS buffers."""
    gpu = [_build(37, [], [], seed=SEED0).cuda(),
           _build(37, *HIDDEN["h7"], seed=SEED0 + 1).cuda(),
           _build(37, [], [], seed=SEED0 + 2).cuda()]
    _, _, _, _, xg, _ = _case(37, "one")
    mean, members = fused_ensemble_predict(pack_ensemble(gpu), xg,
                                           return_members=True)
    for i, m in enumerate(gpu):
        assert torch.equal(members[:, i], fused_predict(pack_mlp(m), xg))
    assert torch.equal(mean, _sum_scale(members))
    assert members.std(dim=0).min().item() >= MIN_STD


def test_deep5_spans_two_launches():
    _, packed, _, _, _, _ = _case(37, "deep5")
    assert packed.group_sizes == [4, 1]


@pytest.mark.parametrize("skey", list(SETS))
@pytest.mark.parametrize("k0", K0S)
def test_reference_numerics(k0, skey):
    _, packed, _, _, xg, refs = _case(k0, skey)
    for i, r in enumerate(refs):
        std = r.std().item()
        print(f"k0={k0} {skey} member {i}: ref std={std:.4f}")
        assert std >= MIN_STD
    want = torch.stack(refs, dim=1).mean(dim=1)
    got = fused_ensemble_predict(packed, xg)
    err = (got.double().cpu() - want).abs().max().item()
    print(f"k0={k0} {skey}: max|mean-ref|={err:.3e}")
    assert err <= TOL


def test_grouping_is_bitwise_invisible():
    """3 x (200 -> [50, 50]) packs as [2, 1]; the first launch takes the
    > 64 KiB dynamic-LDS path.  Forcing [1, 1, 1] must not change a bit."""
    gpu = [m.cuda() for m in _members(200, "pair")] + \
        [_build(200, *HIDDEN["h50x2"], seed=SEED0 + 2).cuda()]
    x = torch.randn(BMAX, 200, generator=torch.Generator().manual_seed(205)).cuda()
    packed = pack_ensemble(gpu)
    assert packed.group_sizes == [2, 1]
    assert packed.group_lds_bytes[0] == 111744 > 65536
    forced = pack_ensemble(gpu, max_group_bytes=39488 + 32768)
    assert forced.group_sizes == [1, 1, 1]
    mean, members = fused_ensemble_predict(packed, x, return_members=True)
    fmean, fmembers = fused_ensemble_predict(forced, x, return_members=True)
    assert torch.equal(mean, fmean) and torch.equal(members, fmembers)
    assert torch.equal(mean, _sum_scale(members))
    for i, m in enumerate(gpu):
        assert torch.equal(members[:, i], fused_predict(pack_mlp(m), x))
    assert members.std(dim=0).min().item() >= MIN_STD


@pytest.mark.parametrize("waves", [2, 4, 8])
def test_grid_stride_wrap(waves):
    """One block walks all 17 tiles; bitwise the default launch."""
    _, packed, _, _, xg, _ = _case(37, "mixed")
    mean, members = fused_ensemble_predict(packed, xg, return_members=True)
    wmean, wmembers = fused_ensemble_predict(packed, xg, return_members=True,
                                             max_blocks=1, waves=waves)
    assert torch.equal(mean, wmean) and torch.equal(members, wmembers)


def test_row_independence_and_determinism():
    _, packed, _, _, xg, _ = _case(37, "mixed")
    mean, members = fused_ensemble_predict(packed, xg, return_members=True)
    for _ in range(4):
        again, mem2 = fused_ensemble_predict(packed, xg, return_members=True)
        assert torch.equal(again, mean) and torch.equal(mem2, members)
    single = torch.cat([fused_ensemble_predict(packed, xg[i:i + 1].contiguous())
                        for i in range(BMAX)])
    assert torch.equal(single, mean)
    # two launches with a carried partial sum
    _, packed, _, _, xg, _ = _case(200, "deep5")
    mean = fused_ensemble_predict(packed, xg)
    single = torch.cat([fused_ensemble_predict(packed, xg[i:i + 1])
                        for i in range(BMAX)])
    assert torch.equal(single, mean)


def test_host_checks_never_launch():
    """A malformed table is rejected by the host function before any launch."""
    ext = hip_ops()
    _, packed, _, _, xg, _ = _case(37, "pair")
    blob, table = packed.blobs[0], packed.tables[0]
    assert ext.mlp_score_fused_ensemble(xg, [blob], [table])[0].shape == (BMAX,)

    shifted = table.clone()
    shifted[shifted[:, 0] == 1, 1] += 16       # second member's offsets + 16
    with pytest.raises(RuntimeError, match="offset"):
        ext.mlp_score_fused_ensemble(xg, [blob], [shifted])

    unchained = table.clone()
    unchained[4, 3] = 49                       # member 1, layer 1: K 50 -> 49
    with pytest.raises(RuntimeError, match="does not chain"):
        ext.mlp_score_fused_ensemble(xg, [blob], [unchained])

    with pytest.raises(RuntimeError, match="does not chain"):   # rows too narrow
        ext.mlp_score_fused_ensemble(xg[:, :36].contiguous(), [blob], [table])

    one = pack_mlp(_build(37, *HIDDEN["h7"]).cuda())
    nine_blob = one.blob.repeat(9)
    rows = [[mi, mi * one.blob.numel() + o, n, k, a]
            for mi in range(9) for o, n, k, a in one.table.tolist()]
    with pytest.raises(RuntimeError, match="members in one group"):
        ext.mlp_score_fused_ensemble(
            xg, [nine_blob], [torch.tensor(rows, dtype=torch.int32)])
    # the same nine members split [8, 1] are fine
    ok = ext.mlp_score_fused_ensemble(
        xg, [one.blob.repeat(8), one.blob],
        [torch.tensor(rows[:16], dtype=torch.int32),
         torch.tensor(rows[:2], dtype=torch.int32)], True)
    want = fused_predict(one, xg)
    assert ok[1].shape == (BMAX, 9)
    assert all(torch.equal(ok[1][:, i], want) for i in range(9))
    assert torch.equal(ok[0], _sum_scale(ok[1]))

    with pytest.raises(RuntimeError, match="trailing"):
        ext.mlp_score_fused_ensemble(xg, [torch.cat([blob, blob[:16]])], [table])
    with pytest.raises(RuntimeError):
        ext.mlp_score_fused_ensemble(xg, [blob, blob], [table])
    wide = torch.zeros(4, 520, device="cuda")
    with pytest.raises(RuntimeError, match="input width"):
        ext.mlp_score_fused_ensemble(wide, [blob], [table])


def test_end_to_end_export_load_score(tmp_path):
    from shifu_amd.serve import ShifuScorer
    from shifu_amd.train.export import export_ensemble, load_exported

    models, packed, _, x, xg, _ = _case(200, "mixed")
    mdir = str(tmp_path / "bag")
    export_ensemble(models, mdir)
    want, want_members = fused_ensemble_predict(packed, xg, return_members=True)

    loaded = load_exported(mdir, device="cuda", fused=True)
    assert torch.equal(loaded.predict(xg), want)
    assert torch.equal(loaded.predict_members(xg), want_members)

    cfg = os.path.join(mdir, "GenericModelConfig.json")
    sc = ShifuScorer()
    sc.init(cfg, device="cuda", fused=True)
    assert sc.num_members == 3
    assert np.array_equal(sc.compute_batch(x.numpy()), want.cpu().numpy())
    p, mem = sc.compute_batch(x.numpy(), return_members=True)
    assert np.array_equal(p, want.cpu().numpy())
    assert np.array_equal(mem, want_members.cpu().numpy())
    for i in (0, 15, 16, 258):
        assert sc.compute(x[i].tolist()) == float(want[i])
        assert sc.compute_members(x[i].tolist()) == \
            [float(v) for v in want_members[i].cpu()]

    # fused=False: the layer path, bitwise EnsembleModel.predict
    direct = EnsembleModel([m.cuda() for m in _members(200, "mixed")]).predict(xg)
    off = ShifuScorer()
    off.init(cfg, device="cuda")
    assert not hasattr(off.model, "_fused_packed")
    assert np.array_equal(off.compute_batch(x.numpy()), direct.cpu().numpy())
