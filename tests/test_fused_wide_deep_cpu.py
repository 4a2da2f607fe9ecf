"""Fused Wide&Deep scoring — eligibility, packing, the CPU emulation and the
`fused_wd` switch.  No GPU needed: on CPU tensors wd_predict runs a pure-torch
emulation with the kernel's rounding points.  Also home of the cases, the
model builder and the fp64 reference the GPU tests share."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from shifu_amd.models.deepfm import DeepFM
from shifu_amd.models.mlp import ShifuMLP
from shifu_amd.models.wide_deep import WideDeep
from shifu_amd.ops.fused_wide_deep import (pack_wide_deep, wd_eligible,
                                           wd_predict)
from shifu_amd.ops.linear import LEAKY_SLOPE
from shifu_amd.train.export import (export_ensemble, export_model,
                                    load_exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-3          # the project's absolute bound per score for this comparison
MIN_STD = 0.02
BMAX = 259

_MIXED26 = [3, 1000, 17, 250, 64, 5, 999, 128, 33, 7, 512, 90, 41, 300, 12, 77,
            640, 4, 201, 58, 831, 26, 150, 9, 444, 63]
# nd, vocab sizes, D, tower, activations
CASES = {
    # scalar loader: chunks straddle dense/embedding and feature boundaries,
    # a size-1 vocab, pad-tile zeroing
    "nd5_d4": (5, [7, 1, 50], 4, [7], ["leakyrelu"]),
    "nd3_d1": (3, [11, 5], 1, [16], ["tanh"]),                  # D = 1, odd nd
    "nd8_d8": (8, [50, 33], 8, [50, 50], ["tanh", "tanh"]),     # smallest vector path
    # the deal wraps, T = 2, ragged 33
    "nd40_d16": (40, [97] * 5, 16, [272, 144, 33], ["relu", "tanh", "sigmoid"]),
    # K0 = 1864, the bench width: a 64-row tile does not fit
    "nd200_d64": (200, _MIXED26, 64, [96, 96], ["tanh", "relu"]),
}


def build(key, seed=42):
    """Project init (fixed seed), randn biases, and wide weights scaled so the
    wide term has a spread near 0.8 in the logit; CPU model."""
    nd, vocab, D, hidden, acts = CASES[key]
    m = WideDeep(nd, vocab, D, hidden, acts, seed=seed)
    g = torch.Generator().manual_seed(seed + 77)
    with torch.no_grad():
        for l in list(m.tower) + [m.shifu_output_0, m.wide_dense]:
            l.bias.copy_(torch.randn(l.bias.shape, generator=g) * 0.1)
        m.wide_dense.weight.copy_(torch.randn(1, nd, generator=g) * 0.5 / nd ** 0.5)
        m.wide_cat.arena.mul_(1.0 / len(vocab) ** 0.5)
    return m.eval()


@functools.lru_cache(maxsize=None)
def inputs(key):
    """(dense [259, nd], ids [259, F]); some rows carry ids outside the vocabulary."""
    nd, vocab, _, _, _ = CASES[key]
    g = torch.Generator().manual_seed(nd + 5)
    dense = torch.randn(BMAX, nd, generator=g)
    sizes = torch.tensor(vocab)
    ids = (torch.rand(BMAX, len(vocab), generator=g) * sizes).long()
    ids[0] = -3                       # B = 1 scores a folded row
    ids[5] = sizes                    # first id past the vocabulary
    ids[16] = sizes * 3 + 2
    ids[200] = -(2 ** 40)
    ids[258] = 2 ** 40 + 1            # needs the 64-bit fold
    return dense, ids


_ACT64 = {"sigmoid": torch.sigmoid, "tanh": torch.tanh, "relu": torch.relu,
          "leakyrelu": lambda z: torch.where(z > 0, z, LEAKY_SLOPE * z)}


def ref64(model, dense, ids):
    """fp64 CPU forward pass with the kernel's rounding points (bf16 tower
    input, weights and activations; the wide term from unrounded values)."""
    def bf(t):
        return t.float().to(torch.bfloat16).double()

    emb = model.embeddings
    rows = ids.clamp(min=0) % emb.sizes + emb.offsets       # MultiEmbedding.forward
    h = torch.cat([bf(dense), bf(emb.arena.detach())[rows.reshape(-1)]
                   .reshape(len(dense), -1)], dim=1)
    for l in model.tower:
        h = bf(_ACT64[l.activation](h @ bf(l.weight.detach()).t()
                                    + l.bias.detach().double()))
    hd, wl = model.shifu_output_0, model.wide_dense
    z = (h @ bf(hd.weight.detach()).t() + hd.bias.detach().double()).reshape(-1)
    wide = (dense.double() @ wl.weight.detach().double().reshape(-1)
            + wl.bias.detach().double()
            + model.wide_cat.arena.detach().double().reshape(-1)[rows].sum(dim=1))
    return 1.0 / (1.0 + torch.exp(-(z + wide)))


@pytest.mark.parametrize("key", list(CASES))
def test_emulation_is_inside_the_bound(key):
    model = build(key)
    dense, ids = inputs(key)
    ref = ref64(model, dense, ids)
    got = wd_predict(pack_wide_deep(model), dense, ids)
    assert got.shape == (BMAX,) and got.dtype == torch.float32
    err = (got.double() - ref).abs().max().item()
    print(f"{key}: max|emulation-ref|={err:.3e} ref std={ref.std().item():.4f}")
    assert ref.std().item() >= MIN_STD
    assert err <= TOL
    if key in ("nd5_d4", "nd3_d1"):     # and of the fp32 layer path
        assert (got - model.predict(dense, ids)).abs().max().item() <= TOL


REFUSED = [
    lambda: ShifuMLP(8, [16], ["relu"]),
    lambda: DeepFM(8, [50, 50], 4, [16], ["relu"]),
    lambda: WideDeep(8, [50, 50], 4, [16], ["relu"], unified=True),
    lambda: WideDeep(8, [50, 50], 4, [16] * 8, ["relu"] * 8),      # 9 layers
    lambda: WideDeep(8, [50, 50], 4, [4100], ["relu"]),
]


def test_eligibility_and_packing(tmp_path):
    mdir = str(tmp_path / "wd")
    model = build("nd8_d8")
    export_model(model, mdir)
    loaded = load_exported(mdir)
    assert wd_eligible(loaded) == (True, "")
    packed = pack_wide_deep(loaded)
    assert (packed.num_dense, packed.num_cat, packed.embed_dim) == (8, 2, 8)
    assert packed.feat_table.tolist() == [[0, 50], [50, 33]]
    assert torch.equal(packed.arena, model.embeddings.arena.detach().to(torch.bfloat16))
    assert torch.equal(packed.wide_vec, model.wide_cat.arena.detach().reshape(-1))
    # A: ceil32(24) = 32 and ceil32(50) = 64 -> 64; B: 64; + wide + 2 ids per row
    assert packed.lds_bytes == 16 * 2 * (64 + 64) + 16 * 4 + 16 * 2 * 4

    reasons = [wd_eligible(make()) for make in REFUSED]
    assert all(not ok and why for ok, why in reasons)
    assert len(set(reasons)) == len(REFUSED)
    for make in REFUSED:
        with pytest.raises(ValueError):
            pack_wide_deep(make())


def test_fused_wd_switch(tmp_path):
    from shifu_amd.serve import ShifuScorer
    wd_dir, mlp_dir, ens_dir = (str(tmp_path / n) for n in ("wd", "mlp", "ens"))
    model = build("nd5_d4")
    dense, ids = inputs("nd5_d4")
    export_model(model, wd_dir)
    export_model(ShifuMLP(8, [16], ["relu"]), mlp_dir)
    export_ensemble([ShifuMLP(8, [16], ["relu"], seed=s) for s in (1, 2)], ens_dir)

    want = wd_predict(pack_wide_deep(model), dense, ids)
    on = load_exported(wd_dir, fused_wd=True)
    assert torch.equal(on.predict(dense, ids), want)
    assert torch.equal(wd_predict(on._fused_wd_packed, dense, ids), want)
    assert not hasattr(load_exported(wd_dir), "_fused_wd_packed")
    sc = ShifuScorer()
    sc.init(os.path.join(wd_dir, "GenericModelConfig.json"), fused_wd=True)
    assert np.array_equal(sc.compute_batch(dense.numpy(), ids.numpy()), want.numpy())

    for d in (mlp_dir, ens_dir):
        with pytest.raises(ValueError, match="not a WideDeep"):
            load_exported(d, fused_wd=True)
        with pytest.raises(ValueError, match="not a WideDeep"):
            ShifuScorer().init(os.path.join(d, "GenericModelConfig.json"),
                               fused_wd=True)


def test_score_cli_fused_wd_on_matches_the_api(tmp_path):
    model = build("nd5_d4")
    dense, ids = inputs("nd5_d4")
    mdir = str(tmp_path / "m")
    export_model(model, mdir)
    data = tmp_path / "part-0.csv"
    data.write_text("\n".join(
        "|".join([f"{v:.6f}" for v in d] + [str(int(c)) for c in i])
        for d, i in zip(dense[:40].tolist(), ids[:40, :].clamp(-9, 99).tolist())) + "\n")
    out = tmp_path / "scores.csv"
    r = subprocess.run(
        [sys.executable, "-m", "shifu_amd.score", "--model", mdir, "--data",
         str(data), "--output", str(out), "--device", "cpu", "--fused-wd", "on"],
        capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.array([float(l) for l in out.read_text().splitlines()])
    from shifu_amd.score import score_files
    want, _ = score_files(mdir, [str(data)], fused_wd=True)
    assert got.shape == (40,) and np.abs(got - want).max() <= 5e-7   # %.6f print
