"""Fused whole-network MLP scoring kernel (ops/hip/fused_mlp.hip) on the GPU.

Reference for the numerics cases: fp64 on the CPU with the kernel's rounding
points (bf16 input and weights, fp32 bias, bf16 activations between layers,
unrounded head logit, sigmoid).  The kernel can differ from it only through
fp32 summation order and the occasional bf16 tie flip that causes, measured
at <= 3.4e-4 on the CPU for these inits; the bound is 2e-3 absolute per row.
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from shifu_amd.models.mlp import ShifuMLP
from shifu_amd.ops.dispatch import hip_available
from shifu_amd.ops.fused_mlp import (LDS_LIMIT, fused_eligible, fused_predict,
                                     pack_mlp)
from shifu_amd.ops.linear import LEAKY_SLOPE

TOL = 2e-3
MIN_STD = 0.02
BMAX = 259


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    assert torch.cuda.is_available(), "GPU test requires a GPU"
    assert hip_available(), "HIP extension must be built (native code not loaded!)"


HIDDEN = {
    "h7": ([7], ["leakyrelu"]),
    "h50x2": ([50, 50], ["tanh", "tanh"]),
    "h33_17_5": ([33, 17, 5], ["tanh", "relu", "sigmoid"]),
    # 8 layers counting the head: the kernel's limit
    "h16x7": ([16] * 7, ["tanh", "leakyrelu", "tanh", "tanh", "leakyrelu",
                         "tanh", "tanh"]),
}
K0S = [5, 32, 37, 200]
BS = [1, 15, 16, 17, 259]


def _build(k0, hidden, acts, seed=42):
    """Project xavier init (fixed seed), biases randn*0.1; CPU model."""
    m = ShifuMLP(k0, hidden, acts, seed=seed)
    g = torch.Generator().manual_seed(seed + 77)
    with torch.no_grad():
        for l in list(m.hidden) + [m.shifu_output_0]:
            l.bias.copy_(torch.randn(l.bias.shape, generator=g) * 0.1)
    return m.eval()


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


def _ref64(model, x, rounded=True):
    """fp64 CPU forward pass; rounded=True applies the kernel's bf16 rounding
    points, rounded=False is the exact forward pass of the fp32 model."""
    def bf(t):
        return t.float().to(torch.bfloat16).double() if rounded else t.double()

    h = bf(x)
    for l in model.hidden:
        z = h @ bf(l.weight.detach()).t() + l.bias.detach().double()
        h = bf(_act64(z, l.activation))
    hd = model.shifu_output_0
    z = h @ bf(hd.weight.detach()).t() + hd.bias.detach().double()
    return (1.0 / (1.0 + torch.exp(-z))).reshape(-1)


@functools.lru_cache(maxsize=None)
def _case(k0, hkey):
    """(cpu model, packed on GPU, x cpu [259, k0], x gpu, fp64 reference)."""
    hidden, acts = HIDDEN[hkey]
    model = _build(k0, hidden, acts)
    x = torch.randn(BMAX, k0, generator=torch.Generator().manual_seed(k0 + 5))
    ref = _ref64(model, x)
    packed = pack_mlp(_build(k0, hidden, acts).cuda())
    return model, packed, x, x.cuda(), ref


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("hkey", list(HIDDEN))
@pytest.mark.parametrize("k0", K0S)
def test_numerics(k0, hkey, B):
    _, packed, _, xg, ref = _case(k0, hkey)
    got = fused_predict(packed, xg[:B].contiguous())
    assert got.shape == (B,) and got.dtype == torch.float32 and got.is_cuda
    err = (got.double().cpu() - ref[:B]).abs().max().item()
    std = ref.std().item()
    print(f"k0={k0} {hkey} B={B}: max|score-ref|={err:.3e} ref std={std:.4f}")
    assert std >= MIN_STD
    assert err <= TOL


def test_wide_input_register_path():
    """K0 = 520 -> 17 k-steps: the widest layer-0 register instantiation, with
    a K0 that is a multiple of 4 but not of 32."""
    model = _build(520, [16], ["tanh"])
    x = torch.randn(37, 520, generator=torch.Generator().manual_seed(9))
    ref = _ref64(model, x)
    got = fused_predict(pack_mlp(_build(520, [16], ["tanh"]).cuda()), x.cuda())
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"520->[16]: max err {err:.3e} std {ref.std().item():.4f}")
    assert ref.std().item() >= MIN_STD
    assert err <= TOL


def test_no_worse_than_layer_path():
    """200 -> [50, 50], B = 259, against the UNROUNDED fp64 forward pass: the
    fused path (fp32 head logit) must be at least as close as model.predict
    through the per-layer kernels (bf16 head logit)."""
    model, packed, x, xg, _ = _case(200, "h50x2")
    exact = _ref64(model, x, rounded=False)
    fused = fused_predict(packed, xg).double().cpu()
    hidden, acts = HIDDEN["h50x2"]
    layer = _build(200, hidden, acts).cuda().predict(xg).double().cpu()
    e_fused = (fused - exact).abs().max().item()
    e_layer = (layer - exact).abs().max().item()
    print(f"max err vs exact fp64: fused {e_fused:.3e}  layer path {e_layer:.3e}")
    assert e_fused <= e_layer


def test_row_independence():
    """Every row scored alone at B = 1 is bitwise its score in the batch."""
    _, packed, _, xg, _ = _case(200, "h50x2")
    batch = fused_predict(packed, xg)
    single = torch.cat([fused_predict(packed, xg[i:i + 1]) for i in range(BMAX)])
    assert torch.equal(batch, single)
    # and for a K0 on the dword-load path with a ragged last tile
    _, packed, _, xg, _ = _case(37, "h33_17_5")
    batch = fused_predict(packed, xg)
    single = torch.cat([fused_predict(packed, xg[i:i + 1].contiguous())
                        for i in range(BMAX)])
    assert torch.equal(batch, single)


def test_determinism():
    _, packed, _, xg, _ = _case(200, "h50x2")
    first = fused_predict(packed, xg)
    for _ in range(4):
        assert torch.equal(fused_predict(packed, xg), first)


@pytest.mark.parametrize("waves", [2, 4, 8])
def test_grid_stride_wrap(waves):
    """One block walks all 17 tiles; bitwise the default launch."""
    _, packed, _, xg, ref = _case(200, "h50x2")
    default = fused_predict(packed, xg)
    wrapped = fused_predict(packed, xg, max_blocks=1, waves=waves)
    assert torch.equal(default, wrapped)
    assert (wrapped.double().cpu() - ref).abs().max().item() <= TOL


def test_lds_ceiling():
    """264 -> [96, 96] needs 126784 B of LDS (weights + 8 waves' activation
    buffers): the largest net of this shape under the 128 KiB ceiling, and it
    takes the > 64 KiB dynamic-LDS launch.  296 -> [96, 96] needs 132928 B and
    must be reported not eligible (never launched)."""
    hidden, acts = [96, 96], ["tanh", "relu"]
    model = _build(264, hidden, acts)
    ok, why = fused_eligible(model)
    assert ok, why
    packed = pack_mlp(_build(264, hidden, acts).cuda())
    assert packed.lds_bytes == 126784 and 65536 < packed.lds_bytes <= LDS_LIMIT
    x = torch.randn(BMAX, 264, generator=torch.Generator().manual_seed(2))
    ref = _ref64(model, x)
    got = fused_predict(packed, x.cuda())
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"264->[96,96]: max err {err:.3e} std {ref.std().item():.4f}")
    assert ref.std().item() >= MIN_STD
    assert err <= TOL

    over = _build(296, hidden, acts)
    ok, why = fused_eligible(over)
    assert not ok and "132928" in why
    with pytest.raises(ValueError):
        pack_mlp(over)


def test_end_to_end_export_load_score(tmp_path):
    from shifu_amd.serve import ShifuScorer
    from shifu_amd.train.export import export_model, load_exported

    model, packed, x, xg, _ = _case(200, "h50x2")
    mdir = str(tmp_path / "bundle")
    export_model(model, mdir)
    want = fused_predict(packed, xg).cpu().numpy()

    loaded = load_exported(mdir, device="cuda", fused=True)
    assert torch.equal(loaded.predict(xg).cpu(), torch.from_numpy(want))

    cfg = os.path.join(mdir, "GenericModelConfig.json")
    sc = ShifuScorer()
    sc.init(cfg, device="cuda", fused=True)
    assert np.array_equal(sc.compute_batch(x.numpy()), want)
    for i in (0, 1, 15, 16, 258):
        assert sc.compute(x[i].tolist()) == float(want[i])

    # fused=False: still the layer path, bitwise a direct model.predict
    hidden, acts = HIDDEN["h50x2"]
    direct = _build(200, hidden, acts).cuda().predict(xg).float().cpu().numpy()
    off = ShifuScorer()
    off.init(cfg, device="cuda")
    assert not hasattr(off.model, "_fused_packed")
    assert np.array_equal(off.compute_batch(x.numpy()), direct)
