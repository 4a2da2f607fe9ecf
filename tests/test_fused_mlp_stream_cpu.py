"""Streamed-weight MLP scoring — eligibility, LDS arithmetic, packing and the
public surface.  No GPU needed: on CPU tensors stream_predict runs the same
pure-torch emulation as fused_predict."""
import pytest
import torch

from shifu_amd.models.mlp import ShifuMLP
from shifu_amd.models.wide_deep import WideDeep
from shifu_amd.ops.fused_mlp import (STREAM_LDS_LIMIT, _emulate, _shapes_of,
                                     _stream_lds_bytes, fused_eligible,
                                     pack_mlp, pack_mlp_stream, stream_eligible,
                                     stream_predict, unpack_mlp)
from shifu_amd.train.export import export_model, load_exported


def test_eligibility_and_lds_arithmetic():
    tower = ShifuMLP(1864, [1024, 512], ["relu", "relu"])
    assert stream_eligible(tower) == (True, "")
    # A: max(ceil32(1864), 512) = 1888, B: 1024, bf16
    assert _stream_lds_bytes(_shapes_of(tower), 16) == 16 * 2 * (1888 + 1024)
    assert _stream_lds_bytes(_shapes_of(tower), 16) <= STREAM_LDS_LIMIT
    assert _stream_lds_bytes(_shapes_of(tower), 32) > STREAM_LDS_LIMIT

    ok, why = stream_eligible(ShifuMLP(64, [4100], ["relu"]))
    assert not ok and "4100" in why
    two = ShifuMLP(8, [16], ["relu"])
    two.shifu_output_0 = torch.nn.Linear(16, 2)
    ok, why = stream_eligible(two)
    assert not ok and "head width 2" in why
    ok, why = stream_eligible(WideDeep(8, [50, 50], 4, [16], ["relu"]))
    assert not ok and "WideDeep" in why


def test_pack_roundtrip_of_a_net_pack_mlp_refuses():
    model = ShifuMLP(296, [96, 96], ["tanh", "relu"], seed=3).eval()
    with pytest.raises(ValueError):
        pack_mlp(model)
    packed = pack_mlp_stream(model)
    assert packed.kind == "stream" and packed.lds_bytes == 16 * 2 * (320 + 96)
    layers = list(model.hidden) + [model.shifu_output_0]
    for l, (w, b, a) in zip(layers, unpack_mlp(packed)):
        assert torch.equal(w, l.weight.detach().to(torch.bfloat16))
        assert torch.equal(b, l.bias.detach()) and a == l._act


def test_load_exported_fused_true_takes_the_streamed_path(tmp_path):
    model = ShifuMLP(296, [96, 96], ["tanh", "relu"], seed=3).eval()
    mdir = str(tmp_path / "m")
    export_model(model, mdir)
    x = torch.randn(40, 296, generator=torch.Generator().manual_seed(1))
    want = _emulate(pack_mlp_stream(model), x)
    on = load_exported(mdir, fused=True)
    assert on._fused_packed.kind == "stream"
    assert torch.equal(on.predict(x), want)
    assert torch.equal(stream_predict(on._fused_packed, x), want)
    assert not hasattr(load_exported(mdir, fused="auto"), "_fused_packed")


def test_neither_kernel_error_names_both_reasons(tmp_path):
    model = ShifuMLP(64, [4100], ["relu"]).eval()
    mdir = str(tmp_path / "m")
    export_model(model, mdir)
    with pytest.raises(ValueError) as e:
        load_exported(mdir, fused=True)
    assert fused_eligible(model)[1] in str(e.value)
    assert stream_eligible(model)[1] in str(e.value)
