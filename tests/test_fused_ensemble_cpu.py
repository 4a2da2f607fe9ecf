"""Fused ensemble scoring — packing, grouping, eligibility, CPU emulation and
the public surface (export_ensemble / load_exported / ShifuScorer / score.py /
server).  No GPU needed: on CPU tensors fused_ensemble_predict runs the
pure-torch emulation with the kernel's rounding points and summation order."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from shifu_amd.config.model_config import ModelConfig
from shifu_amd.models.ensemble import EnsembleModel
from shifu_amd.models.mlp import ShifuMLP
from shifu_amd.models.wide_deep import WideDeep
from shifu_amd.ops.fused_mlp import (LDS_LIMIT, WAVES, _lds_bytes,
                                     ensemble_eligible, ensemble_members,
                                     fused_ensemble_predict, fused_predict,
                                     pack_ensemble, pack_mlp, unpack_mlp)
from shifu_amd.serve import ShifuScorer
from shifu_amd.train.export import (export_ensemble, load_exported,
                                    load_exported_ensemble)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one row scored alone against the same row scored in a batch, on the CPU
ROW_TOL = 1e-6
# a score printed with six decimals is within 5e-7 of the value; the CLI runs
# in another process, allow its CPU GEMM the same ROW_TOL on top
PRINT_TOL = 5e-7 + ROW_TOL

HETERO = [([7], ["leakyrelu"]),
          ([33, 17, 5], ["tanh", "relu", "sigmoid"]),
          ([50, 50], ["tanh", "tanh"])]


def _model(k0, hidden, acts, seed=7):
    m = ShifuMLP(k0, hidden, acts, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for l in list(m.hidden) + [m.shifu_output_0]:
            l.bias.copy_(torch.randn(l.bias.shape, generator=g) * 0.1)
    return m.eval()


def _hetero(k0=37):
    return [_model(k0, h, a, seed=7 + i) for i, (h, a) in enumerate(HETERO)]


def _same(k0, m, hidden=(50, 50)):
    return [_model(k0, list(hidden), ["tanh"] * len(hidden), seed=7 + i)
            for i in range(m)]


def _sum_scale(cols):
    """fp32 left-to-right sum in member order, times float32(1/M)."""
    total = torch.zeros_like(cols[0])
    for c in cols:
        total = total + c
    return total * torch.tensor(1.0 / len(cols), dtype=torch.float32)


@pytest.mark.parametrize("budget", [LDS_LIMIT, 52000])
def test_pack_roundtrip_heterogeneous(budget):
    models = _hetero()
    packed = pack_ensemble(models, max_group_bytes=budget)
    assert packed.num_members == 3 and packed.num_features == 37
    assert sum(packed.group_sizes) == 3
    assert len(packed.blobs) == len(packed.tables) == len(packed.group_sizes)
    if budget == 52000:
        assert len(packed.group_sizes) > 1
    # every group is the members' pack_mlp images back to back
    it = iter(models)
    for blob, table, n in zip(packed.blobs, packed.tables, packed.group_sizes):
        assert blob.dtype == torch.uint8 and blob.numel() % 16 == 0
        assert table.dtype == torch.int32 and table.shape[1] == 5
        assert table[:, 0].tolist() == sorted(table[:, 0].tolist())
        assert int(table[-1, 0]) == n - 1
        want = torch.cat([pack_mlp(next(it)).blob for _ in range(n)])
        assert torch.equal(blob, want)
    # and unpacks, through the fragment-order inverse, to the members' values
    views = ensemble_members(packed)
    assert len(views) == 3
    for model, view in zip(models, views):
        layers = list(model.hidden) + [model.shifu_output_0]
        got = unpack_mlp(view)
        assert len(got) == len(layers)
        for l, (w, b, a) in zip(layers, got):
            assert w.dtype == torch.bfloat16 and b.dtype == torch.float32
            assert torch.equal(w, l.weight.detach().to(torch.bfloat16))
            assert torch.equal(b, l.bias.detach())
            assert a == l._act


def test_grouping_arithmetic():
    shapes200 = [(50, 200), (50, 50), (1, 50)]
    member = pack_mlp(_model(200, [50, 50], ["tanh", "tanh"])).blob.numel()
    bufs = 2 * WAVES * 32 * 64
    assert member == 39488 and bufs == 32768
    assert _lds_bytes(shapes200) == member + bufs

    two = pack_ensemble(_same(200, 2))
    assert two.group_sizes == [2] and two.group_lds_bytes == [111744]
    assert two.group_lds_bytes[0] == 2 * member + bufs

    assert 3 * member + bufs == 151232 > LDS_LIMIT
    three = pack_ensemble(_same(200, 3))
    assert three.group_sizes == [2, 1]
    assert three.group_lds_bytes == [111744, member + bufs]
    assert [b.numel() for b in three.blobs] == [2 * member, member]

    five = pack_ensemble(_same(30, 5))
    m30 = pack_mlp(_model(30, [50, 50], ["tanh", "tanh"])).blob.numel()
    assert m30 == 14912
    assert five.group_sizes == [5] and five.group_lds_bytes == [107328]
    assert 5 * m30 + bufs == 107328

    forced = pack_ensemble(_same(200, 3), max_group_bytes=member + bufs)
    assert forced.group_sizes == [1, 1, 1]
    with pytest.raises(ValueError, match="max_group_bytes"):
        pack_ensemble(_same(200, 3), max_group_bytes=member + bufs - 16)

    # the activation buffers are sized by the widest hidden layer of ANY member
    mixed = pack_ensemble([_model(30, [16], ["tanh"]),
                           _model(30, [96, 96], ["tanh", "relu"])])
    assert mixed.group_sizes == [2]
    blob = sum(b.numel() for b in mixed.blobs)
    assert mixed.group_lds_bytes == [blob + 2 * WAVES * 32 * 96]

    # at most 8 members share one launch
    nine = pack_ensemble(_same(5, 9, hidden=(7,)))
    assert nine.group_sizes == [8, 1]
    # at most 32 layers share one launch: 5 x 8 layers -> [4, 1]
    deep = pack_ensemble(_same(5, 5, hidden=(16,) * 7))
    assert deep.group_sizes == [4, 1]


def test_eligibility_reasons():
    ok, why = ensemble_eligible(_hetero())
    assert ok and why == ""
    reasons = {}
    reasons["widths"] = ensemble_eligible(
        [_model(30, [8], ["tanh"]), _model(31, [8], ["tanh"])])
    reasons["wide"] = ensemble_eligible([_model(520, [16], ["tanh"])] * 2)
    head2 = _model(30, [8], ["tanh"])
    head2.shifu_output_0 = type(head2.shifu_output_0)(8, 2, activation="none")
    reasons["head"] = ensemble_eligible([_model(30, [8], ["tanh"]), head2])
    reasons["count"] = ensemble_eligible([_model(5, [7], ["tanh"])] * 65)
    reasons["family"] = ensemble_eligible(
        [_model(8, [16], ["relu"]), WideDeep(8, [50, 50], 4, [16], ["relu"])])
    reasons["empty"] = ensemble_eligible([])
    for key, (ok, why) in reasons.items():
        assert not ok and why, key
    assert "input width" in reasons["widths"][1] and "30" in reasons["widths"][1] \
        and "31" in reasons["widths"][1]
    assert "520" in reasons["wide"][1] and "512" in reasons["wide"][1]
    assert "member 1" in reasons["head"][1] and "head width 2" in reasons["head"][1]
    assert "65" in reasons["count"][1] and "64" in reasons["count"][1]
    assert "member 1" in reasons["family"][1] and "WideDeep" in reasons["family"][1]
    assert len({why for _, why in reasons.values()}) == len(reasons)
    for bad in ([_model(30, [8], ["tanh"]), _model(31, [8], ["tanh"])], []):
        with pytest.raises(ValueError):
            pack_ensemble(bad)
    # a member that fits alone but not beside the ensemble's widest buffers
    big = ShifuMLP(264, [96, 96], ["tanh", "relu"])
    wide = ShifuMLP(264, [16, 128], ["tanh", "tanh"])
    assert ensemble_eligible([big])[0] and ensemble_eligible([wide])[0]
    ok, why = ensemble_eligible([big, wide])
    assert not ok and "member 0" in why and "LDS" in why


@pytest.mark.parametrize("budget", [LDS_LIMIT, 52000])
def test_emulation_is_the_ordered_fp32_mean(budget):
    models = _hetero()
    x = torch.randn(259, 37, generator=torch.Generator().manual_seed(3))
    packed = pack_ensemble(models, max_group_bytes=budget)
    cols = [fused_predict(pack_mlp(m), x) for m in models]
    mean = fused_ensemble_predict(packed, x)
    assert mean.dtype == torch.float32 and mean.shape == (259,)
    assert torch.equal(mean, _sum_scale(cols))
    mean2, members = fused_ensemble_predict(packed, x, return_members=True)
    assert torch.equal(mean2, mean)
    assert members.shape == (259, 3) and members.dtype == torch.float32
    for i, c in enumerate(cols):
        assert torch.equal(members[:, i], c)
    assert min(c.std().item() for c in cols) >= 0.02
    with pytest.raises(ValueError):
        fused_ensemble_predict(packed, torch.zeros(3, 36))


def test_single_member_is_fused_predict():
    model = _model(37, [33, 17, 5], ["tanh", "relu", "sigmoid"])
    x = torch.randn(40, 37, generator=torch.Generator().manual_seed(4))
    want = fused_predict(pack_mlp(model), x)
    mean, members = fused_ensemble_predict(pack_ensemble([model]), x,
                                           return_members=True)
    assert torch.equal(mean, want) and torch.equal(members[:, 0], want)


def test_ensemble_model_layer_path():
    models = _hetero()
    x = torch.randn(50, 37, generator=torch.Generator().manual_seed(5))
    ens = EnsembleModel(models)
    cols = [m.predict(x).float() for m in models]
    assert torch.equal(ens.predict(x), _sum_scale(cols))
    assert torch.equal(ens.predict_members(x), torch.stack(cols, dim=1))
    with pytest.raises(ValueError):
        EnsembleModel([models[0], _model(36, [7], ["tanh"])])
    with pytest.raises(ValueError):
        EnsembleModel([models[0], WideDeep(37, [50], 4, [16], ["relu"])])
    with pytest.raises(ValueError):
        EnsembleModel([])


def test_end_to_end_export_load_score(tmp_path):
    models = _hetero()
    mdir = str(tmp_path / "bag")
    export_ensemble(models, mdir)
    with open(os.path.join(mdir, "ensemble.json")) as f:
        assert json.load(f) == {"family": "ensemble", "combine": "mean",
                                "members": ["model0", "model1", "model2"]}
    for i in range(3):
        assert os.path.exists(os.path.join(mdir, f"model{i}", "graph.json"))
    with open(os.path.join(mdir, "GenericModelConfig.json")) as f:
        gmc = json.load(f)
    assert gmc["inputnames"] == ["shifu_input_0"]
    assert gmc["outputnames"] == ["shifu_output_0"]
    assert gmc["properties"]["normtype"] == "ZSCALE"
    assert gmc["modelpath"] == os.path.abspath(mdir)

    x = torch.randn(40, 37, generator=torch.Generator().manual_seed(6))
    ens = EnsembleModel(models)
    want = ens.predict(x)
    want_members = ens.predict_members(x)

    loaded = load_exported(mdir)
    assert isinstance(loaded, EnsembleModel) and len(loaded.members) == 3
    assert not hasattr(loaded, "_fused_packed")
    assert torch.equal(loaded.predict(x), want)
    assert torch.equal(load_exported_ensemble(mdir).predict(x), want)

    sc = ShifuScorer()
    sc.init(os.path.join(mdir, "GenericModelConfig.json"))
    assert sc.num_dense == 37 and sc.num_cat == 0 and sc.num_members == 3
    assert np.array_equal(sc.compute_batch(x.numpy()), want.numpy())
    p, mem = sc.compute_batch(x.numpy(), return_members=True)
    assert np.array_equal(p, want.numpy())
    assert np.array_equal(mem, want_members.numpy())
    # one row at a time: a CPU fp32 GEMM may sum in another order at B = 1
    # than at B = 40, a few ulp of a score (6e-8 each), hence ROW_TOL
    for i in (0, 7, 39):
        assert abs(sc.compute(x[i].tolist()) - float(want[i])) <= ROW_TOL
        got = sc.compute_members(x[i].tolist())
        assert len(got) == 3
        assert np.abs(np.array(got) - want_members[i].numpy()).max() <= ROW_TOL

    # fused: the same bundle through the single-kernel path (CPU emulation)
    fwant, fmem = fused_ensemble_predict(pack_ensemble(models), x,
                                         return_members=True)
    for mode in (True, "auto"):
        on = load_exported(mdir, fused=mode)
        assert torch.equal(on.predict(x), fwant)
        assert torch.equal(on.predict_members(x), fmem)
    fs = ShifuScorer()
    fs.init(os.path.join(mdir, "GenericModelConfig.json"), fused=True)
    p, mem = fs.compute_batch(x.numpy(), return_members=True)
    assert np.array_equal(p, fwant.numpy()) and np.array_equal(mem, fmem.numpy())
    assert abs(fs.compute(x[3].tolist()) - float(fwant[3])) <= ROW_TOL
    assert np.abs(np.array(fs.compute_members(x[3].tolist()))
                  - fmem[3].numpy()).max() <= ROW_TOL
    with pytest.raises(ValueError):
        load_exported(mdir, fused="yes")

    # a config file that sits beside ensemble.json but names a stale modelpath
    gmc["modelpath"] = str(tmp_path / "moved-away")
    with open(os.path.join(mdir, "GenericModelConfig.json"), "w") as f:
        json.dump(gmc, f)
    beside = ShifuScorer()
    beside.init(os.path.join(mdir, "GenericModelConfig.json"))
    assert beside.num_members == 3
    assert np.array_equal(beside.compute_batch(x.numpy()), want.numpy())

    # a single bundle still scores as before, as its own only member
    one = ShifuScorer()
    one.init(os.path.join(mdir, "model1", "GenericModelConfig.json"))
    assert one.num_members == 1
    p, mem = one.compute_batch(x.numpy(), return_members=True)
    assert np.array_equal(p, models[1].predict(x).numpy())
    assert mem.shape == (40, 1) and np.array_equal(mem[:, 0], p)


def test_wide_deep_member_keeps_the_layer_path(tmp_path):
    members = [WideDeep(8, [50, 50], 4, [16], ["relu"], seed=3 + i)
               for i in range(2)]
    mdir = str(tmp_path / "wd")
    export_ensemble(members, mdir)
    d = torch.randn(6, 8, generator=torch.Generator().manual_seed(1))
    c = torch.randint(0, 50, (6, 2), generator=torch.Generator().manual_seed(2))
    want = EnsembleModel(members).predict(d, c)
    auto = load_exported(mdir, fused="auto")
    assert not hasattr(auto, "_fused_packed")
    assert torch.equal(auto.predict(d, c), want)
    with pytest.raises(ValueError, match="WideDeep"):
        load_exported(mdir, fused=True)
    sc = ShifuScorer()
    sc.init(os.path.join(mdir, "GenericModelConfig.json"), fused="auto")
    assert sc.num_dense == 8 and sc.num_cat == 2 and sc.num_members == 2
    assert np.array_equal(sc.compute_batch(d.numpy(), c.numpy()), want.numpy())
    row = d[2].tolist() + [float(v) for v in c[2]]
    assert abs(sc.compute(row) - float(want[2])) <= ROW_TOL
    with pytest.raises(ValueError, match="WideDeep"):
        ShifuScorer().init(os.path.join(mdir, "GenericModelConfig.json"),
                           fused=True)


def test_score_cli_on_an_ensemble_directory(tmp_path):
    models = _same(20, 3)
    mdir = str(tmp_path / "bag")
    export_ensemble(models, mdir)
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((300, 20)).astype(np.float32)
    data = tmp_path / "part-0.csv"
    data.write_text("\n".join("|".join(f"{v:.6f}" for v in r) for r in rows) + "\n")
    # what the CLI sees: the rows after the %.6f round trip through the csv
    from shifu_amd.io import load_csv_native
    x = torch.from_numpy(load_csv_native(
        [str(data)], list(range(20)), [], target_column=-1, weight_column=-1,
        delimiter="|").dense)

    def run(*extra):
        out = tmp_path / ("scores" + "".join(extra) + ".csv")
        r = subprocess.run(
            [sys.executable, "-m", "shifu_amd.score", "--model", mdir,
             "--data", str(data), "--output", str(out), "--device", "cpu",
             *extra],
            capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        assert json.loads(r.stderr.strip().splitlines()[-1])["rows"] == 300
        return out.read_text().splitlines()

    def parse(lines, ncol):
        assert len(lines) == 300
        out = np.empty((300, ncol))
        for i, line in enumerate(lines):
            parts = line.split("|")
            assert len(parts) == ncol
            for p in parts:                      # the .6f format is unchanged
                assert len(p.split(".")[1]) == 6
            out[i] = [float(p) for p in parts]
        return out

    ens = EnsembleModel(models)
    want = ens.predict(x).double().numpy()
    wantm = ens.predict_members(x).double().numpy()
    plain = parse(run(), 1)                    # one score per row, as before
    assert np.abs(plain[:, 0] - want).max() <= PRINT_TOL
    assert plain[:, 0].std() >= 0.02
    withm = parse(run("--member-scores"), 1 + 3)
    assert np.array_equal(withm[:, 0], plain[:, 0])
    assert np.abs(withm[:, 1:] - wantm).max() <= PRINT_TOL
    assert wantm.std(axis=0).min() >= 0.02

    fused = parse(run("--fused", "on", "--member-scores"), 1 + 3)
    fwant, fmem = fused_ensemble_predict(pack_ensemble(models), x,
                                         return_members=True)
    assert np.abs(fused[:, 0] - fwant.double().numpy()).max() <= PRINT_TOL
    assert np.abs(fused[:, 1:] - fmem.double().numpy()).max() <= PRINT_TOL
    # the fused path rounds to bf16, so it is a different set of numbers
    assert not np.array_equal(fused, withm)


def test_server_scores_an_ensemble(tmp_path):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from shifu_amd.server import create_app

    models = _hetero()
    mdir = str(tmp_path / "bag")
    export_ensemble(models, mdir)
    client = TestClient(create_app(mdir))
    h = client.get("/health").json()
    assert h["status"] == "ok" and h["num_dense"] == 37 and h["num_cat"] == 0
    assert h["members"] == 3
    x = torch.randn(5, 37, generator=torch.Generator().manual_seed(8))
    r = client.post("/score", json={"rows": x.tolist()}).json()
    want = EnsembleModel(models).predict(x)
    assert len(r["scores"]) == 5
    assert np.abs(np.array(r["scores"]) - want.numpy()).max() <= ROW_TOL


def test_server_health_reports_one_member_for_a_single_bundle(tmp_path):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from shifu_amd.server import create_app
    from shifu_amd.train.export import export_model

    export_model(_model(5, [7], ["tanh"]), str(tmp_path / "one"))
    h = TestClient(create_app(str(tmp_path / "one"))).get("/health").json()
    assert h["members"] == 1 and h["num_dense"] == 5


def test_bagging_num_round_trips():
    assert ModelConfig.from_dict({}).bagging_num == 1
    mc = ModelConfig.from_dict({"train": {"baggingNum": 5}})
    assert mc.bagging_num == 5
    d = mc.to_dict()
    assert d["train"]["baggingNum"] == 5
    assert ModelConfig.from_dict(d).bagging_num == 5
    assert ModelConfig.from_dict(ModelConfig().to_dict()).bagging_num == 1
