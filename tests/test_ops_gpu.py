"""HIP kernel numerics vs plain PyTorch fp32 references (run on MI355X).

Every test feeds the SAME bf16-rounded inputs to the HIP kernel and to a
fp32 torch reference; tolerances cover only the output-side bf16 rounding
(kernels accumulate fp32).  Transpose-detecting inputs (asymmetric, distinct
scales) per the CDNA4 guide's G9/G16 rules."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from shifu_amd.ops.dispatch import hip_available, hip_ops


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    assert torch.cuda.is_available(), "GPU test requires a GPU"
    assert hip_available(), "HIP extension must be built (native code not loaded!)"


def _rand_bf16(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.randn(*shape, generator=g) * scale
    return t.to(torch.bfloat16).cuda()


def _rel_close(a, b, tol=2e-2):
    a, b = a.float().cpu(), b.float().cpu()
    denom = b.abs().max().clamp_min(1e-3)
    return bool(((a - b).abs().max() / denom) < tol), float((a - b).abs().max())


def test_mfma_probe_fragment_mapping():
    """Single 16x16x32 MFMA against torch.matmul — catches any wrong A/B/D
    lane mapping immediately (asymmetric inputs)."""
    a = _rand_bf16(16, 32, seed=1)
    b = _rand_bf16(32, 16, seed=2)
    d = hip_ops().mfma_probe(a, b)
    ref = a.float() @ b.float()
    ok, err = _rel_close(d, ref, 1e-3)
    assert ok, f"MFMA fragment mapping wrong, maxdiff={err}\n{d[:4,:4]}\nvs\n{ref[:4,:4]}"


@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (256, 512, 200), (100, 1, 37),
                                   (1000, 256, 513), (64, 64, 64)])
def test_gemm_nn(M, N, K):
    a = _rand_bf16(M, K, seed=M + 1)
    b = _rand_bf16(K, N, seed=N + 2)
    c = hip_ops().gemm_nn_bf16(a, b)
    ref = a.float() @ b.float()
    ok, err = _rel_close(c, ref)
    assert ok, f"gemm_nn {M}x{N}x{K} maxdiff={err}"


@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_linear_act_fwd(act):
    x = _rand_bf16(300, 150, seed=5)
    w = _rand_bf16(150, 70, seed=6, scale=0.3)
    b = _rand_bf16(70, seed=7)
    y = hip_ops().linear_act_fwd(x, w, b, act)
    z = x.float() @ w.float() + b.float()
    acts = {0: lambda t: t, 1: torch.sigmoid, 2: torch.tanh, 3: torch.relu,
            4: lambda t: torch.nn.functional.leaky_relu(t, 0.01)}
    ok, err = _rel_close(y, acts[act](z))
    assert ok, f"linear_act_fwd act={act} maxdiff={err}"


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 96, 200), (8192, 1024, 1864),
                                   (100, 1, 37), (513, 250, 129)])
def test_gemm_ntv3(M, N, K):
    """v3 fast-path GEMM (glds + swizzle): C = A @ B^T, transpose-detecting."""
    a = _rand_bf16(M, K, seed=M + 3)
    b = _rand_bf16(N, K, seed=N + 4)
    c = hip_ops().gemm_ntv3_bf16(a, b)
    ok, err = _rel_close(c, a.float() @ b.float().t())
    assert ok, f"gemm_ntv3 {M}x{N}x{K} maxdiff={err}"


@pytest.mark.parametrize("M,N,K", [(512, 256, 256), (512, 512, 1864),
                                   (4096, 4096, 4096), (8192, 256, 512),
                                   (600, 300, 777)])
def test_gemm_nt_v4_shapes(M, N, K):
    """256x256 deep-pipelined kernel (v4 route), incl. K-edge + M/N-edge tiles."""
    a = _rand_bf16(M, K, seed=M + 11)
    b = _rand_bf16(N, K, seed=N + 12)
    c = hip_ops().gemm_ntv3_bf16(a, b)
    ok, err = _rel_close(c, a.float() @ b.float().t())
    assert ok, f"v4 {M}x{N}x{K} maxdiff={err}"


def test_gemm_nt_v4_race_screen():
    """The v4 pipeline uses counted vmcnt across raw barriers — a wrong count
    is a data race.  Non-splitk runs must be bitwise-identical across
    repeats."""
    a = _rand_bf16(1024, 512, seed=90)
    b = _rand_bf16(512, 512, seed=91)
    first = hip_ops().gemm_ntv3_bf16(a, b)
    for _ in range(5):
        again = hip_ops().gemm_ntv3_bf16(a, b)
        assert torch.equal(first, again), "v4 nondeterminism: race in pipeline"


def test_gemm_ntv3_f32_splitk():
    a = _rand_bf16(1024, 8192, seed=50, scale=0.5)   # dzT [N,B]
    b = _rand_bf16(1864, 8192, seed=51, scale=0.5)   # xT [K,B]
    c = hip_ops().gemm_ntv3_f32(a, b)
    assert c.dtype == torch.float32
    ok, err = _rel_close(c, a.float() @ b.float().t())
    assert ok, f"ntv3 splitk maxdiff={err}"


@pytest.mark.parametrize("act", [0, 1, 3])
def test_linear_nt_fwd(act):
    x = _rand_bf16(300, 150, seed=60)
    w = _rand_bf16(70, 150, seed=61, scale=0.3)   # [out, in]
    b = _rand_bf16(70, seed=62)
    y = hip_ops().linear_nt_fwd(x, w, b, act)
    z = x.float() @ w.float().t() + b.float()
    acts = {0: lambda t: t, 1: torch.sigmoid, 3: torch.relu}
    ok, err = _rel_close(y, acts[act](z))
    assert ok, f"linear_nt_fwd act={act} maxdiff={err}"


@pytest.mark.parametrize("R,C", [(64, 64), (8192, 1864), (100, 37), (513, 1)])
def test_transpose_bf16(R, C):
    t = _rand_bf16(R, C, seed=R + C)
    tt = hip_ops().transpose_bf16(t)
    assert tt.shape == (C, R)
    assert torch.equal(tt.float().cpu(), t.float().t().cpu())


@pytest.mark.parametrize("act", [0, 1])
def test_gemv_head_path(act):
    """1-unit head GEMV fwd/bwd vs reference (the shifu_output_0 shape)."""
    x = _rand_bf16(1000, 37, seed=70)
    w = _rand_bf16(1, 37, seed=71, scale=0.3)
    b = _rand_bf16(1, seed=72)
    y = hip_ops().gemv_fwd(x, w, b, act)
    z = x.float() @ w.float().t() + b.float()
    ref_y = torch.sigmoid(z) if act == 1 else z
    ok, err = _rel_close(y, ref_y)
    assert ok, f"gemv_fwd maxdiff={err}"

    dz = _rand_bf16(1000, seed=73)
    dw, db, dx = hip_ops().gemv_bwd(x, w.reshape(-1), dz, True)
    ok, err = _rel_close(dw, (dz.float().reshape(1, -1) @ x.float()))
    assert ok, f"gemv dw maxdiff={err}"
    assert abs(float(db) - float(dz.float().sum())) < 0.05 * max(abs(float(dz.float().sum())), 1)
    ok, err = _rel_close(dx, dz.float().reshape(-1, 1) @ w.float())
    assert ok, f"gemv dx maxdiff={err}"


def test_fused_linear_head_autograd_gpu():
    """FusedLinear with out_features=1 routes through GEMV; compare vs CPU."""
    from shifu_amd.ops.linear import fused_linear
    torch.manual_seed(2)
    x32 = torch.randn(512, 64)
    w32 = torch.randn(1, 64) * 0.2
    b32 = torch.randn(1) * 0.1
    xc = x32.clone().requires_grad_(True)
    wc = w32.clone().requires_grad_(True)
    bc = b32.clone().requires_grad_(True)
    fused_linear(xc, wc, bc, "none").pow(2).sum().backward()
    xg = x32.to(torch.bfloat16).cuda().requires_grad_(True)
    wg = w32.clone().cuda().requires_grad_(True)
    bg = b32.clone().cuda().requires_grad_(True)
    fused_linear(xg, wg, bg, "none").float().pow(2).sum().backward()
    for got, want, name in [(wg.grad, wc.grad, "dw"), (bg.grad, bc.grad, "db"),
                            (xg.grad, xc.grad, "dx")]:
        rel = float((got.float().cpu() - want).abs().max() /
                    want.abs().max().clamp_min(1e-3))
        assert rel < 0.08, f"{name} rel {rel}"


@pytest.mark.parametrize("R,M,N", [(64, 128, 128), (512, 256, 384),
                                   (16384, 1024, 1864), (200, 100, 130),
                                   (1000, 37, 64)])
def test_gemm_tt_wgrad(R, M, N):
    """Transpose-free wgrad (hardware tr_b16 reads): dw = dz^T @ x."""
    dz = _rand_bf16(R, M, seed=R + 21, scale=0.5)
    x = _rand_bf16(R, N, seed=N + 22, scale=0.5)
    c = hip_ops().gemm_tt_f32(dz, x)
    ok, err = _rel_close(c, dz.float().t() @ x.float())
    assert ok, f"gemm_tt {R}x{M}x{N} maxdiff={err}"


@pytest.mark.parametrize("R,M,N", [(64, 128, 128), (512, 256, 384),
                                   (16384, 1024, 1864), (200, 104, 136),
                                   (1000, 40, 64), (32768, 512, 464)])
def test_gemm_ttv3_wgrad(R, M, N):
    """ttv3 transpose-free wgrad (scatter-staged v3 image): dw = dz^T @ x,
    fresh-output and accumulate-into variants (deterministic slab split-K)."""
    dz = _rand_bf16(R, M, seed=R + 31, scale=0.5)
    x = _rand_bf16(R, N, seed=N + 32, scale=0.5)
    want = dz.float().t() @ x.float()
    c = hip_ops().gemm_ttv3_f32(dz, x)
    ok, err = _rel_close(c, want)
    assert ok, f"gemm_ttv3 {R}x{M}x{N} maxdiff={err}"
    # into-variant accumulates
    base = torch.randn(M, N, device="cuda") * 0.1
    out = base.clone()
    hip_ops().gemm_ttv3_f32_into(dz, x, out)
    ok, err = _rel_close(out, base + want)
    assert ok, f"gemm_ttv3_into {R}x{M}x{N} maxdiff={err}"
    # bitwise deterministic across runs (slab split-K, no f32 atomics)
    c2 = hip_ops().gemm_ttv3_f32(dz, x)
    assert torch.equal(c, c2)


def test_wgrad_tt_route_matches_default():
    """SHIFU_WGRAD_TT=1 routing in linear.py (ttv3 + colsum-into) must
    produce the same grads as the default transpose+NT route."""
    import shifu_amd.ops.linear as lin
    from shifu_amd.ops.linear import fused_linear

    def grads(tt):
        old = lin._WGRAD_TT
        lin._WGRAD_TT = tt
        try:
            torch.manual_seed(4)
            x = torch.randn(512, 128).to(torch.bfloat16).cuda().requires_grad_(True)
            w = torch.randn(64, 128).cuda().requires_grad_(True)
            b = torch.zeros(64).cuda().requires_grad_(True)
            fused_linear(x, w, b, "relu").float().pow(2).sum().backward()
            return w.grad.clone(), b.grad.clone(), x.grad.clone()
        finally:
            lin._WGRAD_TT = old
    dw1, db1, dx1 = grads(True)
    dw0, db0, dx0 = grads(False)
    assert torch.equal(dx1, dx0), "dx diverged"
    ok, err = _rel_close(dw1, dw0.float(), 1e-2)
    assert ok, f"dw tt-vs-default maxdiff={err}"
    ok, err = _rel_close(db1, db0.float(), 1e-2)
    assert ok, f"db tt-vs-default maxdiff={err}"


def test_gemv_bwd_deterministic():
    """Head wgrad (slab reduce, no atomics): bitwise repeatable and matches
    the fp32 reference, for both vector (K%8==0) and odd-K paths."""
    ext = hip_ops()
    for K in (256, 130):
        x = _rand_bf16(4096, K, seed=K)
        w = _rand_bf16(1, K, seed=K + 1).reshape(-1)
        dz = _rand_bf16(4096, 1, seed=K + 2).reshape(-1)
        dw, db, dx = ext.gemv_bwd(x, w, dz, True)
        dw2, db2, _ = ext.gemv_bwd(x, w, dz, True)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), f"K={K} nondet"
        ref_dw = (dz.float().unsqueeze(0) @ x.float()).reshape(-1)
        ok, err = _rel_close(dw.reshape(-1), ref_dw)
        assert ok, f"K={K} dw maxdiff={err}"
        ok, err = _rel_close(db, dz.float().sum().reshape(1))
        assert ok, f"K={K} db maxdiff={err}"
        ok, err = _rel_close(dx, dz.float().unsqueeze(1) * w.float().unsqueeze(0))
        assert ok, f"K={K} dx maxdiff={err}"


def test_act_grad_colsum_into():
    """dzT-free partner of ttv3: dz = dy*act'(y), db ACCUMULATED into view."""
    torch.manual_seed(5)
    dy = _rand_bf16(700, 96, seed=51)
    y = torch.rand(700, 96, device="cuda").to(torch.bfloat16)  # in (0,1)
    base = torch.randn(96, device="cuda")
    db = base.clone()
    dz = hip_ops().act_grad_colsum_into(dy, y, 1, db)  # sigmoid
    want_dz = dy.float() * y.float() * (1 - y.float())
    ok, err = _rel_close(dz, want_dz)
    assert ok, f"act_grad_colsum_into dz maxdiff={err}"
    ok, err = _rel_close(db, base + want_dz.sum(0))
    assert ok, f"act_grad_colsum_into db maxdiff={err}"


def test_gemm_nt():
    dz = _rand_bf16(320, 96, seed=8)
    w = _rand_bf16(130, 96, seed=9)
    dx = hip_ops().gemm_nt_bf16(dz, w)
    ok, err = _rel_close(dx, dz.float() @ w.float().t())
    assert ok, f"gemm_nt maxdiff={err}"


def test_gemm_tn():
    x = _rand_bf16(513, 130, seed=10)
    dz = _rand_bf16(513, 96, seed=11)
    dw = hip_ops().gemm_tn_f32(x, dz)
    assert dw.dtype == torch.float32
    ok, err = _rel_close(dw, x.float().t() @ dz.float())
    assert ok, f"gemm_tn maxdiff={err}"


def test_gemm_tn_splitk_large_batch():
    """wgrad shape from the bench (B=8192 reduction) — exercises the split-K
    atomic path."""
    x = _rand_bf16(8192, 130, seed=30, scale=0.5)
    dz = _rand_bf16(8192, 96, seed=31, scale=0.5)
    dw = hip_ops().gemm_tn_f32(x, dz)
    ok, err = _rel_close(dw, x.float().t() @ dz.float())
    assert ok, f"gemm_tn splitk maxdiff={err}"


def test_act_grad_colsum_fused():
    dy = _rand_bf16(1000, 96, seed=40)
    y = torch.sigmoid(_rand_bf16(1000, 96, seed=41).float()).to(torch.bfloat16)
    dz, db = hip_ops().act_grad_colsum(dy, y, 1)
    ref_dz = dy.float() * y.float() * (1 - y.float())
    ok, err = _rel_close(dz, ref_dz)
    assert ok, f"fused act_grad maxdiff={err}"
    # db accumulates UNROUNDED f32 terms (more accurate than summing bf16 dz)
    ok, err = _rel_close(db, ref_dz.sum(0), 1e-2)
    assert ok, f"fused colsum maxdiff={err}"


def test_act_grad_and_colsum():
    dy = _rand_bf16(64, 33, seed=12)
    y = torch.sigmoid(_rand_bf16(64, 33, seed=13).float()).to(torch.bfloat16)
    dz = hip_ops().act_grad(dy, y, 1)
    ref = dy.float() * y.float() * (1 - y.float())
    ok, err = _rel_close(dz, ref)
    assert ok, f"act_grad maxdiff={err}"

    db = hip_ops().colsum_f32(dz.reshape(64, 33).contiguous())
    ok, err = _rel_close(db, dz.float().sum(0), 1e-3)
    assert ok, f"colsum maxdiff={err}"


@pytest.mark.parametrize("kind", [0, 1])
def test_weighted_loss(kind):
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(1000, generator=g)).to(torch.bfloat16).cuda()
    y = (torch.rand(1000, generator=g) > 0.5).float().cuda()
    w = (torch.rand(1000, generator=g) * 2).cuda()
    p, ls, ws = hip_ops().weighted_loss_fwd(z, y, w, kind)
    zf = z.float()
    pref = torch.sigmoid(zf)
    if kind == 0:
        per = w * (pref - y) ** 2
    else:
        per = w * torch.nn.functional.binary_cross_entropy_with_logits(zf, y, reduction="none")
    assert torch.allclose(p, pref, atol=1e-5)
    assert abs(float(ls) - float(per.sum())) < 1e-2 * max(float(per.sum()), 1.0)
    nnz = float((w != 0).sum())  # TF SUM_BY_NONZERO_WEIGHTS count
    assert abs(float(ws) - nnz) < 1e-3 * nnz

    dz = hip_ops().weighted_loss_bwd(p, y, w, kind,
                                     torch.tensor([0.125], device="cuda"))
    if kind == 0:
        ref = w * 2 * (pref - y) * pref * (1 - pref) * 0.125
    else:
        ref = w * (pref - y) * 0.125
    ok, err = _rel_close(dz, ref, 3e-2)
    assert ok, f"loss_bwd maxdiff={err}"


@pytest.mark.parametrize("opt", ["sgd", "adam", "adadelta", "adagrad"])
def test_fused_optimizers_gpu(opt):
    from shifu_amd.ops.flat import FlatParams
    from shifu_amd.ops.optim import FusedOptimizer
    torch.manual_seed(0)
    w0 = torch.randn(10000)

    # CPU reference run
    p_cpu = torch.nn.Parameter(w0.clone())
    flat_cpu = FlatParams([p_cpu])
    o_cpu = FusedOptimizer(flat_cpu, [], optimizer=opt, lr=0.1, l2_reg=0.01)

    p_gpu = torch.nn.Parameter(w0.clone().cuda())
    flat_gpu = FlatParams([p_gpu])
    o_gpu = FusedOptimizer(flat_gpu, [], optimizer=opt, lr=0.1, l2_reg=0.01)

    for step in range(5):
        g = torch.randn(10000, generator=torch.Generator().manual_seed(step))
        flat_cpu.flat_grad.copy_(g)
        o_cpu.step()
        flat_gpu.flat_grad.copy_(g.cuda())
        o_gpu.step()
    assert torch.allclose(flat_gpu.flat.cpu(), flat_cpu.flat, atol=1e-4), \
        f"{opt}: maxdiff={float((flat_gpu.flat.cpu()-flat_cpu.flat).abs().max())}"


def test_embedding_gather_gpu():
    arena = _rand_bf16(500, 64, seed=20)
    ids = torch.randint(0, 500, (37, 4)).cuda()
    out = hip_ops().embedding_gather(arena, ids)
    ref = arena.float().index_select(0, ids.reshape(-1)).reshape(37, 4 * 64)
    assert torch.allclose(out.float(), ref, atol=1e-6)
    # D % 8 != 0 (scalar path; D=6 is even -- odd D is covered in
    # test_embedding_kernels_gpu.py)
    arena2 = _rand_bf16(100, 6, seed=21)
    out2 = hip_ops().embedding_gather(arena2, ids % 100)
    ref2 = arena2.float().index_select(0, (ids % 100).reshape(-1)).reshape(37, 4 * 6)
    assert torch.allclose(out2.float(), ref2, atol=1e-6)


def test_emb_updates_gpu():
    torch.manual_seed(1)
    arena = torch.randn(200, 32).to(torch.bfloat16).cuda()
    ref = arena.float().cpu().clone()
    rows = torch.tensor([3, 77, 150]).cuda()
    vals = torch.randn(3, 32).to(torch.bfloat16).cuda()
    hip_ops().emb_sgd_step(arena, rows, vals, 0.5)
    ref[rows.cpu()] -= 0.5 * vals.float().cpu()
    assert torch.allclose(arena.float().cpu(), ref, atol=1e-2)

    acc = torch.zeros(200).cuda()
    arena2 = torch.randn(200, 32).to(torch.bfloat16).cuda()
    ref2 = arena2.float().cpu().clone()
    hip_ops().emb_adagrad_step(arena2, acc, rows, vals, 0.1, 1e-8)
    vf = vals.float()
    rowsq = (vf * vf).mean(dim=1)
    denom = (rowsq.sqrt() + 1e-8).unsqueeze(1)
    ref2[rows.cpu()] -= (0.1 * vf / denom).cpu()
    assert torch.allclose(arena2.float().cpu(), ref2, atol=1e-2)
    assert torch.allclose(acc[rows].cpu(), rowsq.cpu(), atol=1e-5)


def test_fused_linear_autograd_gpu_vs_cpu():
    """Full autograd path through the HIP kernels vs the CPU reference path."""
    from shifu_amd.ops.linear import fused_linear
    torch.manual_seed(0)
    x32 = torch.randn(256, 96)
    w32 = torch.randn(48, 96) * 0.2   # [out, in]
    b32 = torch.randn(48) * 0.1

    # CPU reference
    xc = x32.clone().requires_grad_(True)
    wc = w32.clone().requires_grad_(True)
    bc = b32.clone().requires_grad_(True)
    yc = fused_linear(xc, wc, bc, "relu")
    yc.pow(2).sum().backward()

    # GPU HIP path (bf16 compute)
    xg = x32.to(torch.bfloat16).cuda().requires_grad_(True)
    wg = w32.clone().cuda().requires_grad_(True)
    bg = b32.clone().cuda().requires_grad_(True)
    yg = fused_linear(xg, wg, bg, "relu")
    yg.float().pow(2).sum().backward()

    for got, want, name, tol in [(yg, yc, "y", 3e-2),
                                 (wg.grad, wc.grad, "dw", 8e-2),
                                 (bg.grad, bc.grad, "db", 8e-2),
                                 (xg.grad, xc.grad, "dx", 8e-2)]:
        gotf, wantf = got.float().cpu(), want.float().cpu()
        denom = wantf.abs().max().clamp_min(1e-3)
        rel = float((gotf - wantf).abs().max() / denom)
        assert rel < tol, f"{name} rel diff {rel}"


def test_train_step_gpu_learns():
    """End-to-end: a WideDeep step on GPU decreases loss (native path)."""
    from shifu_amd.config.model_config import ModelConfig
    from shifu_amd.config.run_config import RunConfig
    from shifu_amd.data.csv_loader import TabularDataset
    from shifu_amd.data.synthetic import synthetic_arrays
    from shifu_amd.models.wide_deep import WideDeep
    from shifu_amd.train.trainer import Trainer
    dense, cats, target, weight = synthetic_arrays(4096, 16, (1000, 1000), seed=5)
    full = TabularDataset(dense, cats, target, weight)
    train, valid = full.split(0.2, seed=1)
    mc = ModelConfig.from_dict({"train": {"numTrainEpochs": 3, "params": {
        "NumHiddenLayers": 2, "NumHiddenNodes": [64, 32],
        "ActivationFunc": ["relu", "relu"], "LearningRate": 0.01,
        "Optimizer": "adam", "Loss": "sigmoid_ce", "MiniBatchSize": 512,
        "L2Reg": 0.0}}})
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        rc = RunConfig(tmp_model_path=td + "/ckpt", final_model_path=td + "/final")
        model = WideDeep(16, [1000, 1000], 16, [64, 32], ["relu", "relu"], seed=2)
        tr = Trainer(model, mc, rc, train, valid, device=torch.device("cuda"))
        first = tr.evaluate(tr.valid_data)
        tr.fit()
        last = tr.evaluate(tr.valid_data)
        assert last["loss"] < first["loss"], f"{first} -> {last}"
        assert last["auc"] > 0.55


def test_fm2_fused_gpu():
    """Fused FM interaction kernels vs fp32 reference."""
    from shifu_amd.ops.fm import fm_second_order
    B, F, D = 512, 26, 64
    emb = _rand_bf16(B, F * D, seed=80, scale=0.2).requires_grad_(True)
    out = fm_second_order(emb, F, D)
    v = emb.detach().float().reshape(B, F, D)
    s = v.sum(dim=1)
    ref = 0.5 * (s * s - (v * v).sum(dim=1)).sum(dim=1)
    ok, err = _rel_close(out, ref)
    assert ok, f"fm2 fwd maxdiff={err}"
    g = torch.randn(B, device="cuda")
    out.backward(g)
    dref = ((s.unsqueeze(1) - v) * g.reshape(B, 1, 1)).reshape(B, F * D)
    ok, err = _rel_close(emb.grad, dref, 4e-2)
    assert ok, f"fm2 bwd maxdiff={err}"


def test_gather_concat_fused():
    """Fused [dense|emb] build == gather + cat, forward and arena grads."""
    from shifu_amd.ops.embedding import MultiEmbedding, gather_concat
    emb = MultiEmbedding([50, 70], dim=8, seed=1)
    emb.cuda()
    emb.arena.data = emb.arena.data.to(torch.bfloat16)
    g = torch.Generator().manual_seed(2)
    ids = torch.stack([torch.randint(0, 50, (64,), generator=g),
                       torch.randint(0, 70, (64,), generator=g)], 1).cuda()
    dense = torch.randn(64, 10, generator=g).to(torch.bfloat16).cuda()

    x1 = gather_concat(emb, ids, dense)
    (x1.float() * torch.arange(x1.numel(), device="cuda").reshape(x1.shape)) \
        .sum().backward()
    from shifu_amd.ops.embedding import sparse_rows_values
    r1, v1 = sparse_rows_values(emb.arena.grad)
    emb.arena.grad = None

    x2 = torch.cat([dense, emb(ids).to(dense.dtype)], dim=1)
    assert torch.equal(x1.float().cpu(), x2.float().cpu())
    (x2.float() * torch.arange(x2.numel(), device="cuda").reshape(x2.shape)) \
        .sum().backward()
    r2, v2 = sparse_rows_values(emb.arena.grad)
    d1 = torch.zeros(120, 8, device="cuda")
    d1.index_add_(0, r1, v1.float())
    d2 = torch.zeros(120, 8, device="cuda")
    d2.index_add_(0, r2, v2.float())
    assert torch.allclose(d1.cpu(), d2.cpu(), atol=1e-2)


def test_splitk_atomic_fallback_mode():
    """SHIFU_SPLITK_SLAB=0 restores the f32-atomic split-K epilogue; it must
    stay numerically correct (the knob is read once per process, hence the
    subprocess)."""
    import os
    import subprocess
    import sys
    code = (
        "import torch\n"
        "from shifu_amd.ops.dispatch import hip_ops\n"
        "ext = hip_ops(); torch.manual_seed(0)\n"
        "for (M, N, K) in [(300, 520, 10000), (512, 1024, 8192)]:\n"
        "    a = torch.randn(M, K, device='cuda').to(torch.bfloat16)\n"
        "    b = torch.randn(N, K, device='cuda').to(torch.bfloat16)\n"
        "    want = a.float() @ b.float().t()\n"
        "    got = ext.gemm_ntv3_f32(a, b)\n"
        "    rel = float((got - want).abs().max() / want.abs().max())\n"
        "    assert rel < 1e-4, (M, N, K, rel)\n"
        "print('ATOMIC_OK')\n"
    )
    env = dict(os.environ, SHIFU_SPLITK_SLAB="0")
    r = subprocess.run([sys.executable, "-c", code], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ATOMIC_OK" in r.stdout


def test_unified_gather_split_gpu():
    """emb_gather_split kernel: deep columns into the concat buffer + wide
    column to its own [B,F], against a plain index_select reference."""
    from shifu_amd.ops.embedding import UnifiedMultiEmbedding
    torch.manual_seed(4)
    emb = UnifiedMultiEmbedding([500, 300, 200], dim=16, seed=9,
                                dtype=torch.bfloat16).cuda()
    B, nd = 257, 12
    g = torch.Generator().manual_seed(1)
    ids = torch.stack([torch.randint(0, v, (B,), generator=g)
                       for v in [500, 300, 200]], dim=1).cuda()
    dense = torch.randn(B, nd, generator=g).to(torch.bfloat16).cuda()
    out, wide = emb.gather_split(ids, dense)

    flat = emb.flat_ids(ids).reshape(-1)
    ref = emb.arena.detach().index_select(0, flat).reshape(B, 3, emb.cols)
    assert torch.equal(out[:, nd:].reshape(B, 3, 16), ref[:, :, :16])
    assert torch.equal(wide, ref[:, :, 16])
    assert torch.equal(out[:, :nd], dense)


def test_unified_wide_deep_step_gpu():
    """Full unified Wide&Deep training step on the HIP path: loss finite,
    arena rows move, pad column stays zero."""
    from shifu_amd.models.wide_deep import WideDeep
    from shifu_amd.ops.flat import FlatParams, split_params, bind_mirrors
    from shifu_amd.ops.loss import weighted_loss
    from shifu_amd.ops.optim import FusedOptimizer
    torch.manual_seed(0)
    model = WideDeep(32, [4000] * 4, 16, [64], ["relu"], seed=1,
                     unified=True).cuda()
    for p in model.parameters():
        if getattr(p, "_is_embedding_arena", False):
            p.data = p.data.to(torch.bfloat16)
    dense_params, emb_params = split_params(model)
    flat = FlatParams(dense_params, mirror_bf16=True)
    bind_mirrors(model, flat)
    opt = FusedOptimizer(flat, emb_params, optimizer="adam", lr=1e-3,
                         emb_optimizer="adagrad", emb_lr=0.05)
    g = torch.Generator().manual_seed(2)
    dense = torch.randn(512, 32, generator=g).to(torch.bfloat16).cuda()
    cats = torch.randint(0, 4000, (512, 4), generator=g).cuda()
    y = (torch.rand(512, generator=g) > 0.5).float().cuda()
    w = torch.ones(512, device="cuda")
    arena0 = model.embeddings.arena.data.clone()
    for _ in range(3):
        loss = weighted_loss(model(dense, cats), y, w, "sigmoid_ce")
        loss.backward()
        opt.step()
        opt.zero_grad()
    assert torch.isfinite(loss).all()
    D = model.embed_dim
    a = model.embeddings.arena.data
    assert not torch.equal(a, arena0), "arena never updated"
    assert torch.all(a[:, D + 1].float() == 0), "pad column corrupted"


def test_unified_deferred_matches_packed():
    """The deferred unpacked-grad update path (emb_update_unified) must match
    the packed [n, D+2] sparse path over several adagrad steps."""
    from shifu_amd.models.wide_deep import WideDeep
    from shifu_amd.ops.embedding import UnifiedMultiEmbedding
    from shifu_amd.ops.flat import FlatParams, split_params, bind_mirrors
    from shifu_amd.ops.loss import weighted_loss
    from shifu_amd.ops.optim import FusedOptimizer

    def run(defer):
        torch.manual_seed(0)
        model = WideDeep(16, [2000, 3000], 16, [32], ["relu"], seed=3,
                         unified=True).cuda()
        for p in model.parameters():
            if getattr(p, "_is_embedding_arena", False):
                p.data = p.data.to(torch.bfloat16)
        for m in model.modules():
            if isinstance(m, UnifiedMultiEmbedding):
                m.defer_grads = defer
        dps, eps_ = split_params(model)
        flat = FlatParams(dps, mirror_bf16=True)
        bind_mirrors(model, flat)
        opt = FusedOptimizer(flat, eps_, optimizer="adam", lr=1e-3,
                             emb_optimizer="adagrad", emb_lr=0.05)
        g = torch.Generator().manual_seed(2)
        for _ in range(4):
            dense = torch.randn(256, 16, generator=g).to(torch.bfloat16).cuda()
            cats = torch.stack([torch.randint(0, 2000, (256,), generator=g),
                                torch.randint(0, 3000, (256,), generator=g)],
                               dim=1).cuda()
            y = (torch.rand(256, generator=g) > 0.5).float().cuda()
            loss = weighted_loss(model(dense, cats), y,
                                 torch.ones(256, device="cuda"), "sigmoid_ce")
            loss.backward()
            opt.step()
            opt.zero_grad()
        D = model.embed_dim
        return (model.embeddings.arena.data[:, :D + 1].float().cpu(),
                model.embeddings.adagrad_acc().cpu())

    a1, s1 = run(True)
    a0, s0 = run(False)
    assert torch.allclose(s1, s0, atol=1e-4), "adagrad accumulators diverged"
    assert torch.allclose(a1, a0, atol=2e-2), "arena values diverged"


@pytest.mark.parametrize("R,n,D,adagrad,in_arena", [
    (5000, 8192, 64, True, True),     # bench-like, light dups
    (64, 4096, 64, True, True),       # heavy dups: long chains, multi-chunk
    (300, 2048, 16, True, False),     # external accumulator array
    (300, 2048, 16, False, True),     # sgd mode (no accumulator)
    (2, 4096, 16, False, True),       # bucket > chunk: multi-chunk loop
                                      # (sgd: chunk split has no denominator
                                      # effect, so results still match)
])
def test_emb_update_binned_matches_atomic(R, n, D, adagrad, in_arena):
    """The atomic-free binned unified update must match the atomic
    accsq+scatter chain (same full-step adagrad denominator, f32-accumulated
    values vs per-entry bf16 atomic adds -> small tolerance)."""
    ext = hip_ops()
    DP = D + (4 if in_arena else 2)
    F = 4
    torch.manual_seed(R + D)
    arena = (torch.randn(R, DP, device="cuda") * 0.1).to(torch.bfloat16)
    arena[:, D + 1] = 0  # pad col
    if in_arena:
        arena[:, D + 2:].view(torch.float32).fill_(0.01)
    acc = torch.full((R,), 0.01, device="cuda")
    ids = torch.randint(0, R, (n // F, F), device="cuda")
    rows = ids.reshape(-1)
    dgrad = (torch.randn(n // F, F * D, device="cuda") * 0.1).to(torch.bfloat16)
    wide = (torch.randn(n // F, F, device="cuda") * 0.1).to(torch.bfloat16)

    def run(fn):
        a = arena.clone()
        s = acc.clone()
        fn(a, s, rows, dgrad, 0, wide.reshape(-1), 1, F, 0.05, 1e-8,
           adagrad, in_arena)
        accv = (a[:, D + 2:].view(torch.float32).reshape(-1).clone()
                if in_arena else s)
        return a[:, :D + 1].float(), a[:, D + 1].float(), accv

    va, pada, sa = run(ext.emb_update_unified)
    vb, padb, sb = run(ext.emb_update_unified_binned)
    assert torch.all(pada == 0) and torch.all(padb == 0), "pad corrupted"
    assert torch.allclose(sa, sb, rtol=1e-4, atol=1e-6), \
        f"acc diverged max={float((sa - sb).abs().max())}"
    # thousands of bf16 atomic adds per row accumulate swamping error the
    # f32-summed binned path does not have -> wider tolerance at tiny R
    atol = 0.12 if R < 16 else 3e-2
    assert torch.allclose(va, vb, atol=atol), \
        f"values diverged max={float((va - vb).abs().max())}"
    # rows never touched must be bitwise identical
    touched = torch.zeros(R, dtype=torch.bool, device="cuda")
    touched[rows] = True
    assert torch.equal(va[~touched], vb[~touched])


@pytest.mark.parametrize("B,N,act", [(128, 64, 3), (513, 130, 2), (64, 33, 1),
                                     (1000, 256, 3), (70, 7, 0)])
def test_act_grad_colsum_T(B, N, act):
    """Fused dz + dz^T + colsum against the fp32 reference (edge shapes
    exercise the guarded tile paths)."""
    dy = _rand_bf16(B, N, seed=B + 40)
    y = torch.sigmoid(_rand_bf16(B, N, seed=N + 41).float()).to(torch.bfloat16).cuda()
    dz, dzT, db = hip_ops().act_grad_colsum_T(dy, y, act)
    grads = {0: lambda yy: torch.ones_like(yy), 1: lambda yy: yy * (1 - yy),
             2: lambda yy: 1 - yy * yy, 3: lambda yy: (yy > 0).float()}
    ref = dy.float() * grads[act](y.float())
    ref_b = ref.to(torch.bfloat16).float()
    assert torch.equal(dz.float(), ref_b), "dz mismatch"
    assert torch.equal(dzT.float(), ref_b.t().contiguous()), "dzT mismatch"
    ok, err = _rel_close(db, ref_b.sum(0), 1e-2)
    assert ok, f"db maxdiff={err}"


def test_wgrad_into_gradview_matches_plain():
    """The accumulate-into-flat-grad backward (act_grad_colsum_T_into +
    gemm_ntv3_f32_into) must produce the same dense grads as the plain
    AccumulateGrad route."""
    from shifu_amd.models.mlp import ShifuMLP
    from shifu_amd.ops.flat import FlatParams, split_params, bind_mirrors
    from shifu_amd.ops.loss import weighted_loss

    def grads(bind):
        torch.manual_seed(0)
        model = ShifuMLP(64, [128, 64], ["relu", "tanh"], seed=2).cuda()
        dense_params, _ = split_params(model)
        flat = FlatParams(dense_params, mirror_bf16=True)
        if bind:
            bind_mirrors(model, flat)   # gradviews present -> into-path
        g = torch.Generator().manual_seed(1)
        x = torch.randn(512, 64, generator=g).to(torch.bfloat16).cuda()
        y = (torch.rand(512, generator=g) > 0.5).float().cuda()
        for _ in range(2):   # accumulation across two backwards
            loss = weighted_loss(model(x), y, torch.ones(512, device="cuda"),
                                 "sigmoid_ce")
            loss.backward()
        flat.sync_grads()
        return flat.flat_grad.cpu()

    gi = grads(True)
    gp = grads(False)
    rel = float((gi - gp).abs().max() / gp.abs().max().clamp_min(1e-6))
    assert rel < 5e-3, f"into-path grads diverge: rel {rel}"
