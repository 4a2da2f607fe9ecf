"""Wide-store epilogue of the 256x256 GEMM (gemm_nt_v4_kernel, WIDE) at
shapes that actually reach that kernel (run on MI355X).

The kernel swaps the MFMA operand roles and stages B rows in a permuted
order so that a lane owns 16 contiguous output columns of one row and stores
them as 16-byte chunks.  What can go wrong is therefore a column landing in
the wrong place (permutation, bias mapping), a chunk guard at the M/N edges,
the per-element fallback when rows are not 16-byte aligned, and a wide store
reaching outside the output.  The arithmetic is unchanged, so the closeness
criterion is the one tests/test_ops_gpu.py uses for gemm_ntv3_bf16.

Routes (shifu_ops.hip): gemm_ntv3_bf16 / linear_nt_fwd take the 256x256
kernel when M >= 512, N >= 256, K >= 256 and ceil(M/256)*ceil(N/256) >= 200.
gemm_ntv3_f32_into takes its slab split-K form when z = min(256 // tiles,
ceil(K/64) // 24) > 1 and tiles * z >= 200: at M=3500, N=520/516, K=9224
that is 14*3 = 42 tiles, z = min(6, 145 // 24 = 6) = 6, 252 blocks."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from shifu_amd.ops.dispatch import hip_available, hip_ops


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    assert torch.cuda.is_available(), "GPU test requires a GPU"
    assert hip_available(), "HIP extension must be built (native code not loaded!)"


def _rand_bf16(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randn(*shape, generator=g, device="cuda") * scale
    return t.to(torch.bfloat16)


def _rel_close(a, b, tol=2e-2):
    a, b = a.float().cpu(), b.float().cpu()
    denom = b.abs().max().clamp_min(1e-3)
    return bool(((a - b).abs().max() / denom) < tol), float((a - b).abs().max())


def _tiles(M, N):
    return ((M + 255) // 256) * ((N + 255) // 256)


@pytest.mark.parametrize("M,N,K", [
    (12800, 1024, 256),    # all full tiles: 200 tiles, 4 K-tiles
    (17149, 520, 328),     # every edge: 253-row M tile, 8-col N tile, K tail 8
    (12800, 1864, 320),    # the bench N: 72-col last tile (one chunk in, next out)
    (17149, 515, 264),     # N % 8 != 0: per-element fallback everywhere
])
def test_gemm_wide_epilogue_shapes(M, N, K):
    assert M >= 512 and N >= 256 and K >= 256 and _tiles(M, N) >= 200
    a = _rand_bf16(M, K, seed=M + 11)
    b = _rand_bf16(N, K, seed=N + 12)
    c = hip_ops().gemm_ntv3_bf16(a, b)
    assert c.shape == (M, N) and c.dtype == torch.bfloat16
    ok, err = _rel_close(c, a.float() @ b.float().t())
    assert ok, f"wide epilogue {M}x{N}x{K} maxdiff={err}"


@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_linear_nt_fwd_wide_epilogue_bias(act):
    """Non-zero bias through the per-lane 16-column bias mapping."""
    M, N, K = 17149, 520, 328
    x = _rand_bf16(M, K, seed=60)
    w = _rand_bf16(N, K, seed=61, scale=0.05)     # [out, in]
    b = _rand_bf16(N, seed=62, scale=2.0)          # bias dominates z's spread
    y = hip_ops().linear_nt_fwd(x, w, b, act)
    z = x.float() @ w.float().t() + b.float()
    acts = {0: lambda t: t, 1: torch.sigmoid, 2: torch.tanh, 3: torch.relu,
            4: lambda t: torch.nn.functional.leaky_relu(t, 0.01)}
    ok, err = _rel_close(y, acts[act](z))
    assert ok, f"linear_nt_fwd wide act={act} maxdiff={err}"


def test_gemm_f32_wide_epilogue_nonsplit():
    """f32-out, non-split-K form of the same kernel (>= 200 tiles)."""
    M, N, K = 17149, 520, 328
    assert _tiles(M, N) >= 200
    a = _rand_bf16(M, K, seed=70)
    b = _rand_bf16(N, K, seed=71)
    c = hip_ops().gemm_ntv3_f32(a, b)
    assert c.dtype == torch.float32
    ok, err = _rel_close(c, a.float() @ b.float().t())
    assert ok, f"f32 wide epilogue maxdiff={err}"


@pytest.mark.parametrize("N", [520, 516])
def test_gemm_f32_into_slab_splitk_wide_epilogue(N):
    """Slab split-K route: once on zeros, once accumulating, with `out` the
    middle rows of a sentinel-filled buffer whose other rows must not change.
    N = 516 allows 16-byte f32 stores but would not allow bf16 ones."""
    M, K, pad, sentinel = 3500, 9224, 3, -12345.0
    tiles = _tiles(M, N)
    z = min(256 // tiles, ((K + 63) // 64) // 24)
    assert z > 1 and tiles * z >= 200      # the v4 split-K route
    a = _rand_bf16(M, K, seed=80, scale=0.5)
    b = _rand_bf16(N, K, seed=81, scale=0.5)
    ref = a.float() @ b.float().t()
    buf = torch.full((M + 2 * pad, N), sentinel, device="cuda", dtype=torch.float32)
    out = buf[pad:pad + M]
    out.zero_()
    hip_ops().gemm_ntv3_f32_into(a, b, out)
    ok, err = _rel_close(out, ref)
    assert ok, f"slab split-K N={N} (on zeros) maxdiff={err}"
    hip_ops().gemm_ntv3_f32_into(a, b, out)
    ok, err = _rel_close(out, 2.0 * ref)
    assert ok, f"slab split-K N={N} (accumulating) maxdiff={err}"
    assert bool((buf[:pad] == sentinel).all()), "rows before out were written"
    assert bool((buf[pad + M:] == sentinel).all()), "rows after out were written"


def test_gemm_wide_epilogue_repeatable():
    """Non-split-K runs are bitwise identical across repeats (edge shape)."""
    a = _rand_bf16(17149, 328, seed=90)
    b = _rand_bf16(520, 328, seed=91)
    first = hip_ops().gemm_ntv3_bf16(a, b)
    for _ in range(5):
        again = hip_ops().gemm_ntv3_bf16(a, b)
        assert torch.equal(first, again), "wide epilogue run-to-run difference"
