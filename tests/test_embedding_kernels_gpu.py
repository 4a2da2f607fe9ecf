"""Embedding arena kernels (gather, scatter, accsq, unified and binned
updates) against exact float64 / index_select references.

* exact tests: integer-valued inputs for which every bf16 add is exact in
  any order, so the atomics' result must be BIT-EQUAL to the reference;
* gather tests: a pure copy, torch.equal against index_select;
* adagrad tests: per-row bounds derived from the rounding points of the
  kernels (tests/emb_kernel_cases.py), never from what the kernels return.
  tests/test_embedding_comparator_cpu.py shows the same comparator rejecting
  subtly wrong kernels.

The loop cases are the smallest shapes at which the capped grids
(4096 blocks x 256 threads) make a thread or a 32-lane group iterate.

The adagrad value bound 2^-9 (k+1) S + 1e-5 S budgets 2^-9 per bf16 rounding,
while one rounding can cost up to 2^-8 of the value (half an ulp at the
bottom of a binade).  Correct arithmetic meets it all the same on these
inputs because of how the start values are built: every partial sum of a
touched element stays inside one binade [P, 2P) with |w0| >= 4/3 P and
k <= 2, where a rounding costs 2^-8 P, not 2^-8 |x|
(emb_kernel_cases.adagrad_weights has the derivation).  Each test asserts
that a-priori room from the float64 reference (assert_rounding_fits) and
that the bound stays under a quarter of the row's smallest addend
(assert_bound_is_sharp) before it launches a kernel."""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from shifu_amd.ops.dispatch import hip_available, hip_ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emb_kernel_cases as ec  # noqa: E402

BF16 = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    assert torch.cuda.is_available(), "GPU test requires a GPU"
    assert hip_available(), "HIP extension must be built (native code not loaded!)"


def _update_fn(name):
    return getattr(hip_ops(), name)


UPDATE_FNS = ["emb_update_unified", "emb_update_unified_binned"]


# ===========================================================================
# B1  exact SGD
# ===========================================================================
def _sgd_step_exact(D, R, n, seed):
    g = ec.gen(seed)
    rows = ec.heavy_dup_rows(n, R, seed + 1)
    kmax = ec.assert_exactness_condition(rows, R)
    assert bool((rows % 2 == 0).any()) and bool((rows % 2 == 1).any())
    w0 = ec.int_weights(R, D, g)
    G = ec.int_grads(n, D, g)
    ref = ec.sgd_reference(w0, rows, G, ec.EXACT_LR)
    assert float(ref.abs().max()) <= 256 and bool((ref == ref.round()).all())
    arena = w0.clone().cuda()
    hip_ops().emb_sgd_step(arena, rows.cuda(), G.cuda(), ec.EXACT_LR)
    got = arena.cpu()
    print(f"emb_sgd_step D={D} n={n} R={R} max k={kmax}")
    hit = ec.dup_counts(rows, R) > 0
    assert bool((~hit).any())
    assert torch.equal(ec.bits(got[~hit]), ec.bits(w0[~hit])), "untouched row changed"
    assert torch.equal(ec.bits(got), ec.bits(ref.to(BF16))), \
        f"{int((got.double() != ref).sum())} elements differ from the integer reference"


@pytest.mark.parametrize("D", [1, 2, 3, 5, 6, 7, 32, 33])
def test_sgd_step_exact(D):
    _sgd_step_exact(D, R=64, n=2048, seed=10 + D)


def test_sgd_step_exact_grid_stride_loop():
    """n * pairs = 1 050 003 > 1 048 576 threads: the first threads of
    emb_scatter_kernel take a second grid-stride iteration."""
    n, D = 350001, 6
    assert n * (D // 2) > 4096 * 256
    _sgd_step_exact(D, R=8192, n=n, seed=77)


@functools.lru_cache(maxsize=None)
def _exact_case(layout, in_arena, loop):
    if loop:
        case = ec.exact_unified_case(R=4096, D=8, F=3, B=32781, layout=layout,
                                     in_arena=in_arena, seed=5, nd=6)
        assert case.n == 98343 and case.n > 3 * ec.GROUP_STRIDE
    else:
        F = 3 if layout == "deferred" else 1
        case = ec.exact_unified_case(R=64, D=16, F=F, B=2049 // F, layout=layout,
                                     in_arena=in_arena, seed=6, nd=6)
        assert case.n == 2049
    kmax = ec.assert_exactness_condition(case.rows, case.R)
    ref = ec.sgd_reference(case.w0, case.rows, case.G, ec.EXACT_LR)
    assert float(ref.abs().max()) <= 256
    return case, ref, kmax


def _check_unified_exact(fn, case, ref):
    arena, acc, rows, dgrad, dcol0, wide, wstride, F = case.device_args()
    _update_fn(fn)(arena, acc, rows, dgrad, dcol0, wide, wstride, F,
                   ec.EXACT_LR, 1e-8, False, case.in_arena)
    vals, pad, _, raw = case.split_result(arena, acc)
    hit = ec.dup_counts(case.rows, case.R) > 0
    assert bool((~hit).any())
    assert torch.equal(ec.bits(vals[~hit]), ec.bits(case.w0[~hit])), "untouched row changed"
    assert torch.equal(ec.bits(pad), torch.zeros(case.R, dtype=torch.int16)), \
        "pad column not exactly zero"
    if case.in_arena:
        assert torch.equal(raw, ec.bits(case.arena0[:, case.D + 2:])), \
            "sgd mode changed the raw accumulator columns"
    assert torch.equal(ec.bits(vals), ec.bits(ref.to(BF16))), \
        f"{int((vals.double() != ref).sum())} elements differ from the integer reference"


@pytest.mark.parametrize("in_arena", [True, False])
@pytest.mark.parametrize("layout", ["deferred", "packed"])
@pytest.mark.parametrize("fn", UPDATE_FNS)
def test_unified_sgd_exact(fn, layout, in_arena):
    case, ref, kmax = _exact_case(layout, in_arena, False)
    print(f"{fn} {layout} in_arena={in_arena} n={case.n} max k={kmax}")
    _check_unified_exact(fn, case, ref)


@pytest.mark.parametrize("fn", UPDATE_FNS)
def test_unified_sgd_exact_group_stride_loop(fn):
    """n = 98343 = 3 * 32768 + 39 entries: every 32-lane group of
    emb_scatter_uni_kernel runs 3 iterations, 39 groups a 4th."""
    case, ref, kmax = _exact_case("deferred", True, True)
    print(f"{fn} loop n={case.n} max k={kmax}")
    _check_unified_exact(fn, case, ref)


# ===========================================================================
# B2  gather
# ===========================================================================
def _coded_arena(R, C):
    """arena[r, c] has the bit pattern r*C + c + 1: distinct for every (r, c)
    and a finite positive bf16 (R*C < 0x4000)."""
    assert R * C < 0x4000
    return (torch.arange(R * C, dtype=torch.int32) + 1).to(torch.int16).reshape(R, C).view(BF16)


def _gather_ref(arena, ids, cols):
    """[B, F*cols] bit patterns of arena[ids[b, f], :cols] via index_select"""
    B, F = ids.shape
    sel = ec.bits(arena).index_select(0, ids.reshape(-1))
    return sel[:, :cols].reshape(B, F * cols)


def _ids(B, F, R, seed):
    return torch.randint(0, R, (B, F), generator=ec.gen(seed))


@functools.lru_cache(maxsize=None)
def _loop_ids():
    # 1 048 579 lookups; R small: every row is looked up many times
    return _ids(149797, 7, 1000, 3)


@pytest.mark.parametrize("D", [1, 3, 5, 6, 7, 8, 24, 64])
def test_embedding_gather_exact(D):
    R = 200
    arena = _coded_arena(R, D)
    ids = _ids(257, 3, R, 40 + D)          # 771 lookups of 200 rows: duplicates
    out = hip_ops().embedding_gather(arena.cuda(), ids.cuda())
    assert out.shape == (257, 3 * D)
    assert torch.equal(ec.bits(out.cpu()), _gather_ref(arena, ids, D))


def _sentinel_out(B, cols, nd):
    out = torch.full((B, cols), -3.0, dtype=BF16)
    out[:, :nd] = (torch.arange(B * nd).reshape(B, nd) % 251).to(BF16)
    return out


@pytest.mark.parametrize("D", [8, 16])
@pytest.mark.parametrize("nd", [2, 10, 12])
def test_embedding_gather_into_exact(nd, D):
    R, B, F = 200, 257, 3
    arena = _coded_arena(R, D)
    ids = _ids(B, F, R, 60 + D + nd)
    out0 = _sentinel_out(B, nd + F * D, nd)
    out = out0.clone().cuda()
    hip_ops().embedding_gather_into(arena.cuda(), ids.cuda(), out, nd)
    out = out.cpu()
    assert torch.equal(ec.bits(out[:, :nd]), ec.bits(out0[:, :nd])), "dense columns touched"
    assert torch.equal(ec.bits(out[:, nd:]), _gather_ref(arena, ids, D))


def _check_gather_split(arena, ids, nd, D):
    B, F = ids.shape
    out0 = _sentinel_out(B, nd + F * D, nd)
    out = out0.clone().cuda()
    wide = torch.full((B, F), -5.0, dtype=BF16).cuda()
    hip_ops().emb_gather_split(arena.cuda(), ids.cuda(), out, wide, nd, D)
    out, wide = out.cpu(), wide.cpu()
    sel = ec.bits(arena).index_select(0, ids.reshape(-1))
    assert torch.equal(ec.bits(out[:, :nd]), ec.bits(out0[:, :nd])), "dense columns touched"
    assert torch.equal(ec.bits(out[:, nd:]), sel[:, :D].reshape(B, F * D))
    assert torch.equal(ec.bits(wide), sel[:, D].reshape(B, F)), "wide column is not arena col D"


@pytest.mark.parametrize("extra", [4, 2])          # arena cols = D + extra
@pytest.mark.parametrize("D", [8, 16])
@pytest.mark.parametrize("nd", [2, 10, 12])
def test_gather_split_exact(nd, D, extra):
    R = 200
    arena = _coded_arena(R, D + extra)
    _check_gather_split(arena, _ids(257, 3, R, 80 + D + nd + extra), nd, D)


def test_gather_split_exact_unrolled_loop():
    """1 048 579 lookups at D=8: 2 097 158 work items over the capped grid of
    1 048 576 threads -- every thread takes the second half of the 2-way
    unroll, u lands on both sides of deep_total and of total, and the first
    threads take a second outer iteration."""
    ids = _loop_ids()
    assert ids.numel() == 1048579
    _check_gather_split(_coded_arena(1000, 12), ids, 2, 8)


def test_embedding_gather_exact_grid_stride_loop():
    ids = _loop_ids()
    arena = _coded_arena(1000, 8)
    ref = _gather_ref(arena, ids, 8)
    out = hip_ops().embedding_gather(arena.cuda(), ids.cuda())
    assert torch.equal(ec.bits(out.cpu()), ref)
    nd = 2
    out0 = _sentinel_out(ids.shape[0], nd + 7 * 8, nd)
    into = out0.clone().cuda()
    hip_ops().embedding_gather_into(arena.cuda(), ids.cuda(), into, nd)
    into = into.cpu()
    assert torch.equal(ec.bits(into[:, :nd]), ec.bits(out0[:, :nd])), "dense columns touched"
    assert torch.equal(ec.bits(into[:, nd:]), ref)


def test_embedding_gather_scalar_exact_grid_stride_loop():
    """350 007 lookups at D=3: 1 050 021 elements > 1 048 576 threads."""
    ids = _ids(50001, 7, 1000, 9)
    assert ids.numel() >= 350000 and ids.numel() * 3 > 4096 * 256
    arena = _coded_arena(1000, 3)
    out = hip_ops().embedding_gather(arena.cuda(), ids.cuda())
    assert torch.equal(ec.bits(out.cpu()), _gather_ref(arena, ids, 3))


# ===========================================================================
# B3  adagrad, derived bounds.  Each kernel run is checked by two tests: the
# accumulator (with pad column and untouched rows) and the values, so a
# report shows which of the two bounds a kernel misses.
# ===========================================================================
def _errors(tag, ref, got_w, got_acc, prefix):
    ra, rw = ec.worst_ratios(ref, got_w, got_acc)
    print(f"{tag}: worst acc error / bound = {ra:.3f}, worst value error / bound = {rw:.3f}")
    return [m for m in ec.compare_adagrad(ref, got_w, got_acc) if m.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def _generic_run(D):
    case = ec.generic_adagrad_case(D)
    ref = ec.adagrad_reference(case.w0, case.acc0, case.rows, case.G, D)
    ec.assert_bound_is_sharp(ref)
    ec.assert_rounding_fits(ref, case.binade)
    arena = case.w0.clone().cuda()
    acc = case.acc0.clone().cuda()
    hip_ops().emb_adagrad_step(arena, acc, case.rows.cuda(), case.G.cuda(),
                               ec.ADAGRAD_LR, ec.ADAGRAD_EPS)
    return case, ref, arena.cpu(), acc.cpu()


@pytest.mark.parametrize("D", ec.GENERIC_ADAGRAD_D)
def test_adagrad_step_accumulator(D):
    """emb_accsq_small_kernel (D <= 8 or odd) and emb_accsq_kernel (lane loop
    with a tail at D=130): mean over D, any order of the f32 atomics."""
    case, ref, w, acc = _generic_run(D)
    assert not _errors(case.name, ref, w, acc, "acc")


@pytest.mark.parametrize("D", ec.GENERIC_ADAGRAD_D)
def test_adagrad_step_values(D):
    """emb_scatter_acc_kernel: denominator from the finished accumulator;
    packed atomics at even D, the CAS path at D=1 and D=7."""
    case, ref, w, acc = _generic_run(D)
    assert not _errors(case.name, ref, w, acc, "values")


def _unified_case(key):
    if key[0] == "loop":
        return ec.loop_unified_adagrad_case(key[1])
    return ec.small_unified_adagrad_case(*key)


@functools.lru_cache(maxsize=None)
def _unified_ref(key):
    case = _unified_case(key)
    # unified kernels: mean over ALL arena columns, wide gradient included
    ref = ec.adagrad_reference(case.w0, case.acc0, case.rows, case.G, case.DP)
    ec.assert_bound_is_sharp(ref)
    ec.assert_rounding_fits(ref, case.binade)
    return case, ref


@functools.lru_cache(maxsize=None)
def _unified_run(fn, key):
    case, ref = _unified_ref(key)
    arena, acc, rows, dgrad, dcol0, wide, wstride, F = case.device_args()
    _update_fn(fn)(arena, acc, rows, dgrad, dcol0, wide, wstride, F,
                   ec.ADAGRAD_LR, ec.ADAGRAD_EPS, True, case.in_arena)
    return (case, ref) + case.split_result(arena, acc)


def _check_unified_accumulator(fn, key):
    case, ref, vals, pad, accv, raw = _unified_run(fn, key)
    assert torch.equal(ec.bits(pad), torch.zeros(case.R, dtype=torch.int16)), \
        "pad column not exactly zero"
    if case.in_arena:
        hit = ec.dup_counts(case.rows, case.R) > 0
        assert torch.equal(raw[~hit], ec.bits(case.arena0[:, case.D + 2:])[~hit]), \
            "accumulator columns of an untouched row changed"
    assert not _errors(f"{fn} {case.name}", ref, vals, accv, "acc")


def _check_unified_values(fn, key):
    case, ref, vals, pad, accv, raw = _unified_run(fn, key)
    assert not _errors(f"{fn} {case.name}", ref, vals, accv, "values")


@pytest.mark.parametrize("layout,D,F,in_arena", ec.SMALL_UNIFIED_ADAGRAD)
def test_unified_adagrad_accumulator(layout, D, F, in_arena):
    key = (layout, D, F, in_arena)
    assert _unified_ref(key)[0].n % 2 == 1   # single-entry tail of emb_accsq_uni_kernel
    _check_unified_accumulator("emb_update_unified", key)


@pytest.mark.parametrize("layout,D,F,in_arena", ec.SMALL_UNIFIED_ADAGRAD)
def test_unified_adagrad_values(layout, D, F, in_arena):
    _check_unified_values("emb_update_unified", (layout, D, F, in_arena))


@pytest.mark.parametrize("layout,D,F,in_arena", ec.SMALL_UNIFIED_ADAGRAD)
def test_unified_binned_adagrad_accumulator(layout, D, F, in_arena):
    """n <= 1024: no bucket can overflow one 1024-entry chunk, so the binned
    path sees the same full-step denominator as the reference."""
    key = (layout, D, F, in_arena)
    assert _unified_ref(key)[0].n <= 1024
    _check_unified_accumulator("emb_update_unified_binned", key)


@pytest.mark.parametrize("layout,D,F,in_arena", ec.SMALL_UNIFIED_ADAGRAD)
def test_unified_binned_adagrad_values(layout, D, F, in_arena):
    _check_unified_values("emb_update_unified_binned", (layout, D, F, in_arena))


@pytest.mark.parametrize("in_arena", [True, False])
def test_unified_adagrad_accumulator_group_stride_loop(in_arena):
    case = _unified_ref(("loop", in_arena))[0]
    assert case.n == 98343 and case.R == 131072 and case.D == 8
    _check_unified_accumulator("emb_update_unified", ("loop", in_arena))


@pytest.mark.parametrize("in_arena", [True, False])
def test_unified_adagrad_values_group_stride_loop(in_arena):
    """n = 98343, D = 8, R = 131072: the 2-deep rows -> acc prefetch rotation
    of emb_scatter_uni_kernel must hand every entry its own row's
    denominator (rows have different accumulators); the CPU self-check
    shows a denominator rotated by one group-stride far outside the bound."""
    _check_unified_values("emb_update_unified", ("loop", in_arena))

