"""emb_update_unified_spans: duplicate flags (exact), the fused once-hit
pass plus the atomic duplicate tail against the same exact / derived-bound
references as tests/test_embedding_kernels_gpu.py, and the optimizer switch.

Rows are built per feature: column f of the [B, F] id matrix lies inside
feature f's table, as UnifiedMultiEmbedding.flat_ids guarantees, so
duplicates occur only inside a column.  Every update case mixes once-hit
rows (plain read-modify-write) with duplicate rows (atomic chain), so both
paths of the op run.

Inputs, references and bounds come from tests/emb_kernel_cases.py; the
adagrad bounds are asserted a priori from the float64 reference
(assert_bound_is_sharp, assert_rounding_fits) before a kernel runs.  A
once-hit row is one addend and one add, k = 1 in those bounds."""
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
SIZES3 = (400, 1000, 648)


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    assert torch.cuda.is_available(), "GPU test requires a GPU"
    assert hip_available(), "HIP extension must be built (native code not loaded!)"


def _spans(sizes):
    hi = torch.cumsum(torch.tensor(sizes, dtype=torch.int64), 0)
    return torch.stack([hi - torch.tensor(sizes, dtype=torch.int64), hi], dim=1).contiguous()


def _stack(cols, sizes):
    """per-feature local id columns -> (rows [B*F] global ids, spans)"""
    spans = _spans(sizes)
    rows = torch.stack([c + spans[f, 0] for f, c in enumerate(cols)], dim=1)
    return rows.reshape(-1).contiguous(), spans


def _bounded_rows(B, sizes, seed):
    """one third of the entries on once-hit rows, two thirds on rows hit twice"""
    return _stack([ec.bounded_dup_rows(B, s, seed + f) for f, s in enumerate(sizes)], sizes)


def _distinct_rows(B, sizes, seed):
    return _stack([torch.randperm(s, generator=ec.gen(seed + f))[:B]
                   for f, s in enumerate(sizes)], sizes)


def _heavy_rows(B, sizes, seed):
    """per column: 200 draws from the feature's first 24 rows (about 8 hits
    each) and B - 200 distinct rows from the rest, shuffled"""
    cols = []
    for f, s in enumerate(sizes):
        g = ec.gen(seed + f)
        heavy = torch.randint(0, 24, (200,), generator=g)
        once = torch.randperm(s - 24, generator=g)[:B - 200] + 24
        col = torch.cat([heavy, once])
        cols.append(col[torch.randperm(B, generator=g)])
    return _stack(cols, sizes)


def _expected_flags(rows):
    return (torch.bincount(rows)[rows] > 1).to(torch.uint8)


# ===========================================================================
# 1  duplicate flags, exact
# ===========================================================================
def _span_boundary_rows():
    span = int(hip_ops().emb_dup_span())
    size = span + 37
    once = torch.tensor([0, 31, 32, span - 1, span, span + 36])
    twice = torch.tensor([1, span - 2, span + 1])
    g = ec.gen(91)
    free = torch.ones(size, dtype=torch.bool)
    free[once] = False
    free[twice] = False
    rest = torch.nonzero(free).reshape(-1)
    rest = rest[torch.randperm(rest.numel(), generator=g)[:500]]
    col = torch.cat([once, twice, twice, rest])
    col = col[torch.randperm(col.numel(), generator=g)]
    return _stack([col], (size,))


def _flag_case(name):
    if name == "f3":
        return _bounded_rows(333, SIZES3, 11)
    if name == "all-repeat+distinct":
        cols = [torch.randint(0, 8, (1000,), generator=ec.gen(12)),
                torch.randperm(1500, generator=ec.gen(13))[:1000]]
        return _stack(cols, (8, 1500))
    if name == "B5":
        return _bounded_rows(5, SIZES3, 14)
    if name == "B32781":
        return _bounded_rows(32781, (262181, 40000), 15)
    assert name == "span-boundary"
    return _span_boundary_rows()


@pytest.mark.parametrize("name", ["f3", "all-repeat+distinct", "B5", "B32781",
                                  "span-boundary"])
def test_dup_flags_exact(name):
    rows, spans = _flag_case(name)
    F = spans.shape[0]
    want = _expected_flags(rows)
    assert bool(want.any()) and not bool(want.all())
    if name == "all-repeat+distinct":
        B = rows.numel() // F
        assert bool(want.view(B, F)[:, 0].all()) and not bool(want.view(B, F)[:, 1].any())
    got = hip_ops().emb_dup_flags(rows.cuda(), F, spans).cpu()
    assert got.dtype == torch.uint8 and got.shape == want.shape
    bad = torch.nonzero(got != want).reshape(-1)
    print(f"flags {name}: n={rows.numel()} flagged={int(want.sum())} wrong={bad.numel()}")
    assert bad.numel() == 0, f"first wrong entry {int(bad[0])}: row {int(rows[bad[0]])}"


# ===========================================================================
# shared runners
# ===========================================================================
def _run(case, spans, adagrad, fn="emb_update_unified_spans"):
    arena, acc, rows, dgrad, dcol0, wide, wstride, F = case.device_args()
    lr, eps = (ec.ADAGRAD_LR, ec.ADAGRAD_EPS) if adagrad else (ec.EXACT_LR, 1e-8)
    if fn == "emb_update_unified_spans":
        hip_ops().emb_update_unified_spans(arena, acc, rows, dgrad, dcol0, wide, wstride,
                                           F, lr, eps, adagrad, case.in_arena, spans)
    else:
        getattr(hip_ops(), fn)(arena, acc, rows, dgrad, dcol0, wide, wstride, F,
                               lr, eps, adagrad, case.in_arena)
    return arena, acc


def _sgd_case(D, sizes, B, in_arena, seed, rows_fn):
    g = ec.gen(seed)
    rows, spans = rows_fn(B, sizes, seed + 1)
    R, F = sum(sizes), len(sizes)
    n = B * F
    case = ec.UnifiedCase(R=R, D=D, F=F, B=B, layout="deferred", in_arena=in_arena,
                          adagrad=False, rows=rows, w0=ec.int_weights(R, D + 1, g),
                          G=ec.int_grads(n, D + 1, g), nd=6, seed=seed)
    kmax = ec.assert_exactness_condition(case.rows, R)
    ref = ec.sgd_reference(case.w0, case.rows, case.G, ec.EXACT_LR)
    assert float(ref.abs().max()) <= 256 and bool((ref == ref.round()).all())
    return case, spans, ref, kmax


def _check_sgd_exact(case, spans, ref, expect_untouched=True):
    arena, acc = _run(case, spans, False)
    vals, pad, _, raw = case.split_result(arena, acc)
    hit = ec.dup_counts(case.rows, case.R) > 0
    assert bool((~hit).any()) == expect_untouched
    assert torch.equal(ec.bits(vals[~hit]), ec.bits(case.w0[~hit])), "untouched row changed"
    assert torch.equal(ec.bits(pad), torch.zeros(case.R, dtype=torch.int16)), \
        "pad column not exactly zero"
    if case.in_arena:
        assert torch.equal(raw, ec.bits(case.arena0[:, case.D + 2:])), \
            "sgd mode changed the raw accumulator columns"
    assert torch.equal(ec.bits(vals), ec.bits(ref.to(BF16))), \
        f"{int((vals.double() != ref).sum())} elements differ from the integer reference"


def _adagrad_case(D, sizes, B, in_arena, seed, rows_fn):
    g = ec.gen(seed)
    rows, spans = rows_fn(B, sizes, seed + 1)
    R, F = sum(sizes), len(sizes)
    n = B * F
    G = ec.adagrad_grads(n, D + 1, g)
    acc0 = ec.adagrad_acc0(R, g)
    DP = D + (4 if in_arena else 2)
    w0, P = ec.adagrad_weights(acc0, rows, G, DP, g)
    case = ec.UnifiedCase(R=R, D=D, F=F, B=B, layout="deferred", in_arena=in_arena,
                          adagrad=True, rows=rows, w0=w0, G=G, acc0=acc0, nd=6, seed=seed)
    # unified kernels: mean over ALL arena columns, wide gradient included
    ref = ec.adagrad_reference(case.w0, case.acc0, case.rows, case.G, case.DP)
    ec.assert_bound_is_sharp(ref)
    ec.assert_rounding_fits(ref, P)
    return case, spans, ref


def _adagrad_errors(tag, case, ref, arena, acc):
    vals, pad, accv, raw = case.split_result(arena, acc)
    ra, rw = ec.worst_ratios(ref, vals, accv)
    print(f"{tag}: worst acc error / bound = {ra:.3f}, worst value error / bound = {rw:.3f}")
    errs = ec.compare_adagrad(ref, vals, accv)
    if not torch.equal(ec.bits(pad), torch.zeros(case.R, dtype=torch.int16)):
        errs.append("acc: pad column not exactly zero")
    if case.in_arena:
        hit = ec.dup_counts(case.rows, case.R) > 0
        if not torch.equal(raw[~hit], ec.bits(case.arena0[:, case.D + 2:])[~hit]):
            errs.append("acc: accumulator columns of an untouched row changed")
    return errs


# ===========================================================================
# 2  SGD, bit-equal
# ===========================================================================
@pytest.mark.parametrize("in_arena", [True, False])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("D", [8, 16, 64])
def test_spans_sgd_exact(D, F, in_arena):
    sizes = SIZES3 if F == 3 else (777,)
    case, spans, ref, kmax = _sgd_case(D, sizes, 333, in_arena,
                                       200 + D + 3 * F + int(in_arena), _heavy_rows)
    k = ec.dup_counts(case.rows, case.R)
    once = int((k == 1).sum())
    assert once >= 100 * F and kmax >= 4
    print(f"spans sgd D={D} F={F} in_arena={in_arena}: once-hit rows {once}, max k={kmax}")
    _check_sgd_exact(case, spans, ref)


def test_spans_sgd_exact_grid_stride_loops():
    """n = 1 050 300: more than the 3584 x 32 entries of one sweep of the
    fused grid (ten sweeps, the last one ragged) and more than the
    4096 x 4 x 64 = 1 048 576 entries one pass of the duplicate tail covers,
    with duplicates among the entries of its second pass."""
    B, sizes = 350100, (400000, 400000, 400000)
    case, spans, ref, kmax = _sgd_case(8, sizes, B, True, 77, _bounded_rows)
    assert case.n > 3584 * 32 * 9 and case.n > 4096 * 4 * 64 and kmax == 2
    assert bool(_expected_flags(case.rows)[4096 * 4 * 64:].any())
    _check_sgd_exact(case, spans, ref)


# ===========================================================================
# 3  adagrad against the derived bounds
# ===========================================================================
ADAGRAD_CASES = {
    "D64-f3-in": (64, SIZES3, 333, True),
    "D8-f3-ext": (8, SIZES3, 333, False),
    "D16-f1-in": (16, (777,), 333, True),
    # B = 32781 > 8 x 1024: the flag workgroups' chunked column scan loops
    # with a ragged tail; 262181 rows > the largest sub-range: feature 0
    # crosses a boundary.  (The capped grids of the fused pass and of the
    # duplicate tail loop in test_spans_sgd_exact_grid_stride_loops.)
    "D8-loop-in": (8, (262181, 40000), 32781, True),
}


@functools.lru_cache(maxsize=None)
def _adagrad_run(name):
    D, sizes, B, in_arena = ADAGRAD_CASES[name]
    case, spans, ref = _adagrad_case(D, sizes, B, in_arena, 300 + D + B % 97, _bounded_rows)
    k = ec.dup_counts(case.rows, case.R)
    assert bool((k == 1).any()) and bool((k == 2).any())
    if name == "D8-loop-in":
        assert B > 8 * 1024 and sizes[0] > int(hip_ops().emb_dup_span())
    arena, acc = _run(case, spans, True)
    return _adagrad_errors(f"spans {name}", case, ref, arena, acc)


@pytest.mark.parametrize("name", list(ADAGRAD_CASES))
def test_spans_adagrad_accumulator(name):
    assert not [m for m in _adagrad_run(name) if m.startswith("acc")]


@pytest.mark.parametrize("name", list(ADAGRAD_CASES))
def test_spans_adagrad_values(name):
    assert not [m for m in _adagrad_run(name) if m.startswith("values")]


# ===========================================================================
# 4  adjacent rows: plain and atomic writers share 128-byte lines
# ===========================================================================
def _interleaved_rows(B, sizes, seed):
    """256 rows, all hit: even rows once, odd rows twice"""
    assert sizes == (256,) and B == 384
    even = torch.arange(0, 256, 2)
    odd = torch.arange(1, 256, 2)
    col = torch.cat([even, odd, odd])
    return _stack([col[torch.randperm(B, generator=ec.gen(seed))]], sizes)


def test_spans_adjacent_rows_adagrad():
    case, spans, ref = _adagrad_case(64, (256,), 384, True, 41, _interleaved_rows)
    k = ec.dup_counts(case.rows, case.R)
    assert bool((k[0::2] == 1).all()) and bool((k[1::2] == 2).all())
    arena, acc = _run(case, spans, True)
    assert not _adagrad_errors("spans adjacent", case, ref, arena, acc)


def test_spans_adjacent_rows_sgd():
    case, spans, ref, _ = _sgd_case(64, (256,), 384, True, 42, _interleaved_rows)
    _check_sgd_exact(case, spans, ref, expect_untouched=False)


# ===========================================================================
# 5  once-hit rows against the old chain
# ===========================================================================
def _ordered(b16):
    """bf16 bit patterns -> integers ordered like the values (adjacent
    representable values differ by 1)"""
    b = b16.to(torch.int32)
    return torch.where(b < 0, -(b & 0x7fff), b)


@pytest.mark.parametrize("in_arena", [True, False])
def test_spans_once_hit_matches_atomic_chain(in_arena):
    case, spans, ref = _adagrad_case(64, SIZES3, 333, in_arena, 51 + int(in_arena),
                                     _distinct_rows)
    assert int(ec.dup_counts(case.rows, case.R).max()) == 1
    old = case.split_result(*_run(case, spans, True, fn="emb_update_unified"))
    new = case.split_result(*_run(case, spans, True))
    again = case.split_result(*_run(case, spans, True))
    assert torch.equal(new[2].view(torch.int32), old[2].view(torch.int32)), \
        "accumulator differs from emb_update_unified's"
    diff = (_ordered(ec.bits(new[0])) - _ordered(ec.bits(old[0]))).abs()
    print(f"once-hit vs atomic chain, in_arena={in_arena}: {int((diff != 0).sum())} of "
          f"{diff.numel()} values differ, max {int(diff.max())} bf16 step(s)")
    assert int(diff.max()) <= 1
    assert torch.equal(ec.bits(new[0]), ec.bits(again[0])) and \
        torch.equal(new[2].view(torch.int32), again[2].view(torch.int32)), \
        "two runs of the fused path differ"
    assert torch.equal(ec.bits(new[1]), ec.bits(old[1]))


# ===========================================================================
# 6  the optimizer switch
# ===========================================================================
class _Spy:
    def __init__(self, ext):
        self._ext, self.calls = ext, []

    def __getattr__(self, name):
        fn = getattr(self._ext, name)

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


@pytest.mark.parametrize("switch,op", [("0", "emb_update_unified"),
                                       (None, "emb_update_unified_spans")])
def test_optimizer_switch(monkeypatch, switch, op):
    from shifu_amd.ops import optim
    from shifu_amd.ops.flat import FlatParams
    case, spans, ref = _adagrad_case(64, SIZES3, 333, True, 61, _bounded_rows)
    arena, acc, rows, dgrad, dcol0, wide, wstride, F = case.device_args()
    p = torch.nn.Parameter(arena, requires_grad=False)
    p._is_embedding_arena = True
    p._acc_in_arena = True
    p._unified_grads = [(rows, dgrad, dcol0, wide.reshape(case.B, F), F, case.D, spans)]
    opt = optim.FusedOptimizer(FlatParams([]), [p], optimizer="adam", lr=1e-3,
                               eps=ec.ADAGRAD_EPS, emb_optimizer="adagrad",
                               emb_lr=ec.ADAGRAD_LR)
    spy = _Spy(hip_ops())
    monkeypatch.setattr(optim, "hip_ops", lambda: spy)
    if switch is None:
        monkeypatch.delenv("SHIFU_EMB_UNIQUE", raising=False)
    else:
        monkeypatch.setenv("SHIFU_EMB_UNIQUE", switch)
    opt._emb_step(p, 0)
    assert spy.calls == [op]
    assert p._unified_grads == []
    assert not _adagrad_errors(f"optimizer SHIFU_EMB_UNIQUE={switch}", case, ref, p.data, acc)
