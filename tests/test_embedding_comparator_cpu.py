"""Self-check of the comparator that tests/test_embedding_kernels_gpu.py uses
for the adagrad embedding kernels.  No GPU: a torch emulation of the atomic
path's rounding sequence must be ACCEPTED on every input the GPU tests use,
for several arrival orders, and each of a set of subtly wrong kernels
(mutants) must be REJECTED.  This is the evidence that the GPU tests would
fail on a kernel that is only slightly wrong.

The inputs are built so that correct bf16 arithmetic provably fits the
value bound (emb_kernel_cases.adagrad_weights); the emulation checks that
claim by example, and every mutant must be more than two bounds away."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emb_kernel_cases as ec  # noqa: E402

SHUFFLES = [0, 1, 2]


def _unified_ref(case):
    return ec.adagrad_reference(case.w0, case.acc0, case.rows, case.G, case.DP)


def _generic_ref(case):
    return ec.adagrad_reference(case.w0, case.acc0, case.rows, case.G, case.D)


@pytest.fixture(scope="module")
def loop_case():
    case = ec.loop_unified_adagrad_case(True)
    return case, _unified_ref(case)


@pytest.fixture(scope="module")
def small_case():
    # deferred layout, D=8, F=3, D+4 arena: DP = 12
    case = ec.small_unified_adagrad_case("deferred", 8, 3, True)
    return case, _unified_ref(case)


# --------------------------------------------------------------- acceptance
def _accepts(case, ref, cols, part):
    """The emulation, for several arrival orders, against one of the two
    bounds ('acc' or 'values'); prints the figures before asserting."""
    ec.assert_bound_is_sharp(ref)
    ec.assert_rounding_fits(ref, case.binade)
    for s in SHUFFLES:
        w, acc = ec.emulate_atomic_adagrad(case.w0, case.acc0, case.rows, case.G,
                                           cols, seed=s)
        ra, rw = ec.worst_ratios(ref, w, acc)
        print(f"{case.name} shuffle {s}: worst acc error / bound = {ra:.3f}, "
              f"worst value error / bound = {rw:.3f}")
        errs = [m for m in ec.compare_adagrad(ref, w, acc) if m.startswith(part)]
        assert errs == []


PARTS = ["acc", "values"]


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("D", ec.GENERIC_ADAGRAD_D)
def test_comparator_accepts_emulation_generic(D, part):
    case = ec.generic_adagrad_case(D)
    _accepts(case, _generic_ref(case), case.D, part)


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("layout,D,F,in_arena", ec.SMALL_UNIFIED_ADAGRAD)
def test_comparator_accepts_emulation_unified(layout, D, F, in_arena, part):
    case = ec.small_unified_adagrad_case(layout, D, F, in_arena)
    _accepts(case, _unified_ref(case), case.DP, part)


@pytest.mark.parametrize("part", PARTS)
def test_comparator_accepts_emulation_loop_case(loop_case, part):
    case, ref = loop_case
    _accepts(case, ref, case.DP, part)


def test_layouts_hold_the_logical_gradient():
    """The builders lay G out the way the kernels address it: entry e=(b,f)
    at dgrad[b, dcol0 + f*D + d] and wide[e * wstride]."""
    for layout, F in (("deferred", 3), ("packed", 1)):
        case = ec.small_unified_adagrad_case(layout, 8, F, True)
        D, n = case.D, case.n
        dflat = case.dgrad.reshape(-1)
        dstride = case.dgrad.shape[1]
        e = torch.arange(n)
        base = (e // F) * dstride + case.dcol0 + (e % F) * D
        deep = dflat[base.unsqueeze(1) + torch.arange(D)]
        assert torch.equal(deep, case.G[:, :D])
        wflat = (case.wide.reshape(-1) if layout == "deferred"
                 else dflat[D:])
        assert torch.equal(wflat[e * case.wstride], case.G[:, D])


# ------------------------------------------------------------------ mutants
def _rejected(ref, w, acc, part):
    """The comparator reports a violation of the given bound, and the worst
    error is more than two bounds away, so the rejection does not hang on
    the last bit of the bound."""
    ra, rw = ec.worst_ratios(ref, w, acc)
    print(f"mutant: worst acc error / bound = {ra:.3f}, worst value error / bound = {rw:.3f}")
    errs = ec.compare_adagrad(ref, w, acc)
    assert any(m.startswith(part) for m in errs), errs
    assert (ra if part == "acc" else rw) > 2.0
    return ra, rw


def _a_duplicate(case):
    """an entry whose row is hit more than once"""
    k = ec.dup_counts(case.rows, case.R)
    return int(torch.nonzero(k[case.rows] >= 2)[0])


@pytest.mark.parametrize("which", ["drop_scatter", "drop_both"])
def test_comparator_rejects_dropped_duplicate(small_case, which):
    case, ref = small_case
    e = _a_duplicate(case)
    for s in SHUFFLES:
        w, acc = ec.emulate_atomic_adagrad(case.w0, case.acc0, case.rows, case.G,
                                           case.DP, seed=s, **{which: e})
        _rejected(ref, w, acc, "values")


def test_comparator_rejects_dropped_duplicate_generic():
    case = ec.generic_adagrad_case(7)
    ref = _generic_ref(case)
    e = _a_duplicate(case)
    w, acc = ec.emulate_atomic_adagrad(case.w0, case.acc0, case.rows, case.G,
                                       case.D, seed=0, drop_both=e)
    _rejected(ref, w, acc, "values")
    _rejected(ref, w, acc, "acc")


def test_comparator_rejects_pre_step_denominator(small_case):
    case, ref = small_case
    for s in SHUFFLES:
        w, acc = ec.emulate_atomic_adagrad(case.w0, case.acc0, case.rows, case.G,
                                           case.DP, seed=s, pre_step_denominator=True)
        # the accumulator itself is right; only the values give it away
        ra, _ = _rejected(ref, w, acc, "values")
        assert ra <= 1.0


def test_comparator_rejects_mean_over_D(small_case):
    case, ref = small_case
    assert case.DP != case.D
    w, acc = ec.emulate_atomic_adagrad(case.w0, case.acc0, case.rows, case.G,
                                       case.DP, seed=0, acc_cols=case.D)
    _rejected(ref, w, acc, "acc")


def test_comparator_rejects_wide_stride_DP(small_case):
    """deferred layout: wide is [B, F] with stride 1; a kernel that strides
    it by DP reads another entry's wide gradient (wrapped here to stay in
    range)."""
    case, ref = small_case
    assert case.wstride == 1
    wflat = case.wide.reshape(-1)
    G = case.G.clone()
    G[:, case.D] = wflat[(torch.arange(case.n) * case.DP) % case.n]
    w, acc = ec.emulate_atomic_adagrad(case.w0, case.acc0, case.rows, G,
                                       case.DP, seed=0)
    _rejected(ref, w, acc, "values")


def test_comparator_rejects_rotated_denominator(loop_case):
    """loop case: entry e scaled with the denominator of the entry one
    group-stride later -- what a wrong prefetch rotation would do."""
    case, ref = loop_case
    e = torch.arange(case.n)
    other = torch.where(e + ec.GROUP_STRIDE < case.n, e + ec.GROUP_STRIDE, e)
    w, acc = ec.emulate_atomic_adagrad(case.w0, case.acc0, case.rows, case.G,
                                       case.DP, seed=0, denominator_of=other)
    ra, _ = _rejected(ref, w, acc, "values")
    assert ra <= 1.0


def test_exactness_condition_holds_for_the_exact_cases():
    """The ids of the loop-iterating exact cases keep every partial sum an
    integer bf16 represents."""
    rows = ec.heavy_dup_rows(98343, 4096, 1)
    assert ec.assert_exactness_condition(rows, 4096) <= ec.EXACT_K_MAX
    with pytest.raises(AssertionError):
        ec.assert_exactness_condition(torch.zeros(201, dtype=torch.long), 4)
