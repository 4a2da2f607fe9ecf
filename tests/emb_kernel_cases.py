"""Input builders, float64 references and the adagrad comparator shared by
tests/test_embedding_kernels_gpu.py (runs the HIP kernels) and
tests/test_embedding_comparator_cpu.py (proves the comparator tells a right
answer from a subtly wrong one).  Plain helper module: nothing here touches
the project's own dispatch path, every reference is torch in float64 with
index_add_ over the duplicates, every random draw uses a seeded CPU
generator.

Vocabulary
----------
G         logical per-entry gradient [n, C] (bf16 values): C = D for the
          generic kernels, C = D + 1 (deep columns, then the wide column)
          for the unified ones.
mean_cols the divisor of the adagrad mean-square: D for the generic
          kernels, DP (all arena columns) for the unified ones.
k         number of entries (duplicates) that hit a row.
"""
import math

import torch

BF16 = torch.bfloat16
GROUP_STRIDE = 32768        # entries per group-stride of emb_scatter_uni_kernel
                            # once the grid is capped (4096 blocks x 8 groups)


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def bits(t):
    """Raw 16-bit view of a bf16 tensor, for bit-equality asserts."""
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------
# ids
# ---------------------------------------------------------------------------
def heavy_dup_rows(n, R, seed):
    """n uniform draws from R rows (R << n: heavy duplicates, odd and even
    row ids); every row with r % 8 == 3 is left out, so some rows stay
    untouched."""
    assert R % 8 == 0
    v = torch.randint(0, R - R // 8, (n,), generator=gen(seed))
    rows = v + v // 7 + (v % 7 >= 3).long()
    assert not bool((rows % 8 == 3).any()) and int(rows.max()) < R
    return rows


def bounded_dup_rows(n, R, seed, kmax=2):
    """n row ids over [0, R) in which every row occurs at most kmax times
    (multiplicities cycle 1..kmax), shuffled; about half of the rows stay
    untouched.  Needs R >= n."""
    assert R >= n
    g = gen(seed)
    perm = torch.randperm(R, generator=g)
    mult = (torch.arange(n) % kmax) + 1          # 1,2,1,2,...
    rows = torch.repeat_interleave(perm[:n], mult)[:n]
    return rows[torch.randperm(n, generator=g)].contiguous()


def dup_counts(rows, R):
    return torch.bincount(rows, minlength=R)


# ---------------------------------------------------------------------------
# exact (order-independent) SGD cases
# ---------------------------------------------------------------------------
EXACT_LR = 0.5
EXACT_W_MAX = 32
EXACT_K_MAX = 200


def assert_exactness_condition(rows, R):
    """Every addend is in {-1, 0, 1} and |w0| <= 32, so with k duplicates
    every partial sum is an integer of magnitude <= 32 + k.  bf16 holds all
    integers up to 256 exactly, so k <= 200 makes every add exact in any
    order."""
    kmax = int(dup_counts(rows, R).max())
    assert kmax <= EXACT_K_MAX, f"max duplicates {kmax} > {EXACT_K_MAX}"
    assert EXACT_W_MAX + kmax * 1 <= 256
    return kmax


def int_weights(R, C, g):
    return torch.randint(-EXACT_W_MAX, EXACT_W_MAX + 1, (R, C), generator=g).to(BF16)


def int_grads(n, C, g):
    return (torch.randint(-1, 2, (n, C), generator=g) * 2).to(BF16)


def sgd_reference(w0, rows, G, lr):
    """float64 w0 - lr * sum over duplicates, [R, C]."""
    w = w0.double().clone()
    w.index_add_(0, rows, -lr * G.double())
    return w


# ---------------------------------------------------------------------------
# unified-arena layouts
# ---------------------------------------------------------------------------
class UnifiedCase:
    """One call of emb_update_unified / emb_update_unified_binned.

    arena  [R, DP] bf16: deep cols 0..D-1, wide col D, zero pad col D+1 and,
           with in_arena, the raw f32 accumulator in cols D+2..D+3.
    acc    [R] f32 external accumulator (empty when in_arena or sgd).
    G      [n, D+1] logical gradient, laid out as the call layout says:
           'deferred'  dgrad [B, nd + F*D] with dcol0 = nd, wide [B, F],
                       wstride 1 -- the dense columns hold junk;
           'packed'    dgrad = vals [n, DP], dcol0 = 0, wide = vals[:, D],
                       wstride DP, F = 1 -- the pad/acc columns hold junk.
    """

    def __init__(self, *, R, D, F, B, layout, in_arena, adagrad, rows, w0,
                 G, acc0=None, nd=6, seed=0, name=""):
        assert layout in ("deferred", "packed")
        if layout == "packed":
            assert F == 1
        self.R, self.D, self.F, self.B = R, D, F, B
        self.n = B * F
        self.layout, self.in_arena, self.adagrad = layout, in_arena, adagrad
        self.DP = D + (4 if in_arena else 2)
        self.rows, self.G, self.name = rows.contiguous(), G, name
        self.w0 = w0                                   # [R, D+1] bf16
        self.acc0 = acc0                               # [R] f32 or None
        g = gen(seed + 977)
        n, DP = self.n, self.DP
        assert rows.numel() == n and G.shape == (n, D + 1)

        arena = torch.zeros(R, DP, dtype=BF16)
        arena[:, :D + 1] = w0
        if in_arena:
            if adagrad:
                arena[:, D + 2:].view(torch.float32)[:, 0] = acc0
            else:  # sgd must not touch these: arbitrary raw bits
                arena[:, D + 2:] = torch.randint(
                    -32768, 32768, (R, 2), generator=g).to(torch.int16).view(BF16)
        self.arena0 = arena
        self.acc_ext0 = (acc0.clone() if (adagrad and not in_arena)
                         else torch.empty(0, dtype=torch.float32))

        junk = lambda *s: (torch.rand(*s, generator=g) * 4 + 3).to(BF16)
        if layout == "deferred":
            assert nd and nd % 2 == 0
            self.dcol0, self.wstride = nd, 1
            dgrad = torch.empty(B, nd + F * D, dtype=BF16)
            dgrad[:, :nd] = junk(B, nd)
            dgrad[:, nd:] = G[:, :D].reshape(B, F * D)
            self.dgrad = dgrad
            self.wide = G[:, D].reshape(B, F).contiguous()
        else:
            self.dcol0, self.wstride = 0, DP
            vals = junk(n, DP)
            vals[:, :D + 1] = G
            self.dgrad = vals
            self.wide = None                           # view of dgrad, made on device

    def device_args(self, dev="cuda"):
        """(arena, acc, rows, dgrad, dcol0, wide, wstride, F) on the device,
        fresh copies of the pristine inputs."""
        arena = self.arena0.clone().to(dev)
        acc = self.acc_ext0.clone().to(dev)
        dgrad = self.dgrad.to(dev)
        wide = (self.wide.to(dev).reshape(-1) if self.layout == "deferred"
                else dgrad[:, self.D])
        return arena, acc, self.rows.to(dev), dgrad, self.dcol0, wide, self.wstride, self.F

    def split_result(self, arena, acc):
        """(values [R, D+1] bf16, pad [R] bf16, accumulator [R] f32 or None,
        raw accumulator bits [R, 2] int16 or None), all on the CPU."""
        arena = arena.cpu()
        D = self.D
        accv = raw = None
        if self.in_arena:
            raw = bits(arena[:, D + 2:])
            accv = arena[:, D + 2:].contiguous().view(torch.float32)[:, 0].clone()
        elif self.adagrad:
            accv = acc.cpu()
        return arena[:, :D + 1].contiguous(), arena[:, D + 1].contiguous(), accv, raw


def exact_unified_case(*, R, D, F, B, layout, in_arena, seed, nd=6, name=""):
    g = gen(seed)
    n = B * F
    rows = heavy_dup_rows(n, R, seed + 1)
    return UnifiedCase(R=R, D=D, F=F, B=B, layout=layout, in_arena=in_arena,
                       adagrad=False, rows=rows, w0=int_weights(R, D + 1, g),
                       G=int_grads(n, D + 1, g), nd=nd, seed=seed, name=name)


# ---------------------------------------------------------------------------
# adagrad inputs (toleranced cases)
# ---------------------------------------------------------------------------
ADAGRAD_LR = 0.75
ADAGRAD_EPS = 1e-8


def adagrad_grads(n, C, g):
    """|g| in [0.5, 1], random sign, bf16.  Such a g is a multiple of 2^-8,
    g*g a multiple of 2^-16 that is <= 1, so any f32 sum of up to 255 squares
    is exact: the kernels' own sum of squares adds no error to the
    accumulator bound."""
    mag = torch.rand(n, C, generator=g) * 0.5 + 0.5
    sign = torch.randint(0, 2, (n, C), generator=g) * 2 - 1
    G = (mag * sign).to(BF16)
    assert float(G.float().abs().min()) >= 0.5 and float(G.float().abs().max()) <= 1.0
    return G


ADAGRAD_K_MAX = 2


def adagrad_weights(acc0, rows, G, mean_cols, g, lr=None, eps=None):
    """Start values [R, C] for which CORRECT bf16 arithmetic provably meets
    the value bound 2^-9 (k+1) S + 1e-5 S, whatever the order of the adds.

    bf16 keeps 8 significant bits.  Rounding x costs at most half an ulp:
    2^-8 |x| in general, but exactly 2^-8 P for every x in the binade
    [P, 2P), P a power of two -- less than 2^-8 |x| there.  A row hit k times
    with scale sc = lr / (sqrt(acc) + eps) (from the float64 reference; it
    does not depend on the start values) has addends |u| <= |sc|, so with
    U = k |sc| every partial sum of w0 + sum u lies within |w0| +- U.  Pick
    P = 2^ceil(log2(4.5 |sc|)) and |w0| with
        |w0| - U >= P  and  |w0| + U < 2P      (all partial sums in [P, 2P))
    then the error is at most 2^-8 sum|u| (addends) + k 2^-8 P (adds), and
        2 sum|u| + 2 k P <= (k+1) (|w0| + sum|u|)
    holds for k = 1 as |w0| >= P and for k = 2 once |w0| >= 4/3 P.  (For
    k = 3 it needs |w0| >= 3/2 P, which together with the sharpness
    condition below leaves no P for some sc; the cases use k <= 2.)  The
    upper end also keeps the bound below a quarter of the smallest addend,
    0.5 |sc|.  assert_rounding_fits re-checks all of it per element from the
    reference.  Untouched rows get values in [-1, 1]."""
    lr = ADAGRAD_LR if lr is None else lr
    eps = ADAGRAD_EPS if eps is None else eps
    R, C = acc0.numel(), G.shape[1]
    k = dup_counts(rows, R).double()
    assert int(k.max()) <= ADAGRAD_K_MAX
    Gd = G.double()
    acc = acc0.double().clone().index_add_(0, rows, (Gd * Gd).sum(dim=1) / mean_cols)
    sc = lr / (acc.sqrt() + eps)
    P = 2.0 ** torch.ceil(torch.log2(4.5 * sc))
    U = 1.02 * k * sc
    ulp = P * 2.0 ** -7
    lo = torch.maximum(P + U, P * (4.0 / 3.0)) + ulp
    sharp = 0.25 * 0.5 * sc / (2.0 ** -9 * (k + 1) + 1e-5) - U
    hi = torch.minimum(2 * P - U, sharp) - ulp
    hit = k > 0
    assert bool((lo[hit] < hi[hit]).all())
    mag = lo.unsqueeze(1) + torch.rand(R, C, generator=g).double() * (hi - lo).unsqueeze(1)
    sign = (torch.randint(0, 2, (R, C), generator=g) * 2 - 1).double()
    w = mag * sign
    w[~hit] = torch.rand(int((~hit).sum()), C, generator=g).double() * 2 - 1
    return w.to(BF16), P


def assert_rounding_fits(ref, P):
    """A-priori check, from the reference alone, that the value bound leaves
    room for correct arithmetic on these inputs (see adagrad_weights): all
    partial sums stay in the binade [P, 2P), and one rounding per addend plus
    one per add plus 2e-6 S for the f32 scale fit under the bound."""
    hit = ref.k > 0
    Pc = P[hit].unsqueeze(1)
    k = ref.k[hit].double().unsqueeze(1)
    w = ref.w0[hit].double().abs()
    S = ref.S[hit]
    U = S - w
    assert bool((w - U >= Pc).all()) and bool((w + U < 2 * Pc).all())
    worst = 2.0 ** -8 * U + k * 2.0 ** -8 * Pc + 2e-6 * S
    assert bool((worst <= ref.w_bound[hit]).all()), \
        f"worst case / bound = {float((worst / ref.w_bound[hit]).max()):.3f}"


def adagrad_acc0(R, g):
    """non-zero, different per row, in [0.5, 2)"""
    return (torch.rand(R, generator=g) * 1.5 + 0.5).float()


def adagrad_unified_case(*, R, D, F, B, layout, in_arena, seed, nd=6, name=""):
    g = gen(seed)
    n = B * F
    rows = bounded_dup_rows(n, R, seed + 1)
    G = adagrad_grads(n, D + 1, g)
    acc0 = adagrad_acc0(R, g)
    DP = D + (4 if in_arena else 2)          # unified kernels: mean over DP
    w0, P = adagrad_weights(acc0, rows, G, DP, g)
    case = UnifiedCase(R=R, D=D, F=F, B=B, layout=layout, in_arena=in_arena,
                       adagrad=True, rows=rows, w0=w0, G=G, acc0=acc0,
                       nd=nd, seed=seed, name=name)
    case.binade = P
    return case


class GenericCase:
    """One call of emb_adagrad_step on a plain [R, D] arena."""

    def __init__(self, *, R, D, n, seed):
        g = gen(seed)
        self.R, self.D, self.n = R, D, n
        self.rows = bounded_dup_rows(n, R, seed + 1)
        self.G = adagrad_grads(n, D, g)
        self.acc0 = adagrad_acc0(R, g)
        self.w0, self.binade = adagrad_weights(self.acc0, self.rows, self.G, D, g)
        self.name = f"generic-D{D}"


# the shapes both test files iterate ---------------------------------------
GENERIC_ADAGRAD_D = [1, 4, 7, 8, 10, 64, 130]


def generic_adagrad_case(D):
    # n odd: the last emb_accsq_kernel block is partly filled
    return GenericCase(R=1024, D=D, n=999, seed=100 + D)


def _small_unified_params():
    out = []
    for D in (8, 16, 64):
        for in_arena in (True, False):
            for F in (1, 3):
                out.append(("deferred", D, F, in_arena))
            out.append(("packed", D, 1, in_arena))
    return out


SMALL_UNIFIED_ADAGRAD = _small_unified_params()


def small_unified_adagrad_case(layout, D, F, in_arena):
    # B odd -> n = B*F odd for F in {1, 3}: the single-entry tail of
    # emb_accsq_uni_kernel; n <= 1024 keeps every binned bucket in one chunk
    B = 333
    seed = 7 * D + 3 * F + (1 if in_arena else 0) + (50 if layout == "packed" else 0)
    return adagrad_unified_case(R=1024, D=D, F=F, B=B, layout=layout,
                                in_arena=in_arena, seed=seed, nd=6,
                                name=f"{layout}-D{D}-F{F}-{'in' if in_arena else 'ext'}")


LOOP_B, LOOP_F, LOOP_D = 32781, 3, 8        # n = 98343 = 3 * 32768 + 39


def loop_unified_adagrad_case(in_arena):
    """Every 32-lane group of emb_scatter_uni_kernel runs 3 iterations and 39
    groups a 4th: the rows -> acc prefetch rotation is exercised."""
    assert LOOP_B * LOOP_F > 3 * GROUP_STRIDE
    return adagrad_unified_case(R=131072, D=LOOP_D, F=LOOP_F, B=LOOP_B,
                                layout="deferred", in_arena=in_arena,
                                seed=31 + (1 if in_arena else 0), nd=6,
                                name=f"loop-{'in' if in_arena else 'ext'}")


# ---------------------------------------------------------------------------
# float64 adagrad reference + the comparator
# ---------------------------------------------------------------------------
class AdagradRef:
    pass


def adagrad_reference(w0, acc0, rows, G, mean_cols, lr=ADAGRAD_LR, eps=ADAGRAD_EPS):
    """acc = acc0 + sum_j mean(g_j^2);  w = w0 + sum_j u_j with
    u_j = -lr / (sqrt(acc_final) + eps) * g_j, all float64."""
    R = w0.shape[0]
    Gd = G.double()
    ref = AdagradRef()
    ref.R, ref.rows = R, rows
    ref.k = dup_counts(rows, R)
    ref.acc0 = acc0
    ref.w0 = w0
    meansq = (Gd * Gd).sum(dim=1) / mean_cols
    ref.acc = acc0.double().clone().index_add_(0, rows, meansq)
    sc = -lr / (ref.acc.sqrt() + eps)
    u = sc[rows].unsqueeze(1) * Gd
    ref.w = w0.double().clone().index_add_(0, rows, u)
    ref.S = w0.double().abs().index_add_(0, rows, u.abs())          # [R, C]
    ref.min_u = torch.full((R,), math.inf, dtype=torch.float64).scatter_reduce_(
        0, rows, u.abs().amin(dim=1), reduce="amin")
    # per element: one bf16 rounding of each addend, one per atomic add,
    # plus the f32 sqrt and divide
    kp1 = (ref.k + 1).double().unsqueeze(1)
    ref.w_bound = 2.0 ** -9 * kp1 * ref.S + 1e-5 * ref.S
    # per row: k f32 atomic adds in any order (+ the f32 mean)
    ref.acc_bound = (ref.k + 2).double() * 2.0 ** -23 * ref.acc
    return ref


def assert_bound_is_sharp(ref):
    """The value bound must stay below a quarter of the smallest single
    addend of the row, for every touched element: a dropped or doubled entry
    is then at least four bounds away."""
    hit = ref.k > 0
    assert int(ref.k.max()) <= 3
    worst = (ref.w_bound[hit] / ref.min_u[hit].unsqueeze(1)).max()
    assert float(worst) <= 0.25, f"bound / smallest addend = {float(worst):.3f}"


def worst_ratios(ref, got_w, got_acc):
    """(max |acc error| / acc bound, max |value error| / value bound) over
    the touched rows: the figures the tests print before they assert."""
    hit = ref.k > 0
    ra = ((got_acc.double() - ref.acc).abs() / ref.acc_bound)[hit].max()
    rw = ((got_w.double() - ref.w).abs() / ref.w_bound)[hit].max()
    return float(ra), float(rw)


def compare_adagrad(ref, got_w, got_acc):
    """Violations of the derived bounds, as a list of strings (empty =
    accepted).  got_w [R, C] bf16, got_acc [R] f32, both on the CPU."""
    errs = []
    hit = ref.k > 0
    # accumulator
    dacc = (got_acc.double() - ref.acc).abs()
    bad = hit & ~(dacc <= ref.acc_bound)
    if bad.any():
        r = int(torch.nonzero(bad)[0])
        errs.append(f"acc: {int(bad.sum())} rows out of bound, e.g. row {r}: got "
                    f"{float(got_acc[r])!r} ref {float(ref.acc[r])!r} "
                    f"bound {float(ref.acc_bound[r]):.3e}")
    if not torch.equal(got_acc[~hit].view(torch.int32), ref.acc0[~hit].view(torch.int32)):
        errs.append("acc: an untouched row changed")
    # values
    dw = (got_w.double() - ref.w).abs()
    badw = hit.unsqueeze(1) & ~(dw <= ref.w_bound)
    if badw.any():
        r, c = (int(x) for x in torch.nonzero(badw)[0])
        errs.append(f"values: {int(badw.sum())} elements out of bound, e.g. [{r},{c}]: "
                    f"got {float(got_w[r, c])!r} ref {float(ref.w[r, c])!r} "
                    f"bound {float(ref.w_bound[r, c]):.3e} (k={int(ref.k[r])})")
    if not torch.equal(bits(got_w[~hit]), bits(ref.w0[~hit])):
        errs.append("values: an untouched row changed")
    return errs


# ---------------------------------------------------------------------------
# torch emulation of the atomic path's rounding sequence (CPU self-check)
# ---------------------------------------------------------------------------
def _rounds(rows, order):
    """Split a shuffled application order into rounds in which every row
    occurs at most once, keeping each row's entries in shuffled order -- a
    vectorised stand-in for applying the entries one by one."""
    r = rows[order]
    srt = torch.argsort(r, stable=True)
    rs = r[srt]
    first = torch.ones_like(rs, dtype=torch.bool)
    first[1:] = rs[1:] != rs[:-1]
    idx = torch.arange(rs.numel())
    start = torch.cummax(torch.where(first, idx, torch.zeros_like(idx)), 0).values
    rank = idx - start
    ent = order[srt]
    return [ent[rank == q] for q in range(int(rank.max()) + 1)]


def emulate_atomic_adagrad(w0, acc0, rows, G, mean_cols, seed, lr=ADAGRAD_LR,
                           eps=ADAGRAD_EPS, *, acc_cols=None, drop_scatter=None,
                           drop_both=None, pre_step_denominator=False,
                           denominator_of=None):
    """The kernels' arithmetic on the CPU: f32 mean-square per entry, f32
    accumulator adds in a shuffled order, then per entry a bf16-rounded
    addend added in a (different) shuffled order with a bf16 rounding after
    every add.  The keyword switches build the mutants:
      acc_cols              divisor of the mean other than mean_cols
      drop_scatter / _both  entry index left out of the scatter / of both passes
      pre_step_denominator  sqrt(acc0) instead of sqrt(acc_final)
      denominator_of        [n] entry whose row's denominator each entry uses
    """
    g = gen(seed)
    n = rows.numel()
    Gf = G.float()
    keep = torch.ones(n, dtype=torch.bool)
    if drop_both is not None:
        keep[drop_both] = False
    meansq = (Gf * Gf).sum(dim=1) / float(acc_cols or mean_cols)
    acc = acc0.clone()
    order = torch.randperm(n, generator=g)
    for ent in _rounds(rows, order[keep[order]]):
        acc[rows[ent]] = acc[rows[ent]] + meansq[ent]            # f32 adds
    den_acc = acc0 if pre_step_denominator else acc
    src = rows if denominator_of is None else rows[denominator_of]
    sc = torch.tensor(-lr, dtype=torch.float32) / (den_acc[src].sqrt() + torch.tensor(
        eps, dtype=torch.float32))
    add = (sc.unsqueeze(1) * Gf).to(BF16)                        # rounded addend
    if drop_scatter is not None:
        keep[drop_scatter] = False
    w = w0.clone()
    order = torch.randperm(n, generator=g)
    for ent in _rounds(rows, order[keep[order]]):
        w[rows[ent]] = (w[rows[ent]].float() + add[ent].float()).to(BF16)
    return w, acc
