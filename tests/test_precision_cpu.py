"""precision_rules.py is right and has teeth -- on the CPU, before any kernel is held to it.

exact_struct equals an evaluation in rationals; the C oracle (the reference's order) and an emulation of the kernels'
FMA order stay inside gamma(7 m) A at every width; seven ways of being subtly wrong are rejected, two of which
conftest.assert_struct_close accepts at 1e-6 (the gap this file pins); and every input of test_gpu_precision.py has at
least half of its in-record windows in the tight class."""
import math

import numpy as np
import pytest

import precision_rules as pr
from conftest import assert_struct_close
from rnascan_amd import pack

WIDTHS = [1, 2, 7, 8, 9, 12, 18, 19, 24, 64, 65, 200]
SPECIAL = [-np.inf, np.inf, np.nan, 0.0, -0.0, 1e-300, -1e300]     # the cells test_gpu_property draws


def small_case(m, dtype, with_inf, rows=3000, seed=5):
    rng = np.random.default_rng([seed, m, int(with_inf), int(dtype == np.float64)])
    P, col = pr.tight_pssm(rng, m, with_inf)
    s = pack.pack(profiles=pr.tight_records(rng, pr.record_lengths(rng, m, max(rows, 3 * m)), col, dtype), profile_dtype=dtype)
    return s, P


# ---------------------------------------------------------------------------
# the helper against rationals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 7, 12, 40])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("special", [0.0, 0.05, 0.3])
def test_exact_struct_equals_the_rational_sum(oracle, m, dtype, special):
    rng = np.random.default_rng([11, m, int(special * 100), int(dtype == np.float64)])
    profs = []
    for L in (0, m - 1, m, 300, 1, 257):
        p = rng.dirichlet(np.full(7, 0.3), size=L) if L else np.zeros((0, 7))
        p[p < 0.05] = 0.0
        profs.append(p.astype(dtype))
    s = pack.pack(profiles=profs, profile_dtype=dtype)
    if special:
        s.profile[rng.integers(0, s.n_pos, size=4), rng.integers(0, 7, size=4)] = [np.nan, np.inf, -np.inf, 1e-30]
    P = rng.normal(-1, 3, size=(m, 7))
    mask = rng.random(P.shape) < special
    P[mask] = rng.choice(SPECIAL, size=int(mask.sum()))
    res = pr.exact_struct(s.profile, P)
    want_ref = oracle.stream_struct(s.profile, P)
    seen = set()
    for p in np.concatenate([rng.choice(s.n_pos, size=80, replace=False), np.arange(s.n_pos - m - 2, s.n_pos)]):
        ex, A, cls = pr.fraction_struct(s.profile, P, int(p))
        seen.add(cls)
        assert res.cls[p] == cls, (p, cls)
        if cls == pr.OUT:
            assert math.isnan(res.exact[p]) and math.isnan(want_ref[p])
        elif cls == pr.TIGHT:
            assert res.exact[p] == ex, (p, res.exact[p], ex)                 # correctly rounded: the same double
            assert abs(res.A[p] - A) <= 1e-12 * A, (p, res.A[p], A)
        else:                                                                # the reference's own value, bit for bit
            assert res.exact[p] == want_ref[p] and res.A[p] == 0
    assert (pr.TIGHT in seen or (special == 0.3 and m == 40)) and (pr.OUT in seen or m == 1)      # (40 rows at 30 % special cells: every window saturates)
    # positions= scores the same windows
    pick = np.array([0, 5, s.n_pos - 1, 17])
    sub = pr.exact_struct(s.profile, P, positions=pick)
    assert np.array_equal(sub.exact, res.exact[pick], equal_nan=True) and np.array_equal(sub.cls, res.cls[pick])


def test_integer_path_equals_rationals_on_extreme_cells():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    r = rng.random(84) * rng.choice([1.0, 1e-300, 1e-30, 0.0], size=84)
    p = rng.normal(0, 3, size=84) * rng.choice([1.0, 1e-300, -1e300, 1e300], size=84)
    total = sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(r, p))
    mag = sum(abs(Fraction(float(a)) * Fraction(float(b))) for a, b in zip(r, p))
    assert pr._exact_ints(r, p) == (float(total), float(mag))


# ---------------------------------------------------------------------------
# correct evaluations pass
# ---------------------------------------------------------------------------
def fma(a, b, c):
    """the rounded exact a * b + c"""
    p, e = pr.two_prod(np.float64(a), np.float64(b))
    return math.fsum((float(p), float(e), c))


def fma_order_scores(profile, P, positions, chained):
    """the kernels' order: per row a multiply and six FMAs; chained straight into the window sum (finite PSSM), or a
    row-dot that goes through nan_to_num and is added (any PSSM)"""
    m = P.shape[0]
    out = []
    for p in positions:
        R = np.asarray(profile[p:p + m], dtype=np.float64)
        score = 0.0
        for j in range(m):
            if chained:
                for k in range(7):
                    score = float(R[j, k] * P[j, k]) if j == 0 and k == 0 else fma(R[j, k], P[j, k], score)
                continue
            with np.errstate(all="ignore"):
                ref_d = pr._row_dots(R[None, j:j + 1], P[j:j + 1])[0, 0]
            if not np.isfinite(ref_d):                       # the class is the order's business, not the rounding's
                d = 0.0 if np.isnan(ref_d) else math.copysign(np.finfo(np.float64).max, ref_d)
            else:
                d = float(R[j, 0] * P[j, 0])
                for k in range(1, 7):
                    d = fma(R[j, k], P[j, k], d)
            score += d
        out.append(score)
    return np.array(out)


@pytest.mark.parametrize("m", WIDTHS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("with_inf", [False, True])
def test_the_oracle_and_the_fma_order_are_inside_the_bound(oracle, m, dtype, with_inf):
    s, P = small_case(m, dtype, with_inf)
    worst, share = pr.assert_struct_tight(oracle.stream_struct(s.profile, P), s.profile, P, in_record=s.window_mask(m))
    assert share >= pr.MIN_TIGHT_SHARE and worst <= 1.0
    rng = np.random.default_rng(m)
    inside = np.flatnonzero(s.window_mask(m))
    pos = np.sort(rng.choice(inside, size=min(inside.size, max(20, 4000 // m)), replace=False))
    for chained in ([True, False] if not with_inf else [False]):
        got = fma_order_scores(s.profile, P, pos, chained)
        w, _ = pr.assert_struct_tight(got, s.profile, P, positions=pos)
        assert w <= 1.0


# ---------------------------------------------------------------------------
# wrong evaluations do not
# ---------------------------------------------------------------------------
def numpy_scores(profile, P, row_dot=None, acc=np.float64):
    """the reference's order in numpy with a hook on the row-dots [n][m] and on the accumulator's type"""
    p64 = np.asarray(profile, dtype=np.float64)
    n, m = p64.shape[0], P.shape[0]
    out = np.full(n, np.nan)
    if n < m:
        return out
    R = p64[np.arange(n - m + 1)[:, None] + np.arange(m)[None, :]]
    with np.errstate(all="ignore"):
        d = pr._row_dots(R, P) if row_dot is None else row_dot(R, P)
        score = np.zeros(n - m + 1, dtype=acc)
        for j in range(m):
            score = score + np.nan_to_num(d[:, j]).astype(acc)
    out[:n - m + 1] = score.astype(np.float64)
    return out


def rejected(got, s, P):
    with pytest.raises(AssertionError):
        pr.assert_struct_tight(got, s.profile, P)
    return True


@pytest.mark.parametrize("m", [1, 7, 12, 18, 24])
def test_float32_mutants_pass_1e_6_and_fail_the_bound(oracle, m):
    """the gap: rows or PSSM rounded to float32 are inside the contract's 1e-6 at these widths"""
    s, P = small_case(m, np.float64, False, rows=6000)
    want = oracle.stream_struct(s.profile, P)
    assert np.array_equal(numpy_scores(s.profile, P), want, equal_nan=True)          # the hook-free form IS the oracle
    rows32 = oracle.stream_struct(s.profile.astype(np.float32), P)
    pssm32 = oracle.stream_struct(s.profile, P.astype(np.float32).astype(np.float64))
    for got in (rows32, pssm32):
        assert_struct_close(got, want)                       # accepted today
        assert rejected(got, s, P)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_arithmetic_mutants_are_rejected(oracle, dtype):
    m = 12
    s, P = small_case(m, dtype, False, rows=6000)
    want = oracle.stream_struct(s.profile, P)
    pr.assert_struct_tight(want, s.profile, P)
    assert rejected(numpy_scores(s.profile, P, acc=np.float32), s, P)               # float accumulator
    assert rejected(oracle.stream_struct(s.profile, P.astype(np.float32).astype(np.float64)), s, P)
    # one term of at least median size dropped, in every window
    def drop_median_term(R, Pm):
        prod = R * Pm[None]
        flat = np.abs(prod).reshape(prod.shape[0], -1)
        k = np.argsort(flat, axis=1)[:, flat.shape[1] // 2 + 7 * m // 4]          # above the median of all 7 m terms
        lost = np.take_along_axis(prod.reshape(prod.shape[0], -1), k[:, None], axis=1)[:, 0]
        d = pr._row_dots(R, Pm)
        d[:, 0] -= lost
        return d
    assert rejected(numpy_scores(s.profile, P, row_dot=drop_median_term), s, P)
    shifted = want.copy()
    shifted[:-1] = want[1:]                                                         # the window one row further on
    assert rejected(shifted, s, P)
    # ... and each of them in a SINGLE window is enough
    one = want.copy()
    p = int(np.flatnonzero(s.window_mask(m))[1234])
    one[p] = np.float64(np.float32(one[p]))
    assert rejected(one, s, P)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m", [7, 12, 24])
def test_row_rule_mutants_are_rejected(oracle, m, dtype):
    s, P = small_case(m, dtype, True, rows=6000)
    want = oracle.stream_struct(s.profile, P)
    worst, share = pr.assert_struct_tight(want, s.profile, P, in_record=s.window_mask(m))
    assert share >= pr.MIN_TIGHT_SHARE

    def keep_finite_terms(R, Pm):                # a 0 * -inf row keeps its finite terms instead of contributing 0
        prod = R * Pm[None]
        prod = np.where(np.isnan(prod), 0.0, prod)
        return prod.sum(axis=-1)
    assert rejected(numpy_scores(s.profile, P, row_dot=keep_finite_terms), s, P)

    def saturated_is_zero(R, Pm):                # a -inf row-dot treated like a NaN one
        d = pr._row_dots(R, Pm)
        return np.where(np.isinf(d), 0.0, d)
    assert rejected(numpy_scores(s.profile, P, row_dot=saturated_is_zero), s, P)
    if dtype == np.float64:
        assert rejected(oracle.stream_struct(s.profile.astype(np.float32), P), s, P)


# ---------------------------------------------------------------------------
# the input condition of test_gpu_precision.py, from the rules alone
# ---------------------------------------------------------------------------
def test_existing_inf_draw_is_mostly_saturated():
    """why the precision cases need inputs of their own: -inf cells drawn per cell over dirichlet rows leave a few per cent"""
    rng = np.random.default_rng(512)
    m = 12
    profs = []
    for _ in range(12):
        p = rng.dirichlet(np.full(7, 0.3), size=int(rng.integers(200, 2501)))
        p[p < 0.02] = 0.0
        profs.append((p / p.sum(axis=1, keepdims=True)).astype(np.float32))
    s = pack.pack(profiles=profs)
    P = rng.normal(-1, 2.5, size=(m, 7))
    P[rng.random((m, 7)) < 1.0 / m] = -np.inf
    assert np.isinf(P).sum() >= 3
    share, _ = pr.tight_share(s.profile, P, s.window_mask(m))
    assert share < 0.2


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_gpu_case_is_mostly_tight(dtype):
    for with_inf in (False, True):
        for m in sorted(set(pr.GENERIC_WIDTHS + pr.FIXED_WIDTHS + pr.WIDE_WIDTHS + [12, 100])):
            s, P, mask = pr.precision_case(m, dtype, with_inf, with_codes=True)
            share, _ = pr.tight_share(s.profile, P, mask)
            assert share >= pr.MIN_TIGHT_SHARE and mask.sum() >= 500, (m, with_inf, share)
            assert (s.lengths == 0).any() and (s.lengths == max(m - 1, 0)).any()      # empty records, records shorter than the PFM
        for n in (1, 2, 9, 16, 25, 33):
            s, LP, mask = pr.precision_case(12, dtype, with_inf, n_motifs=n, with_codes=True)
            for k in range(n):
                assert pr.tight_share(s.profile, LP[k], mask)[0] >= pr.MIN_TIGHT_SHARE, (n, k)
        for m in (12, 24):
            for extra in pr.TAIL_EXTRAS:
                streams, P = pr.tail_case(m, dtype, with_inf, extra)
                tight = total = 0
                for s in streams:
                    mask = s.window_mask(m)
                    share, _ = pr.tight_share(s.profile, P, mask)
                    tight += share * mask.sum()
                    total += mask.sum()
                assert total == 0 or tight >= pr.MIN_TIGHT_SHARE * total, (m, extra)
