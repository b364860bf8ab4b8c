"""The exact structure score of a window and the rounding-error bound a correct fp64 evaluation of it must meet.

A window's score is  sum_j nan_to_num(dot(profile[p + j, :], pssm[j, :]))  (rnascan.py:302-307): 7 m products r_jk * P_jk.
Any evaluation of that sum in IEEE fp64 in which a term passes through at most k roundings is within gamma(k) * A of
the exact sum, gamma(k) = k u / (1 - k u), u = 2^-53, A = sum |r_jk P_jk| (Higham, Accuracy and Stability of Numerical
Algorithms, sections 3.1 and 4.2).  The reference order (product rounded, k ascending, row-dot rounded, then added) has
k <= m + 6; the kernels' order (a multiply and six FMAs per row, chained through the window when the PSSM is finite) has
k <= 7 m; float32 rows convert to double exactly.  So  |score - exact| <= gamma(7 m) A  holds for every order in play,
and nothing has to be measured to set it.

Rows follow numpy.nan_to_num per row-dot: a row whose dot is NaN (a 0 * inf product, a NaN cell, a NaN profile entry,
+inf and -inf in one row) contributes 0 AS A WHOLE and leaves A; a row whose dot is +-inf becomes +-DBL_MAX and
saturates the window -- there the finite rows are absorbed, no tight bound exists and the comparison is the one
conftest.assert_struct_close makes.  A window that runs past the end of the stream scores NaN; the separator position
after a record is an all-zero profile row like any other (the structure kernels and the oracle score across it).

Plain numpy / Python: nothing here imports the library under test or the oracle."""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

from conftest import assert_struct_close

U = 2.0 ** -53
OUT, TIGHT, SATURATED = 0, 1, 2
_SPLIT = 134217729.0                       # 2^27 + 1 (Veltkamp)
_SAFE_LO, _SAFE_HI = 2.0 ** -450, 2.0 ** 450     # products and their error terms stay normal, the split cannot overflow
_DBL_MAX = np.finfo(np.float64).max

Exact = namedtuple("Exact", "exact A cls")


def gamma(k):
    return k * U / (1.0 - k * U)


def two_prod(a, b):
    """error-free product (Dekker): a * b == p + e exactly, for operands inside [_SAFE_LO, _SAFE_HI] or zero"""
    p = a * b
    t = _SPLIT * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLIT * b
    bh = t - (t - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _row_dots(R, P):
    """the reference's row-dots (products rounded, k ascending) of gathered rows R [c][m][7] with P [m][7] -> [c][m]"""
    with np.errstate(all="ignore"):
        prod = R * P[None]
        d = prod[..., 0].copy()
        for k in range(1, 7):
            d = d + prod[..., k]
    return d


def _exact_ints(r_terms, p_terms):
    """exact sum and exact sum of magnitudes of the products r * p, any finite doubles, in integer arithmetic ->
    (correctly rounded sum, rounded A)"""
    mr, er = np.frexp(np.asarray(r_terms, dtype=np.float64))
    mp, ep = np.frexp(np.asarray(p_terms, dtype=np.float64))
    mr = np.ldexp(mr, 53).astype(np.int64).tolist()
    mp = np.ldexp(mp, 53).astype(np.int64).tolist()
    e = (er.astype(np.int64) + ep.astype(np.int64) - 106).tolist()
    emin = min(e) if e else 0
    total = mag = 0
    for a, b, x in zip(mr, mp, e):
        if a and b:
            t = (a * b) << (x - emin)
            total += t
            mag += abs(t)
    scale = Fraction(2) ** emin

    def to_float(v):
        try:
            return float(Fraction(v) * scale)        # int / int true division: correctly rounded
        except OverflowError:
            return math.copysign(math.inf, v)
    return to_float(total), to_float(mag)


def exact_struct(profile, pssm, positions=None, classes_only=False, chunk_elems=1 << 21):
    """Per window (at `positions`, default every stream position): the correctly rounded exact score, A and the class.

    TIGHT      every row-dot finite or NaN: `exact` is the exact sum over the rows that count, rounded once
    SATURATED  some row-dot +-inf: `exact` is the score in the reference's own order (+-DBL_MAX-sized or +-inf)
    OUT        the window runs past the end of the stream: NaN
    Profile entries convert to double exactly; `pssm` is [m][7] float64.  `classes_only` skips the exact sums: `exact` then
    holds the reference-order score of every in-stream window (for thresholds and shares), A is 0."""
    P = np.ascontiguousarray(pssm, dtype=np.float64)
    prof = np.asarray(profile)
    assert prof.ndim == 2 and prof.shape[1] == 7 and P.ndim == 2 and P.shape[1] == 7
    p64 = prof.astype(np.float64)
    n, m = p64.shape[0], P.shape[0]
    pos = np.arange(n, dtype=np.int64) if positions is None else np.asarray(positions, dtype=np.int64)
    exact = np.full(pos.shape, np.nan)
    A = np.zeros(pos.shape)
    cls = np.full(pos.shape, OUT, dtype=np.int8)
    inside = np.flatnonzero(pos + m <= n)
    step = max(1, chunk_elems // (7 * m))
    j = np.arange(m, dtype=np.int64)
    for c0 in range(0, inside.size, step):
        sel = inside[c0:c0 + step]
        R = p64[pos[sel, None] + j[None, :]]                       # [c][m][7]
        d = _row_dots(R, P)
        counts = np.isfinite(d)                                    # a NaN row-dot: the row contributes 0
        sat = np.isinf(d).any(axis=1)
        with np.errstate(all="ignore"):
            ref = np.zeros(len(sel))
            for jj in range(m):                                    # the reference's order, for the saturated windows
                ref = ref + np.clip(np.where(np.isnan(d[:, jj]), 0.0, d[:, jj]), -_DBL_MAX, _DBL_MAX)
        cls[sel] = np.where(sat, SATURATED, TIGHT)
        if classes_only:
            exact[sel] = ref
            continue
        Rz = np.where(counts[..., None], R, 0.0)
        Pz = np.where(counts[..., None], P[None], 0.0)
        aR, aP = np.abs(Rz), np.abs(Pz)
        safe_el = (aR == 0) | (aP == 0) | ((aR >= _SAFE_LO) & (aR <= _SAFE_HI) & (aP >= _SAFE_LO) & (aP <= _SAFE_HI))
        safe = safe_el.all(axis=(1, 2))
        fast = ~sat & safe
        ex = np.empty(len(sel))
        Aw = np.zeros(len(sel))
        if fast.any():
            p, e = two_prod(Rz[fast], Pz[fast])
            parts = np.concatenate([p.reshape(p.shape[0], -1), e.reshape(e.shape[0], -1)], axis=1)
            ex[fast] = [math.fsum(row) for row in parts.tolist()]
            Aw[fast] = np.abs(p).sum(axis=(1, 2))
        for w in np.flatnonzero(~sat & ~safe):                     # 1e-300 / 1e300 cells: integers
            ex[w], Aw[w] = _exact_ints(Rz[w].ravel(), Pz[w].ravel())
        ex[sat] = ref[sat]
        exact[sel] = ex
        A[sel] = np.where(sat, 0.0, Aw)
    return Exact(exact, A, cls)


def fraction_struct(profile, pssm, p):
    """window p in rationals only, straight from the rules in the module text -> (exact, A, class); the slow witness
    exact_struct is tested against"""
    P = np.asarray(pssm, dtype=np.float64)
    prof = np.asarray(profile)
    m = P.shape[0]
    if p + m > prof.shape[0]:
        return math.nan, 0.0, OUT
    total = mag = Fraction(0)
    for j in range(m):
        row = [float(x) for x in prof[p + j]]
        cells = [float(x) for x in P[j]]
        with np.errstate(all="ignore"):
            prods = [float(np.float64(r) * np.float64(c)) for r, c in zip(row, cells)]
        if any(math.isnan(x) for x in prods) or (any(x == math.inf for x in prods) and any(x == -math.inf for x in prods)):
            continue                                               # NaN row-dot: contributes 0
        if any(math.isinf(x) for x in prods):
            return None, 0.0, SATURATED
        for r, c in zip(row, cells):
            t = Fraction(r) * Fraction(c)
            total += t
            mag += abs(t)
    return float(total), float(mag), TIGHT


def assert_struct_tight(got, profile, pssm, positions=None, in_record=None):
    """`got[i]` is the structure score of the window at positions[i] (default: all stream positions, in order).

    out-of-stream windows: NaN; tight windows: |got - exact| <= gamma(7 m) A (equality when A == 0); saturated windows:
    what conftest.assert_struct_close asks of them.  `exact` is the exact sum rounded once, so it is itself within u |S| of
    the sum S the bound is about.  `in_record` (bool per window) restricts the share's denominator to windows inside one
    record.  Returns (largest error / bound over the tight windows, share of the in-record windows that are tight)."""
    got = np.asarray(got, dtype=np.float64)
    m = np.asarray(pssm).shape[0]
    res = exact_struct(profile, pssm, positions)
    assert got.shape == res.exact.shape
    out, tight, sat = res.cls == OUT, res.cls == TIGHT, res.cls == SATURATED
    assert np.isnan(got[out]).all(), "a window past the end of the stream has a score"
    bound = gamma(7 * m) * res.A[tight]
    with np.errstate(invalid="ignore"):
        err = np.abs(got[tight] - res.exact[tight])
    bad = ~(err <= bound)                                          # (a NaN score is bad)
    worst = 0.0
    if err.size:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        worst = float(ratio.max())
    if bad.any():
        w = np.flatnonzero(tight)[np.flatnonzero(bad)]
        k = w[np.argmax(np.where(np.isnan(err[bad]), np.inf, err[bad] - bound[bad]))]
        where = k if positions is None else np.asarray(positions)[k]
        raise AssertionError("%d of %d tight windows outside gamma(%d) A; worst error/bound %.3g; window %d: got %r, exact %r, A %.3e"
                             % (bad.sum(), tight.sum(), 7 * m, worst, where, got[k], res.exact[k], res.A[k]))
    if sat.any():
        assert_struct_close(got[sat], res.exact[sat])
    base = ~out if in_record is None else (np.asarray(in_record, dtype=bool) & ~out)
    share = float((tight & base).sum()) / max(int(base.sum()), 1)
    return worst, share


# ---------------------------------------------------------------------------
# inputs of the precision tests: most windows tight, also under -inf cells
# ---------------------------------------------------------------------------
def tight_pssm(rng, m, with_inf):
    """normal cells; with_inf: 2-4 -inf cells (at most every second row, so that a narrow PFM keeps rows that count; one cell
    below four rows), ALL in one column -> (P, that column or None)"""
    P = rng.normal(-1, 2.5, size=(m, 7))
    if not with_inf:
        return P, None
    col = int(rng.integers(0, 7))
    P[inf_rows(rng, m), col] = -np.inf
    return P, col


def inf_rows(rng, m):
    return rng.choice(m, size=min(max(1, m // 2), int(rng.integers(2, 5))), replace=False)


def tight_records(rng, lengths, zero_col=None, dtype=np.float32):
    """per-record [L][7] probability rows (entries below 0.02 snapped to 0 as the parity tests do); `zero_col` is 0 in
    about nine rows of ten, so that most windows meet a -inf cell of that column with a 0 (the row then contributes 0:
    the rule under test) and few with a probability (the window saturates)"""
    out = []
    for L in lengths:
        p = rng.dirichlet(np.full(7, 0.3), size=L) if L else np.zeros((0, 7))
        if L:
            p[p < 0.02] = 0.0
            if zero_col is not None:
                p[rng.random(L) < 0.9, zero_col] = 0.0
            tot = p.sum(axis=1, keepdims=True)
            p = np.divide(p, tot, out=np.zeros_like(p), where=tot > 0)
        out.append(p.astype(dtype))
    return out


def record_lengths(rng, m, total):
    """record lengths summing to about `total` rows: empty records, records shorter than / as long as / one longer than the
    PFM, and long ones of ragged lengths"""
    lengths = [0, max(m - 1, 0), m, m + 1, 0, 1]
    while sum(lengths) < total:
        lengths.append(int(rng.integers(m, max(m + 2, min(2500, total // 3)))))
    order = rng.permutation(len(lengths))
    return [lengths[i] for i in order]


# the cases of test_gpu_precision.py; test_precision_cpu.py asserts the tight share of each from the rules above alone
GENERIC_WIDTHS = [1, 2, 3, 19, 24, 40, 64, 65, 100, 180]          # k_profile<V> (it takes widths up to 180)
FIXED_WIDTHS = list(range(4, 19))                                  # k_profile_fixed (test_gpu_parity.FIXED_WIDTHS)
WIDE_WIDTHS = [181, 200, 1500]                                     # k_wide
TAIL_EXTRAS = [0, 1, 2, 3, 5, 1791, 1792, 1793]                    # test_stream_tail_sizes
TAIL_BASES = [0, 11, 12, 13, 4096]
MIN_TIGHT_SHARE = 0.5


def case_rows(m):
    """stream rows of a case: 16 000 up to width 64 (15-20 k windows), fewer for wider PFMs -- the exact sum of a window
    costs 14 m parts -- but always several records longer than the PFM"""
    return 16000 if m <= 64 else max(4 * m + 2000, 16000 * 64 // m)


def precision_case(m, dtype, with_inf, seed=0, n_motifs=None, with_codes=False):
    """-> (Stream, P [m][7] or [n][m][7], in-record window mask).  The -inf cells of every PSSM of a case sit in ONE column,
    the column the profiles keep at 0 in most rows."""
    from rnascan_amd import pack
    rng = np.random.default_rng([seed, m, int(with_inf), int(np.dtype(dtype) == np.float64), n_motifs or 0])
    first, col = tight_pssm(rng, m, with_inf)
    P = first
    if n_motifs is not None:
        rest = [tight_pssm(rng, m, False)[0] for _ in range(n_motifs - 1)]
        for Q in rest:
            if with_inf:
                Q[inf_rows(rng, m), col] = -np.inf
        P = np.stack([first] + rest)
    lengths = record_lengths(rng, m, case_rows(m))
    profs = tight_records(rng, lengths, col, dtype)
    codes = None
    if with_codes:
        codes = [rng.integers(0, 4, size=L).astype(np.uint8) for L in lengths]
        for c in codes:
            c[rng.random(len(c)) < 0.002] = 7
    s = pack.pack(codes, profs, profile_dtype=dtype)
    return s, P, s.window_mask(m)


def tail_case(m, dtype, with_inf, extra):
    """one-record streams of TAIL_BASES + extra rows (a tile +- 1, tiny streams) -> list of Stream, P"""
    from rnascan_amd import pack
    rng = np.random.default_rng([77, m, int(with_inf), int(np.dtype(dtype) == np.float64), extra])
    P, col = tight_pssm(rng, m, with_inf)
    streams = [pack.pack(profiles=tight_records(rng, [b + extra], col, dtype), profile_dtype=dtype) for b in TAIL_BASES if b + extra]
    return streams, P


def tight_share(profile, pssm, in_record):
    """share of the in-record windows that are tight, and the reference-order score of every tight window of the stream (NaN
    elsewhere; the structure kernels score across the separator rows too): from the rules alone"""
    res = exact_struct(profile, pssm, classes_only=True)
    base = np.asarray(in_record, dtype=bool) & (res.cls != OUT)
    tight = base & (res.cls == TIGHT)
    return float(tight.sum()) / max(int(base.sum()), 1), np.where(res.cls == TIGHT, res.exact, np.nan)


def sample_positions(n_pos, m, rng, max_parts=40_000_000):
    """all stream positions when their exact sums fit the budget of parts, else a random sample plus both ends of the stream"""
    if n_pos * 14 * m <= max_parts:
        return None
    k = max(64, max_parts // (14 * m))
    ends = np.concatenate([np.arange(min(32, n_pos)), np.arange(max(n_pos - m - 32, 0), n_pos)])
    return np.unique(np.concatenate([ends, rng.choice(n_pos, size=min(k, n_pos), replace=False)]))
