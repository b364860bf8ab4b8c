"""The joint credit tables of k_pair_cred_sum (pfmscan_debug_pair_credits), checked EXHAUSTIVELY on a GPU-less host in the
style of tests/test_library_credits.py: one 16-bit credit sum per window over BOTH code streams, the joint threshold folded
into row 0.  No window whose printed LogOdds.SeqStruct passes may be dropped -- for every window of (4 letters + foreign) x
(7 codes + foreign) up to width 3, for 10^6 random windows of widths 4..12, with -inf / NaN / +inf cells, and with thr_sum
ON and one ulp either side of printed sums -- the filter must reject most windows on random tables, and every switch-off
must switch it off."""
import itertools

import numpy as np
import pytest

from pairsum_helpers import printed_sum, table
from rnascan_amd import _lib

SEP = 7


def _scores(T1, T2, c1, c2):
    """float32 of the sequential fp64 sequence sum, the sequential fp64 structure sum (matrix.py:25-43), per window"""
    s1, s2 = np.zeros(c1.shape[0]), np.zeros(c1.shape[0])
    with np.errstate(invalid="ignore"):
        for j in range(T1.shape[0]):
            s1 = s1 + T1[j, c1[:, j]]
            s2 = s2 + T2[j, c2[:, j]]
        return s1.astype(np.float32), s2


def _credit_sums(cr, c1, c2):
    tot = np.zeros(c1.shape[0], dtype=np.int64)
    for j in range(c1.shape[1]):
        tot += cr["seq"][j, c1[:, j]].astype(np.int64) + cr["struct"][j, c2[:, j]].astype(np.int64)
    assert tot.max() < 65536, "a credit sum leaves its 16 bits"
    return tot


def _passes(f, st, printed, T):
    with np.errstate(invalid="ignore"):
        return (f > -np.inf) & (st > -np.inf) & (printed > T)


def _check(T1, T2, c1, c2, f, st, printed, T):
    cr = _lib.debug_pair_credits(T1, T2, T)
    want = _passes(f, st, printed, T)
    if cr["mode"] == 3:
        return cr, want, None
    surv = _credit_sums(cr, c1, c2) >= 32768
    assert surv[want].all(), (T, int((want & ~surv).sum()), "windows whose printed sum passes were dropped")
    return cr, want, surv


def _all_windows(m):
    one = list(itertools.product([0, 1, 2, 3, SEP], range(8)))         # (sequence code, structure code) of one position
    w = np.array(list(itertools.product(one, repeat=m)), dtype=np.int64)      # [n][m][2]
    return w[:, :, 0], w[:, :, 1]


def _planted(printed, want_n, rng):
    fin = np.unique(printed[np.isfinite(printed)])
    picks = rng.choice(fin, size=min(want_n, fin.size), replace=False)
    out = []
    for p in picks:
        out += [float(p), float(np.nextafter(p, -np.inf)), float(np.nextafter(p, np.inf))]
    return out


@pytest.mark.parametrize("cells", ["finite", "neg_inf_nan"])
@pytest.mark.parametrize("m", [1, 2, 3])
def test_every_window_up_to_width_3(m, cells):
    rng = np.random.default_rng(40 + m)
    kw = dict(neg_inf=0.15, nan=0.1) if cells == "neg_inf_nan" else {}
    for rep in range(3):
        T1, T2 = table(rng, m, 4, **kw), table(rng, m, 7, dyadic=(rep == 1), **kw)
        c1, c2 = _all_windows(m)
        f, st = _scores(T1, T2, c1, c2)
        printed = printed_sum(f, st)
        if not np.isfinite(printed).any():
            continue
        rejected = total = 0
        for T in _planted(printed, 12, rng) + [float(np.round(np.nanmax(printed[np.isfinite(printed)]) - 0.5, 3)), -1e300, 1e300]:
            cr, want, surv = _check(T1, T2, c1, c2, f, st, printed, T)
            assert cr["mode"] in (1, 2)
            rejected += int((~surv).sum())
            total += surv.size
        assert rejected > 0.3 * total


@pytest.mark.parametrize("m", range(4, 13))
def test_a_million_random_windows(m):
    rng = np.random.default_rng(60 + m)
    n = 1_000_000
    T1, T2 = table(rng, m, 4), table(rng, m, 7, dyadic=(m % 3 == 0))
    if m % 4 == 0:
        T1[1, 2], T2[m - 1, 4], T2[0, 0] = -np.inf, np.nan, -np.inf
    c1 = rng.integers(0, 4, size=(n, m))
    c2 = rng.integers(0, 7, size=(n, m))
    c1[rng.random((n, m)) < 0.002] = SEP
    c2[rng.random((n, m)) < 0.002] = SEP
    f, st = _scores(T1, T2, c1, c2)
    printed = printed_sum(f, st)
    top = np.sort(printed[np.isfinite(printed)])
    sparse = float(top[-100])                                   # a 10^-4 hit rate: ON a printed sum
    for T in (sparse, float(np.nextafter(sparse, -np.inf)), float(np.nextafter(sparse, np.inf)), float(np.round(sparse, 2)), float(top[-20000])):
        cr, want, surv = _check(T1, T2, c1, c2, f, st, printed, T)
        assert cr["mode"] in (1, 2) and want.sum() > 0
        assert surv.mean() <= max(40 * want.mean(), cr["survive"] * 3 + 1e-3), (m, T, surv.mean(), want.mean())
    # not vacuous at the sparse threshold: most windows go, and the prediction (uniform letters) says so too
    cr, want, surv = _check(T1, T2, c1, c2, f, st, printed, sparse)
    assert surv.mean() < 0.05 and cr["mode"] == 1 and cr["survive"] < 1.0 / 32.0
    # the folded threshold lies below thr_sum by the cheap test's margin and a little more, never above
    assert sparse - 0.0011 - 1e-5 * (1 + abs(sparse)) < cr["thr_joint"] < sparse - 0.001
    assert cr["slack"] == pytest.approx(2 * m * cr["quantum"]) and 0 < cr["quantum"] < 0.2


def test_switch_offs_and_the_dense_verdict():
    rng = np.random.default_rng(7)
    m = 8
    T1, T2 = table(rng, m, 4), table(rng, m, 7)
    assert _lib.debug_pair_credits(T1, T2, 8.0)["mode"] in (1, 2)
    # a threshold most windows pass: dense, the exact kernel's
    dense = _lib.debug_pair_credits(T1, T2, -30.0)
    assert dense["mode"] == 2 and dense["survive"] > 1.0 / 32.0
    for side in (0, 1):                                          # a +inf cell on either side: no bound, no prefilter
        A, B = T1.copy(), T2.copy()
        (A, B)[side][3, 1] = np.inf
        off = _lib.debug_pair_credits(A, B, 8.0)
        assert off["mode"] == 3 and np.isinf(off["slack"]) and np.isinf(off["quantum"]) and not off["seq"].any() and not off["struct"].any()
    big = T1.copy()
    big[0, 0] = 3.1e35                                           # letter sums beyond ROUND3_SAFE: the round3 bound does not hold
    assert _lib.debug_pair_credits(big, T2, 8.0)["mode"] == 3
    huge = T2.copy()
    huge[:, :7] = 1.7e308                                        # the quantum is not finite
    assert _lib.debug_pair_credits(T1, huge, 8.0)["mode"] == 3
    assert _lib.debug_pair_credits(T1, T2, -np.inf)["mode"] == 3  # no joint threshold: nothing to fold in
    nothing = _lib.debug_pair_credits(T1, T2, np.inf)            # nothing exceeds +inf: no credit at all
    assert nothing["mode"] == 1 and not nothing["seq"].any() and not nothing["struct"].any()
    with pytest.raises(ValueError):
        _lib.debug_pair_credits(T1, T2, np.nan)
    with pytest.raises(ValueError):
        _lib.debug_pair_credits(table(rng, 33, 4), table(rng, 33, 7), 1.0)
    # -inf / NaN cells and foreign letters get no credit beyond the folded row-0 constant
    A = T1.copy()
    A[2, 1], A[4, 3] = -np.inf, np.nan
    cr = _lib.debug_pair_credits(A, T2, 8.0)
    assert cr["seq"][2, 1] == 0 and cr["seq"][4, 3] == 0 and not cr["seq"][1:, 4:].any() and not cr["struct"][:, 7].any()
    assert len(set(cr["seq"][0, 4:].tolist())) == 1 and cr["seq"][0, 4] <= cr["seq"][0, :4].min()


# ---- thr_eff of the two-FASTA library route (pfmscan_library_letters_sum_thresholds) ------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3])
def test_library_thr_eff_is_a_superset_threshold_and_its_bound_is_attained(m):
    """every window of the exhaustive set whose printed sum passes has (double) f > thr_eff; the window made of the structure
    table's row maxima scores exactly U2, so thr_eff lies within the margins (~0.0011) of T - U2: the bound is tight"""
    rng = np.random.default_rng(80 + m)
    for rep in range(4):
        T1 = table(rng, m, 4, neg_inf=0.1 if rep == 2 else 0.0)
        T2 = table(rng, m, 7, dyadic=(rep == 1), neg_inf=0.1 if rep == 3 else 0.0, nan=0.1 if rep == 3 else 0.0)
        c1, c2 = _all_windows(m)
        f, st = _scores(T1, T2, c1, c2)
        printed = printed_sum(f, st)
        fin = np.isfinite(printed)
        if not fin.any():
            continue
        U2 = st[np.isfinite(st)].max()                          # attained by a real window
        for T in _planted(printed, 10, rng) + [float(np.round(printed[fin].max() - 0.3, 3))]:
            for thr_seq in (-np.inf, float(np.median(f[np.isfinite(f)]))):
                eff = _lib.library_letters_sum_thresholds(T1[None], T2[None], thr_seq, T)[0]
                want = _passes(f, st, printed, T) & (f.astype(np.float64) > thr_seq)
                assert (f.astype(np.float64)[want] > eff).all(), (m, T, thr_seq)
                assert eff >= thr_seq
                e = T - U2
                assert eff == thr_seq or e - 0.0011 - 1e-6 * (1 + abs(T) + abs(U2)) < eff < e - 0.001, (eff, e)
        # not vacuous: at a T near the top most windows fall below thr_eff
        top = float(np.sort(printed[fin])[-3])
        eff = _lib.library_letters_sum_thresholds(T1[None], T2[None], -np.inf, top)[0]
        assert (f[np.isfinite(f)].astype(np.float64) <= eff).mean() > 0.3 or m == 1


def test_library_thr_eff_switch_offs():
    rng = np.random.default_rng(90)
    m = 8
    T1, T2 = table(rng, m, 4), table(rng, m, 7)
    thr = lambda A, B, ts, tj: _lib.library_letters_sum_thresholds(A[None], B[None], ts, tj)[0]
    assert np.isfinite(thr(T1, T2, -np.inf, 5.0)) and thr(T1, T2, 100.0, 5.0) == 100.0
    B = T2.copy()
    B[2, 3] = np.inf                                             # no bound on the structure score
    assert np.isneginf(thr(T1, B, -np.inf, 5.0)) and thr(T1, B, 1.5, 5.0) == 1.5
    for bad in (np.inf, np.nan):                                 # the prefilter is off for such a sequence table anyway
        A = T1.copy()
        A[1, 2] = bad
        assert np.isneginf(thr(A, T2, -np.inf, 5.0))
    A = T1.copy()
    A[0, 0] = 3.1e35                                             # beyond ROUND3_SAFE
    assert np.isneginf(thr(A, T2, -np.inf, 5.0))
    assert np.isneginf(thr(T1, T2, -np.inf, -np.inf)) and thr(T1, T2, 2.0, -np.inf) == 2.0      # no joint threshold
    assert thr(T1, T2, -np.inf, np.inf) == np.inf                # nothing exceeds +inf
    B = T2.copy()
    B[3, :] = np.nan                                             # a row without a finite cell: every window is NaN, it adds nothing to U2
    assert np.isfinite(thr(T1, B, -np.inf, 5.0))
    with pytest.raises(ValueError):
        _lib.library_letters_sum_thresholds(T1[None], T2[None], np.nan, 1.0)
