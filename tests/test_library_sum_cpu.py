"""The letters threshold a PFM library's prefilter is built for under a joint threshold on LogOdds.SeqStruct
(pfmscan_library_sum_thresholds; the bound is derived in rnascan_amd/csrc/pfmscan_exact.hpp), on a GPU-less host.

Soundness by brute force: the oracle scores every window of random and adversarial streams; every window whose three
predicates hold -- seq > thr_seq, and the printed sum float64(round(float32 seq, 3)) + struct > T -- must have
float64(seq) > thr_eff, or the library kernel's integer prefilter, built for thr_eff, could drop a hit.  The streams put
the structure score ON the bound (rows one-hot on each PSSM row's largest cell) and T on, and one ulp beside, the printed
sums of such windows."""
import numpy as np
import pytest

from oracle import oracle
from rnascan_amd import _lib

SEP = 7
ROUND3_SAFE = 3.0e35
STRUCT_ROW_MAX = 1024.0


def row_bound_np(codes, profile):
    """the numpy restatement of pfmscan_profile_row_bound_*: the largest fp64 row sum (c ascending) over the rows whose code
    is not 7, inf when one of them holds a NaN, infinite or negative entry, 0.0 when no row counts"""
    p = np.asarray(profile)
    keep = np.ones(p.shape[0], bool) if codes is None else (np.asarray(codes) & 7) != SEP
    r = p[keep].astype(np.float64)
    if not r.shape[0]:
        return 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        s = r[:, 0].copy()
        for c in range(1, 7):
            s = s + r[:, c]
        bad = ~((r >= 0.0) & (r < np.inf)).all(axis=1)
    s[bad] = np.inf
    return float(max(0.0, s.max()))          # (a row of -0.0 entries leaves +0.0, as the kernel's `x > best`)


def struct_band(P):
    m = P.shape[0]
    return 24.0 * m * 2.0 ** -53 * STRUCT_ROW_MAX * float(np.abs(P[np.isfinite(P)]).sum())


def printed_sum(sq, st):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.round(sq, 3).astype(np.float64) + st


def letter_tables(rng, n, m, kind):
    T = np.full((n, m, 8), np.nan)
    if kind == "normal":
        T[:, :, :4] = rng.normal(0, 2, size=(n, m, 4))
    else:                                      # maximal |L| with either sign: the |f| term of the bound at work
        T[:, :, :4] = rng.choice([-1.0, 1.0], size=(n, m, 4)) * rng.uniform(20.0, 60.0, size=(n, m, 4))
    return T


def struct_pssms(rng, n, m, cells):
    P = rng.normal(-1, 2.5, size=(n, m, 7))
    if cells == "inf":
        for k in range(n):
            at = rng.choice(m * 7, size=min(3, m * 7 - 1), replace=False)
            P[k].reshape(-1)[at[:-1]] = -np.inf
            P[k].reshape(-1)[at[-1]] = np.nan
    return P


def argmax_columns(P):
    """per PSSM row the column of its largest cell that is neither NaN nor -inf (0 when there is none)"""
    Q = np.where(np.isnan(P) | (P == -np.inf), -np.inf, P)
    return np.argmax(Q, axis=1)


def make_streams(rng, T, P, m):
    """(name, codes, profile) of ~1500 positions each; the adversarial ones aim at motif 0"""
    n_pos = 1500
    out = []

    def codes_random():
        c = rng.integers(0, 4, size=n_pos).astype(np.uint8)
        c[rng.random(n_pos) < 0.004] = SEP
        return c

    def codes_extreme(sign):                  # every position the letter with the largest (smallest) log-odds at its row of motif 0
        j = np.arange(n_pos) % m
        L = T[0][:, :4]
        c = (np.argmax(L, axis=1) if sign > 0 else np.argmin(L, axis=1))[j].astype(np.uint8)
        c[rng.random(n_pos) < 0.002] = SEP
        return c

    dir32 = rng.dirichlet(np.full(7, 0.3), size=n_pos).astype(np.float32)            # float32-rounded draws: sums beside 1 by ulps
    assert (dir32.astype(np.float64).sum(axis=1) > 1.0).any()
    out.append(("dirichlet32", codes_random(), dir32))
    p = rng.dirichlet(np.full(7, 0.3), size=n_pos)
    p[p < 0.02] = 0.0
    p /= p.sum(axis=1, keepdims=True)
    out.append(("random64", codes_random(), p))
    cols = argmax_columns(P[0])
    for name, scale, dtype in (("onehot", 1.0, np.float32), ("rows-of-sum-3", 3.0, np.float64)):
        q = np.zeros((n_pos, 7), dtype=dtype)
        # windows starting at multiples of m score exactly S * the sum of the non-negative row maxima (a row whose largest
        # cell is negative does best with an all-zero profile row)
        best = np.where(np.isnan(P[0]) | (P[0] == -np.inf), -np.inf, P[0]).max(axis=1)
        q[np.arange(n_pos), cols[np.arange(n_pos) % m]] = np.where(best > 0.0, scale, 0.0)[np.arange(n_pos) % m]
        if name == "rows-of-sum-3":
            mix = rng.random(n_pos) < 0.3                             # other rows that sum to exactly 3
            q[mix] = 0.0
            q[mix, :3] = 1.0
        out.append((name + "+max-letters", codes_extreme(+1), q))
        out.append((name + "+min-letters", codes_extreme(-1), q.copy()))
        out.append((name, codes_random(), q.copy()))
    z = rng.dirichlet(np.full(7, 0.3), size=n_pos).astype(np.float32)
    z[rng.random(n_pos) < 0.5] = 0.0                                  # all-zero rows
    out.append(("zero-rows", codes_random(), z))
    return out


def thresholds_on_sums(rng, sums_by_motif):
    """per motif a T ON a printed sum (the largest ones and random ones), with its two neighbours"""
    picks = []
    for which in ("top", "high", "random"):
        on = np.empty(len(sums_by_motif))
        for k, s in enumerate(sums_by_motif):
            v = np.sort(s[np.isfinite(s) & (np.abs(s) < 1e300)])
            if not v.size:
                on[k] = 0.0
            elif which == "top":
                on[k] = v[-1]
            elif which == "high":
                on[k] = v[max(0, v.size - 1 - int(rng.integers(1, 6)))]
            else:
                on[k] = v[int(rng.integers(0, v.size))]
        picks += [on, np.nextafter(on, -np.inf), np.nextafter(on, np.inf)]
    return picks


@pytest.mark.parametrize("cells", ["finite", "inf"])
@pytest.mark.parametrize("letters", ["normal", "extreme"])
@pytest.mark.parametrize("m,n", [(1, 13), (2, 7), (5, 1), (12, 13), (18, 5), (33, 2)])
def test_no_window_that_passes_lies_at_or_below_thr_eff(m, n, letters, cells):
    rng = np.random.default_rng(1000 * m + 10 * n + (1 if letters == "extreme" else 0) + (2 if cells == "inf" else 0))
    T, P = letter_tables(rng, n, m, letters), struct_pssms(rng, n, m, cells)
    n_checked = n_tight = 0
    for name, codes, prof in make_streams(rng, T, P, m):
        S = row_bound_np(codes, prof)
        assert np.isfinite(S) and S >= 1.0 - 1e-6, name
        sq = [oracle.stream_seq(codes, T[k]) for k in range(n)]
        st = [oracle.stream_struct(prof, P[k]) for k in range(n)]
        sums = [printed_sum(a, b) for a, b in zip(sq, st)]
        for Tsum in thresholds_on_sums(rng, sums):
            for thr_seq in (-np.inf, float(np.nanquantile(sq[0].astype(np.float64), 0.6))):
                eff = _lib.library_sum_thresholds(T, P, thr_seq, Tsum, S)
                assert (eff >= thr_seq).all()
                for k in range(n):
                    with np.errstate(invalid="ignore"):
                        hit = (sq[k] > thr_seq) & (sums[k] > Tsum[k])
                        f = sq[k][hit].astype(np.float64)
                    assert (f > eff[k]).all(), (name, k, Tsum[k], thr_seq, eff[k], f.min())
                    n_checked += int(hit.sum())
                    if thr_seq == -np.inf and f.size and np.isfinite(eff[k]):
                        n_tight += int((f - eff[k] < 0.01).any())
    assert n_checked > 100
    if cells == "finite" and letters == "normal":
        assert n_tight > 0, "no window came within 0.01 of its thr_eff: the adversarial streams do not reach the bound"


def test_switch_off_conditions_give_thr_seq_back():
    rng = np.random.default_rng(5)
    n, m = 4, 12
    T, P = letter_tables(rng, n, m, "normal"), struct_pssms(rng, n, m, "finite")
    thr_seq = np.array([-np.inf, -3.0, 0.5, -np.inf])
    Tsum = np.array([1.0, -2.0, 3.0, -4.0])
    base = _lib.library_sum_thresholds(T, P, thr_seq, Tsum, 1.0)
    assert np.isfinite(base).all() and (base >= thr_seq).all()
    # S = inf: no promise about the rows
    assert np.array_equal(_lib.library_sum_thresholds(T, P, thr_seq, Tsum, np.inf), thr_seq)
    # a +inf PSSM cell: no bound for that motif, the others keep theirs
    P2 = P.copy()
    P2[1, 3, 2] = np.inf
    got = _lib.library_sum_thresholds(T, P2, thr_seq, Tsum, 1.0)
    assert got[1] == thr_seq[1] and np.array_equal(got[[0, 2, 3]], base[[0, 2, 3]])
    # F_k > ROUND3_SAFE: the round3 bound does not hold
    T2 = T.copy()
    T2[0, 0, 1] = 2.0 * ROUND3_SAFE
    got = _lib.library_sum_thresholds(T2, P, thr_seq, Tsum, 1.0)
    assert got[0] == thr_seq[0] and np.array_equal(got[1:], base[1:])
    # +inf / NaN letter sums (the prefilter is off for such a motif anyway)
    for bad in (np.inf, np.nan):
        T3 = T.copy()
        T3[3, 5, 0] = bad
        got = _lib.library_sum_thresholds(T3, P, thr_seq, Tsum, 1.0)
        assert got[3] == thr_seq[3] and np.array_equal(got[:3], base[:3])
    # -inf letters and -inf / NaN PSSM cells do NOT switch it off
    T4, P4 = T.copy(), P.copy()
    T4[2, 1, 3] = -np.inf
    P4[2, 0, 0], P4[2, 4, 6] = -np.inf, np.nan
    assert np.isfinite(_lib.library_sum_thresholds(T4, P4, -np.inf, Tsum, 1.0)).all()
    # T = -inf rejects nothing: thr_seq; T = +inf: nothing passes
    assert np.array_equal(_lib.library_sum_thresholds(T, P, thr_seq, -np.inf, 1.0), thr_seq)
    assert (_lib.library_sum_thresholds(T, P, thr_seq, np.inf, 1.0) == np.inf).all()
    # a letter table with a fifth letter is not a library's (columns 4..7 must be NaN): refused
    T5 = T.copy()
    T5[1, 2, 4] = 0.5
    with pytest.raises(ValueError):
        _lib.library_sum_thresholds(T5, P, thr_seq, Tsum, 1.0)
    # NaN arguments are refused
    for args in ((np.nan, Tsum, 1.0), (thr_seq, np.nan, 1.0), (thr_seq, Tsum, np.nan)):
        with pytest.raises(ValueError):
            _lib.library_sum_thresholds(T, P, *args)


@pytest.mark.parametrize("m", [1, 5, 12, 33, 64])
def test_thr_eff_is_not_vacuous(m):
    """one-hot arg-max rows (S = 1): thr_eff >= T - U - struct_band - 0.0005 - the |f| term - a few ulps, every quantity
    computed here.  The |f| term is ROUND3_C 2^-24 F (1 + 2^-20), F = the sum of the rows' largest |log-odds|; the ulps: the
    host rounds each of its ~2 m + 16 operations away from the safe side by one."""
    rng = np.random.default_rng(40 + m)
    n = 6
    T, P = letter_tables(rng, n, m, "normal"), struct_pssms(rng, n, m, "finite")
    Tsum = rng.normal(0, 5, size=n)
    S = 1.0
    eff = _lib.library_sum_thresholds(T, P, -np.inf, Tsum, S)
    for k in range(n):
        U = S * float(np.maximum(P[k].max(axis=1), 0.0).sum())
        F = float(np.abs(T[k][:, :4]).max(axis=1).sum())
        f_term = 4.0 * 2.0 ** -24 * F * (1.0 + 2.0 ** -20)
        floor = Tsum[k] - U - struct_band(P[k]) - 0.0005 - f_term
        ulps = (2 * m + 16) * 2.0 ** -52 * (abs(Tsum[k]) + U + 1.0)
        assert eff[k] >= floor - ulps, (k, eff[k], floor, ulps)
        assert eff[k] <= Tsum[k] - U, "above the bound itself: not a superset filter"
        # and the one-hot window reaches the bound: its structure score is U up to rounding
        prof = np.zeros((m, 7), dtype=np.float32)
        prof[np.arange(m), np.argmax(P[k], axis=1)] = 1.0
        st = oracle.stream_struct(prof, P[k])[0]
        assert abs(st - float(P[k].max(axis=1).sum())) <= 1e-12 * m * 10 and st <= U + 1e-12
