"""A numpy restatement of the occupancy on averaged-structure profiles (include/pfmscan.h "occupancy on averaged-structure
profiles"; k_occ_profile_blocks in rnascan_amd/csrc/pfmscan_occupancy.hip): the marginal of a profile row under
a motif row, the term of a window in both modes, and -- imported from occupancy_rules, unchanged -- the summation tree.  No
tolerance in any of it: the GPU tests compare bit patterns.

numpy evaluates ``d + x * s`` as two ufunc calls over whole arrays, a rounded product and a rounded sum: nothing is fused.
"""
import numpy as np

from occupancy_rules import FANIN, SEP, U, same_bits, tree  # noqa: F401  (re-exported for the tests)
import occupancy_rules as orules

NSTRUCT = 7


# ---- the definitions -------------------------------------------------------------------------------------------------
def marginal(rows, s):
    """rows [n][7] (float32 rows are widened first, which is exact), s = one motif row [7] in the profile's stored column
    order -> d float64 [n]: d = r[0] * s[0], then d = d + r[c] * s[c] for c ascending, every operation rounded"""
    x = np.asarray(rows).astype(np.float64)
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = x[:, 0] * s[0]
        for c in range(1, NSTRUCT):
            d = d + x[:, c] * s[c]
    return d


def terms(profile, off, length, S, codes=None, R=None, marg=None):
    """the record's windows in order -> (t float64 [n_win] with +0.0 where the window has no term, has bool [n_win]).
    Structure only (R None): t = d(s, 0), then t = t * d(s + k, k); every window has a term and the codes are not read.
    Joint: the letter chain of occupancy_rules.terms over R [m][8] (4 letters) first, then t = t * d(s + k, k) for k = 0 ..
    ``marg``: another marginal in ``marginal``'s place (the CPU tests put deliberate mistakes there)"""
    marg = marg or marginal
    S = np.asarray(S, dtype=np.float64)
    m = S.shape[0]
    n_win = max(int(length) - m + 1, 0)
    if n_win == 0:
        return np.zeros(0), np.zeros(0, dtype=bool)
    x = profile[int(off):int(off) + int(length)]
    with np.errstate(all="ignore"):
        if R is None:
            has = np.ones(n_win, dtype=bool)
            t = marg(x[0:n_win], S[0])
            first = 1
        else:
            R = np.asarray(R, dtype=np.float64)
            c = np.asarray(codes[int(off):int(off) + int(length)]) & 7
            t = R[0][c[0:n_win]]
            for k in range(1, m):
                t = t * R[k][c[k:k + n_win]]
            has = np.ones(n_win, dtype=bool)
            for k in range(m):
                has &= c[k:k + n_win] < 4
            first = 0
        for k in range(first, m):
            t = t * marg(x[k:k + n_win], S[k])                # whole arrays: one rounded product per window and k
    return np.where(has, t, 0.0), has


def occupancy(profile, offsets, lengths, struct_tables, codes=None, seq_tables=None, marg=None):
    """-> occ float64 [n_rec][n_motifs], windows int64 [n_rec]; struct_tables [n_motifs][m][7], seq_tables [n_motifs][m][8] | None"""
    st = np.asarray(struct_tables, dtype=np.float64)
    if st.ndim == 2:
        st = st[None]
    sq = None
    if seq_tables is not None:
        sq = np.asarray(seq_tables, dtype=np.float64)
        if sq.ndim == 2:
            sq = sq[None]
    occ = np.zeros((len(offsets), st.shape[0]))
    win = np.zeros(len(offsets), dtype=np.int64)
    for r, (o, n) in enumerate(zip(offsets, lengths)):
        for q in range(st.shape[0]):
            t, has = terms(profile, o, n, st[q], codes, None if sq is None else sq[q], marg)
            occ[r, q] = tree(t)
            win[r] = int(has.sum())
    return occ, win


# ---- the bound of a term against exact arithmetic --------------------------------------------------------------------
def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): (1 + d_1) ... (1 + d_n) = 1 + theta with |theta| <= gamma_n for |d_i| <= u"""
    return n * U / (1.0 - n * U)


def term_bound(m, joint):
    """relative error of a term against the exact value of the same expression over the same (exact) inputs, for rows and
    tables that are non-negative and finite and products that stay normal.

    A marginal is a dot product of length 7 of non-negative numbers, 7 rounded products and 6 rounded additions: every
    summand passes through at most 1 + 6 = 7 roundings, so the computed d = exact d * (1 + theta_7) (no cancellation: the
    summands have one sign).  Structure only: m marginals, 7 m roundings, and m - 1 rounded products between them:
    7 m + m - 1 = 8 m - 1 factors (1 + d_i).  Joint: the letter chain multiplies m exact table cells with m - 1 roundings,
    then m more rounded products take the marginals in: (m - 1) + m + 7 m = 9 m - 1."""
    return gamma((9 if joint else 8) * m - 1)


# ---- streams and tables for the tests --------------------------------------------------------------------------------
def rows(rng, n, dtype=np.float64, zeros=0.3):
    """n profile rows: non-negative, summing to about 1, a share of the cells exactly zero"""
    x = rng.random((n, NSTRUCT))
    x[rng.random((n, NSTRUCT)) < zeros] = 0.0
    s = x.sum(axis=1, keepdims=True)
    s[s == 0] = 1.0
    return (x / s).astype(dtype)


def stream(rng, lengths, dtype=np.float64, foreign=0.0, separator=np.nan):
    """records of the given lengths, one separator row after each -> (codes uint8, profile [n_pos][7], offsets, lengths).
    The separator rows hold NaN: a kernel that read one as data would show it."""
    codes, offsets, lengths = orules.stream(rng, lengths, 4, foreign)
    profile = np.full((codes.size, NSTRUCT), separator, dtype=dtype)
    for o, n in zip(offsets, lengths):
        profile[o:o + n] = rows(rng, int(n), dtype)
    return codes, profile, offsets, lengths


def struct_table(rng, m, lo=0.2, hi=3.0):
    """a structure table [m][7] with ratios drawn log-uniformly from [lo, hi]"""
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size=(m, NSTRUCT)))


def one_hot(letter_codes, dtype=np.float64):
    """structure-letter codes (0..6, bit 3 = case ignored) -> profile rows with a single 1; a separator (7) gets a zero row"""
    c = np.asarray(letter_codes) & 7
    p = np.zeros((c.size, NSTRUCT), dtype=dtype)
    ok = c < NSTRUCT
    p[np.flatnonzero(ok), c[ok]] = 1
    return p


def base_case(seed=20, dtype=np.float32, m=12, n_motifs=3):
    """the stream and tables of the GPU tests' basic comparison (tests/test_gpu_occupancy_profile.py); the CPU tests show
    that a contracted product, float32 accumulation, a reversed column order or a shifted window give other bits on it"""
    rng = np.random.default_rng(seed)
    lengths = [m + 40, m - 1, m, 300, 77]
    codes, profile, offsets, lengths = stream(rng, lengths, dtype, foreign=0.01)
    st = np.stack([struct_table(rng, m) for _ in range(n_motifs)])
    sq = np.stack([orules.table(rng, m) for _ in range(n_motifs)])
    return codes, profile, offsets, lengths, st, sq
