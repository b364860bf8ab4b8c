"""The rule of the in-silico mutagenesis in plain numpy over the pinned oracle: `oracle.stream_seq` on the
MUTATED codes is the score of a mutated window, bit for bit; everything else here is the max over the windows that cover
a position, with the tie rule (lowest start) and the NaN rule (never chosen).  Not a test module."""
import numpy as np

EFFECTS = ("none", "gain", "loss", "kept")


def _take(best, where, v, j):
    """fold the scores v of the windows at offset j into (best, where): greater as float32, NaN never, a tie keeps what
    came first -- the callers go from the lowest start on"""
    take = ~np.isnan(v) & (np.isnan(best) | (v > best))
    best[take] = v[take]
    where[take] = j


def mutmap(oracle, codes, T):
    """best float32 [n][4], where int8 [n][4] of a whole stream: for phase f and letter a every position p = f (mod m)
    that holds a letter is set to a -- the mutated positions lie m apart, so a window holds at most one -- and the stream
    is scored once; m * 4 oracle passes in all"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    T = np.asarray(T, dtype=np.float64)
    n, m = codes.size, T.shape[0]
    best = np.full((n, 4), np.nan, dtype=np.float32)
    where = np.full((n, 4), -1, dtype=np.int8)
    if n == 0:
        return best, where
    idx = np.arange(n)
    for f in range(min(m, n)):
        P = idx[(idx % m == f) & (codes < 4)]
        if P.size == 0:
            continue
        for a in range(4):
            mut = codes.copy()
            mut[P] = a
            sc = oracle.stream_seq(mut, T)
            b = np.full(P.size, np.nan, dtype=np.float32)
            w = np.full(P.size, -1, dtype=np.int8)
            for j in range(m - 1, -1, -1):                 # the lowest start first
                s = P - j
                v = np.where(s >= 0, sc[np.maximum(s, 0)], np.float32(np.nan)).astype(np.float32)
                _take(b, w, v, j)
            best[P, a] = b
            where[P, a] = w
    return best, where


def variant_slow(oracle, codes, T, p, a):
    """(best, where) of ONE variant by the definition: one mutated stream, a Python loop over cover(p)"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    T = np.asarray(T, dtype=np.float64)
    n, m = codes.size, T.shape[0]
    if not (0 <= p < n) or codes[p] >= 4 or a > 3:
        return np.float32(np.nan), -1
    mut = codes.copy()
    mut[p] = a
    sc = oracle.stream_seq(mut, T)
    best, where = np.float32(np.nan), -1
    for s in range(max(0, p - m + 1), min(p, n - m) + 1):  # ascending start: a tie keeps the lowest
        v = sc[s]
        if not np.isnan(v) and (np.isnan(best) or v > best):
            best, where = v, p - s
    return best, where


def mutmap_slow(oracle, codes, T):
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    best = np.full((codes.size, 4), np.nan, dtype=np.float32)
    where = np.full((codes.size, 4), -1, dtype=np.int8)
    for p in range(codes.size):
        for a in range(4):
            best[p, a], where[p, a] = variant_slow(oracle, codes, T, p, a)
    return best, where


def passes(score, thr):
    """score > thr as everywhere else: strict, the float32 widened, NaN and -inf never pass"""
    with np.errstate(invalid="ignore"):
        return np.asarray(score, dtype=np.float32).astype(np.float64) > float(thr)


def effect_codes(ref, alt, thr):
    """0 none, 1 gain, 2 loss, 3 kept (index into EFFECTS)"""
    return passes(alt, thr).astype(np.int64) + 2 * passes(ref, thr).astype(np.int64)


def events(codes, best, thr):
    """(key int64 = 4 p + a sorted, ref float32, alt float32) of the gain / loss entries of a map"""
    codes = np.asarray(codes, dtype=np.uint8)
    n = codes.size
    ok = codes < 4
    ref = np.full(n, np.nan, dtype=np.float32)
    ref[ok] = best[np.flatnonzero(ok), codes[ok]]
    eff = effect_codes(ref[:, None], best, thr)
    is_event = ((eff == 1) | (eff == 2)) & ok[:, None] & (np.arange(4)[None, :] != codes[:, None])
    p, a = np.nonzero(is_event)
    return 4 * p.astype(np.int64) + a, ref[p], best[p, a]


def table(rng, m, kind="finite"):
    """a letter table double [m][8], columns 4..7 NaN"""
    T = np.full((m, 8), np.nan)
    T[:, :4] = rng.normal(0, 2, size=(m, 4))
    if kind == "neginf":
        T[:, :4][rng.random((m, 4)) < 0.15] = -np.inf
    elif kind == "bothinf":                                   # a +inf and a -inf cell in different rows: NaN sums
        T[0, 1] = np.inf
        T[m - 1, 2] = -np.inf
    elif kind == "negzero":
        T[:, :4] = np.where(rng.random((m, 4)) < 0.6, -0.0, T[:, :4])
        T[0, :4] = -0.0
    elif kind == "halves":                                    # two identical halves and few distinct values: windows tie
        h = max(m // 2, 1)
        half = rng.integers(-2, 3, size=(h, 4)).astype(np.float64)
        T[:, :4] = np.concatenate([half] * (m // h + 1))[:m]
    elif kind != "finite":
        raise ValueError(kind)
    return T


def stream(rng, lengths, foreign=0.0):
    """packed codes of records of the given lengths (one separator after each), a share of foreign letters inside"""
    parts = []
    for L in lengths:
        c = rng.integers(0, 4, size=L).astype(np.uint8)
        if foreign and L:
            c[rng.random(L) < foreign] = 7
        parts.append(c)
        parts.append(np.asarray([7], dtype=np.uint8))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
