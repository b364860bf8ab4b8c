"""A numpy restatement of the ORDER OF ADDITIONS of the per-record column sums (rnascan_amd/csrc/pfmscan_background.hip,
include/pfmscan.h), which the kernels equal bit for bit, the depth of that order (for the error bound against math.fsum),
and the background that follows from the sums (the arithmetic of compute_background, rnascan.py:440-465).

    piece p of a record   rows [p * PIECE, min((p + 1) * PIECE, L)), counted from the record's first row
    lane t of a piece     acc = 0.0; acc += row[t]; acc += row[t + LANES]; ...           (float32 rows widened to fp64 first)
    wave w of a piece     its 64 lanes folded as a[i] += a[i + s] for s = 32, 16, 8, 4, 2, 1
    piece                 ((wave 0 + wave 1) + wave 2) + wave 3
    record                piece 0, += piece 1, += piece 2, ...                              (0.0 for an empty record)
"""
import math

import numpy as np

PIECE = 2048
LANES = 256
WAVE = 64
STRUCT = "EHTBLRM"


def _fold(acc):
    """lane accumulators [..., LANES, 7] -> piece sums [..., 7]"""
    w = acc.reshape(acc.shape[:-2] + (LANES // WAVE, WAVE, 7))
    s = WAVE // 2
    while s:
        w = w[..., :s, :] + w[..., s:2 * s, :]
        s //= 2
    w = w[..., 0, :]
    return ((w[..., 0, :] + w[..., 1, :]) + w[..., 2, :]) + w[..., 3, :]


def record_sums(rows):
    """[L][7] float32 / float64 rows of ONE record -> float64 [7]"""
    rows = np.asarray(rows).astype(np.float64).reshape(-1, 7)
    total = np.zeros(7, dtype=np.float64)
    for p, a in enumerate(range(0, rows.shape[0], PIECE)):
        piece = rows[a:a + PIECE]
        acc = np.zeros((LANES, 7), dtype=np.float64)
        for k in range(0, piece.shape[0], LANES):
            tile = piece[k:k + LANES]
            acc[:tile.shape[0]] += tile
        s = _fold(acc)
        total = s if p == 0 else total + s
    return total


def colsums(profile, offsets, lengths):
    """packed profile [n_pos][7] + record table -> float64 [n_rec][7].  Records of at most LANES rows (one tile: a lane
    holds 0.0 + its row) are folded many at a time."""
    offsets = np.asarray(offsets, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    out = np.zeros((len(offsets), 7), dtype=np.float64)
    short = np.flatnonzero(lengths <= LANES)
    for lo in range(0, short.size, 4096):
        grp = short[lo:lo + 4096]
        acc = np.zeros((grp.size, LANES, 7), dtype=np.float64)
        for i, r in enumerate(grp):
            acc[i, :lengths[r]] += profile[offsets[r]:offsets[r] + lengths[r]]
        out[grp] = _fold(acc)
    for r in np.flatnonzero(lengths > LANES):
        out[r] = record_sums(profile[offsets[r]:offsets[r] + lengths[r]])
    return out


def depth(lengths):
    """the longest chain of additions one element passes through, over records of these lengths: the tile adds of its
    lane (the first one, onto 0.0, included), 6 for the lanes of a wave, 3 for the waves, one per further piece; and the
    same for the columns of all records together, had they been added in that order"""
    d = 0
    for L in set(int(x) for x in np.asarray(lengths).ravel()):
        if L <= 0:
            continue
        pieces = (L + PIECE - 1) // PIECE
        tiles = (min(L, PIECE) + LANES - 1) // LANES
        d = max(d, tiles + 6 + 3 + pieces - 1)
    return d


def content(sums, letters):
    """per-record sums [n][7] in column order ``letters`` -> {letter: probability} in EHTBLRM order"""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 7)
    letters = list(letters)
    count = [math.fsum(sums[:, letters.index(c)].tolist()) for c in STRUCT]
    total = math.fsum([7.0] + count)
    return {c: (count[k] + 1) / total for k, c in enumerate(STRUCT)}


def first_bad(profile, offsets, lengths):
    """flat element index row * 7 + column of the earliest NaN / infinite / negative cell inside a record, or -1"""
    best = -1
    for off, L in zip(offsets, lengths):
        rows = np.asarray(profile[off:off + L], dtype=np.float64)
        bad = np.flatnonzero(~((rows >= 0) & (rows < np.inf)).ravel())
        if bad.size:
            at = int(off) * 7 + int(bad[0])
            best = at if best < 0 else min(best, at)
    return best
