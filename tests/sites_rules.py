"""A numpy restatement of the site profiles (include/pfmscan.h, rnascan_amd/csrc/pfmscan_sites.hip): the groups of a sorted
hit list and the ORDER OF ADDITIONS inside a group, which the kernels equal bit for bit.

    column j of hit h     stream row x = pos[h] - F + j, j in [0, W), W = m + 2 F; it counts iff x lies inside the hit's record
    group                 at most GROUP consecutive hits of one record, counted from that record's first hit
    wave v of a group     acc = 0.0 per cell; hits v, v + 4, v + 8, ... of the group in ascending order: acc += (double) cell
                          where the column counts (float32 rows widened to fp64 first)
    group                 ((wave 0 + wave 1) + wave 2) + wave 3
    counts[j][k]          the number of the group's hits whose column j counts and min(code, 7) == k
"""
import math

import numpy as np

GROUP = 4096
WAVES = 4


def groups(pos, offsets, lengths, m):
    """sorted hit list -> (grp_first int64 [n_grp + 1], grp_rec int64 [n_grp]); ValueError for what pfmscan_site_groups rejects"""
    pos = np.asarray(pos, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    if m < 1:
        raise ValueError("width")
    if np.any(offsets < 0) or np.any(lengths < 0) or np.any(offsets[1:] <= offsets[:-1] + lengths[:-1]):
        raise ValueError("record table")
    if np.any(pos[1:] <= pos[:-1]):
        raise ValueError("hits do not ascend")
    first, rec = [], []
    if pos.size:
        if offsets.size == 0:
            raise ValueError("hit outside every record")
        r = np.searchsorted(offsets, pos, side="right") - 1
        if np.any(r < 0) or np.any(pos + m > offsets[r] + lengths[r]):
            raise ValueError("window outside its record")
        h = 0
        while h < pos.size:
            e = int(np.searchsorted(r, r[h], side="right"))
            for a in range(h, e, GROUP):
                first.append(a)
                rec.append(int(r[h]))
            h = e
    first.append(pos.size)
    return np.asarray(first, dtype=np.int64), np.asarray(rec, dtype=np.int64)


def _rows(pos, grp_first, grp_rec, offsets, lengths, m, flank):
    """per group and slot: (stream row [n_grp][S][WAVES][W], counted mask of the same shape); slot s of wave v is hit 4 s + v"""
    n_grp = grp_rec.size
    W = m + 2 * flank
    size = np.diff(grp_first)
    S = int((size.max() + WAVES - 1) // WAVES) if n_grp else 0
    h = np.arange(S * WAVES, dtype=np.int64).reshape(S, WAVES)[None] + np.zeros((n_grp, 1, 1), dtype=np.int64)
    live = h < size[:, None, None]
    idx = np.where(live, grp_first[:-1, None, None] + h, 0)
    p = pos[idx] if pos.size else np.zeros_like(idx)
    x = p[..., None] - flank + np.arange(W, dtype=np.int64)
    lo = offsets[grp_rec][:, None, None, None]
    hi = lo + lengths[grp_rec][:, None, None, None]
    counted = live[..., None] & (x >= lo) & (x < hi)
    return np.where(counted, x, 0), counted


def site_sums(profile, codes, pos, offsets, lengths, m, flank=0):
    """-> (grp_rec, sums float64 [n_grp][W][7] | None, counts uint32 [n_grp][W][8] | None) as the device produces them"""
    pos = np.asarray(pos, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    grp_first, grp_rec = groups(pos, offsets, lengths, m)
    n_grp, W = grp_rec.size, m + 2 * flank
    sums = counts = None
    size = np.diff(grp_first)
    a = b = 0
    while b < n_grp:                                     # a few groups at a time: the gathered rows stay small
        a, b = b, b + 1
        while b < n_grp and (b + 1 - a) * max(int(size[a:b + 1].max()), 1) * W <= (1 << 20):
            b += 1
        x, counted = _rows(pos, grp_first[a:b + 1], grp_rec[a:b], offsets, lengths, m, flank)
        if profile is not None:
            if sums is None:
                sums = np.zeros((n_grp, W, 7), dtype=np.float64)
            acc = np.zeros((b - a, WAVES, W, 7), dtype=np.float64)
            for s in range(x.shape[1]):
                rows = np.asarray(profile[x[:, s]], dtype=np.float64)
                acc = np.where(counted[:, s][..., None], acc + rows, acc)
            sums[a:b] = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
        if codes is not None:
            if counts is None:
                counts = np.zeros((n_grp, W, 8), dtype=np.uint32)
            k = np.minimum(np.asarray(codes)[x], 7)
            hot = (k[..., None] == np.arange(8)) & counted[..., None]
            counts[a:b] = hot.sum(axis=(1, 2)).astype(np.uint32)
    if profile is not None and sums is None:
        sums = np.zeros((0, W, 7), dtype=np.float64)
    if codes is not None and counts is None:
        counts = np.zeros((0, W, 8), dtype=np.uint32)
    return grp_rec, sums, counts


def first_bad(profile, pos, offsets, lengths, m, flank=0):
    """flat element index row * 7 + column of the earliest NaN / infinite / negative cell under a counted column of a hit, or -1"""
    pos = np.asarray(pos, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    touched = np.zeros(len(profile), dtype=bool)
    r = np.searchsorted(offsets, pos, side="right") - 1
    for p, rr in zip(pos.tolist(), r.tolist()):
        lo = max(p - flank, int(offsets[rr]))
        hi = min(p + m + flank, int(offsets[rr] + lengths[rr]))
        touched[lo:hi] = True
    rows = np.asarray(profile, dtype=np.float64)
    bad = ~((rows >= 0) & (rows < np.inf)) & touched[:, None]
    at = np.flatnonzero(bad.ravel())
    return int(at[0]) if at.size else -1


def coverage(pos, offsets, lengths, m, flank=0):
    """n[j], int64 [W]: the number of hits whose column j counts, from positions and record bounds alone"""
    pos = np.asarray(pos, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    W = m + 2 * flank
    if pos.size == 0:
        return np.zeros(W, dtype=np.int64)
    r = np.searchsorted(offsets, pos, side="right") - 1
    x = pos[:, None] - flank + np.arange(W, dtype=np.int64)
    return ((x >= offsets[r][:, None]) & (x < (offsets[r] + lengths[r])[:, None])).sum(axis=0).astype(np.int64)


def total(sums):
    """group rows [n][W][7] -> float64 [W][7], math.fsum per cell"""
    sums = np.asarray(sums, dtype=np.float64)
    out = np.zeros(sums.shape[1:], dtype=np.float64)
    for j in range(out.shape[0]):
        for c in range(out.shape[1]):
            out[j, c] = math.fsum(sums[:, j, c].tolist())
    return out
