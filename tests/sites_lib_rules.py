"""A restatement, in Python ints and numpy, of the site profiles of a motif LIBRARY (include/pfmscan.h, "site profiles of a
library"; rnascan_amd/csrc/pfmscan_sites_lib.hip, pfmscan_sites_lib_host.hip, pfmscan_superacc.hpp).

    hit list            (pos, motif), MOTIF-MAJOR: motif does not descend, positions ascend strictly inside one motif
    groups of motif k   sites_rules.groups of motif k's hit list alone
    group cell          sites_rules.site_sums (the order of additions inside a group)
    A[k][e]             the exact integer sum over motif k's groups of (group cell / 2^-1074)
    limbs               A = sum of limb[i] * 2^(32 i), 66 limbs; a double v > 0 with exponent field E and fraction f:
                        M = f, b = 0 (E == 0) else M = f | 2^52, b = E - 1; x = M << (b mod 32); its three 32-bit pieces
                        go to limbs b // 32, b // 32 + 1, b // 32 + 2
    rounding            A / 2^1074, int true division: correctly rounded, ties to even; +inf beyond DBL_MAX
"""
import struct

import numpy as np

import sites_rules as rules

LIMBS = 66


def as_int(v):
    """finite double v >= 0 -> the integer v / 2^-1074"""
    if v == 0:
        return 0
    bits = struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    assert bits >> 63 == 0 and (bits >> 52) != 0x7ff, v
    E, f = bits >> 52, bits & ((1 << 52) - 1)
    return f if E == 0 else (f | (1 << 52)) << (E - 1)


def pieces(v):
    """v > 0 -> (first limb, [three pieces below 2^32])"""
    bits = struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    E, f = bits >> 52, bits & ((1 << 52) - 1)
    M, b = (f, 0) if E == 0 else (f | (1 << 52), E - 1)
    x = M << (b % 32)
    assert x < 1 << 85
    return b // 32, [x & 0xffffffff, (x >> 32) & 0xffffffff, x >> 64]


def raw_limbs(values):
    """the RAW accumulator of one cell, a list of LIMBS ints: what adding every value's pieces leaves"""
    acc = [0] * LIMBS
    for v in values:
        if v == 0:
            continue
        first, p = pieces(v)
        for i in range(3):
            acc[first + i] += p[i]
    return acc


def limbs_int(acc):
    """limbs [LIMBS] (raw or normalised; ints or uint64) -> A"""
    return sum(int(x) << (32 * i) for i, x in enumerate(acc))


def acc_int(acc):
    """uint64 [..][LIMBS][n] -> object array [..][n] of the integers A"""
    acc = np.asarray(acc)
    out = np.zeros(acc.shape[:-2] + acc.shape[-1:], dtype=object)
    for i in range(LIMBS):
        out = out + (acc[..., i, :].astype(object) << (32 * i))
    return out


def round_int(A):
    """A * 2^-1074 to the nearest double, ties to even, +inf beyond DBL_MAX"""
    try:
        return A / (1 << 1074)
    except OverflowError:
        return float("inf")


def motif_major(pos, motif):
    """hits in any order -> the stable permutation that sorts them by motif"""
    return np.argsort(np.asarray(motif), kind="stable")


def groups(pos, motif, n_motifs, offsets, lengths, m):
    """motif-major list -> (grp_first [n_grp + 1], grp_rec, grp_motif); ValueError for what pfmscan_site_groups_lib rejects"""
    pos, motif = np.asarray(pos, dtype=np.int64), np.asarray(motif, dtype=np.int64)
    if np.any(motif < 0) or np.any(motif >= n_motifs) or np.any(motif[1:] < motif[:-1]):
        raise ValueError("motif indices")
    rules.groups(pos[:0], offsets, lengths, m)                # the record table and the width, also without hits
    first, rec, mot = [], [], []
    for k in range(n_motifs):
        a, b = np.searchsorted(motif, [k, k + 1])
        gf, gr = rules.groups(pos[a:b], offsets, lengths, m)
        first += (gf[:-1] + a).tolist()
        rec += gr.tolist()
        mot += [k] * gr.size
    first.append(pos.size)
    return np.asarray(first, dtype=np.int64), np.asarray(rec, dtype=np.int64), np.asarray(mot, dtype=np.int64)


def site_sums_library(profile, codes, pos, motif, n_motifs, offsets, lengths, m, flank=0):
    """hits in any order that ascends inside a motif -> (A object [n_motifs][W * 7] | None, counts int64 [n_motifs][W][8] |
    None, group rows per motif: list of float64 [n_grp_k][W][7] | None)"""
    pos, motif = np.asarray(pos, dtype=np.int64), np.asarray(motif, dtype=np.int64)
    W = m + 2 * flank
    A = np.zeros((n_motifs, W * 7), dtype=object) if profile is not None else None
    counts = np.zeros((n_motifs, W, 8), dtype=np.int64) if codes is not None else None
    rows = [] if profile is not None else None
    for k in range(n_motifs):
        _, sums, cnt = rules.site_sums(profile, codes, pos[motif == k], offsets, lengths, m, flank)
        if sums is not None:
            rows.append(sums)
            flat = sums.reshape(sums.shape[0], W * 7)
            for e in range(W * 7):
                A[k, e] = sum(as_int(v) for v in flat[:, e].tolist())
        if cnt is not None:
            counts[k] = cnt.astype(np.int64).sum(axis=0)
    return A, counts, rows


def normalised(acc):
    acc = np.asarray(acc)
    return bool(np.all(acc[..., :-1, :] < (1 << 32)))
