"""A restatement, in Python ints, of the device-side merge of the expected counts (include/pfmscan.h, "expected counts: the
records added up on the device"; rnascan_amd/csrc/pfmscan_expect_merge.hip).  The long accumulator is the library site
profiles' (tests/sites_lib_rules.py), with m * 8 cells per motif.

    cell                a finite double > 0 is the integer v / 2^-1074; +0.0 and -0.0 are 0 and add nothing
    rejected            a NaN, +-inf or negative cell is never decomposed: it adds nothing and names its record in bad
    A[k][e]             the exact integer sum over the records of cell e = 8 row + column of motif k
    limbs               A cut into 66 limbs of weight 2^(32 i), every limb but the top one below 2^32 (normalised)
    rounding            A / 2^1074, int true division: to nearest, ties to even; +inf beyond DBL_MAX -- math.fsum of the cells
                        wherever that does not overflow
    bad[k]              [smallest record with a NaN or +-inf cell of motif k, smallest record with a cell < 0 (-inf is both)];
                        -1: none.  Added to an earlier verdict, the smaller index >= 0 stays.
"""
import math

import numpy as np

import sites_lib_rules as lrules

LIMBS = lrules.LIMBS


def accepted(v):
    """is the cell decomposed (or a zero)?"""
    return math.isfinite(v) and not v < 0


def merge_ints(exp):
    """exp float64 [n_rec][n_motifs][m][8] -> A object [n_motifs][m * 8]: the exact sums of the accepted cells, in units of 2^-1074"""
    exp = np.asarray(exp, dtype=np.float64)
    n_rec, n_motifs = exp.shape[:2]
    flat = exp.reshape(n_rec, n_motifs, -1)
    A = np.zeros((n_motifs, flat.shape[2]), dtype=object)
    for k in range(n_motifs):
        for e in range(flat.shape[2]):
            A[k, e] = sum(lrules.as_int(v) for v in flat[:, k, e].tolist() if accepted(v))
    return A


def limbs_of(A):
    """A object [n_motifs][n] -> NORMALISED uint64 [n_motifs][LIMBS][n]"""
    A = np.asarray(A, dtype=object)
    out = np.zeros((A.shape[0], LIMBS, A.shape[1]), dtype=np.uint64)
    for k in range(A.shape[0]):
        for e in range(A.shape[1]):
            x = int(A[k, e])
            for i in range(LIMBS - 1):
                out[k, i, e] = x & 0xffffffff
                x >>= 32
            assert x < 1 << 64
            out[k, LIMBS - 1, e] = x
    return out


def normalise(acc):
    """uint64 [..][LIMBS][n] raw or normalised -> normalised (through the integers)"""
    acc = np.asarray(acc)
    A = lrules.acc_int(acc)
    return limbs_of(A.reshape(-1, A.shape[-1])).reshape(acc.shape)


def rounded(A):
    """A object [..] -> float64 [..]: what pfmscan_site_acc_round gives"""
    A = np.asarray(A, dtype=object)
    out = np.zeros(A.shape, dtype=np.float64)
    for idx in np.ndindex(*A.shape):
        out[idx] = lrules.round_int(int(A[idx]))
    return out


def bad(exp, before=None):
    """exp float64 [n_rec][n_motifs][m][8] -> int64 [n_motifs][2]; ``before``: the verdicts the call adds to"""
    exp = np.asarray(exp, dtype=np.float64)
    n_rec, n_motifs = exp.shape[:2]
    flat = exp.reshape(n_rec, n_motifs, -1)
    out = np.full((n_motifs, 2), -1, dtype=np.int64) if before is None else np.array(before, dtype=np.int64)
    for k in range(n_motifs):
        for col, hit in enumerate((~np.isfinite(flat[:, k]), flat[:, k] < 0)):
            rows = np.flatnonzero(hit.any(axis=1))
            if rows.size and (out[k, col] < 0 or rows[0] < out[k, col]):
                out[k, col] = rows[0]
    return out


def fsum_cells(exp):
    """math.fsum over the records, cell by cell -> float64 [n_motifs][m * 8] (every cell accepted, no overflow)"""
    exp = np.asarray(exp, dtype=np.float64)
    flat = exp.reshape(exp.shape[0], exp.shape[1], -1)
    out = np.zeros(flat.shape[1:], dtype=np.float64)
    for k in range(flat.shape[1]):
        for e in range(flat.shape[2]):
            out[k, e] = math.fsum(flat[:, k, e].tolist())
    return out
