"""TEST-ONLY helpers for the joint threshold of the two-FASTA mode (pfmscan_hits_pair_sum_*, ``--min-seqstruct`` on
``seqs.fa structs.fa``): the predicate restated on the oracle's all-scores arrays with numpy / Python rounding, an
oracle-backed engine that HAS ``hits_pair_sum``, and the generators the CPU and GPU tests share."""
import numpy as np

from engines import OracleEngine
from oracle import oracle


def printed_sum(sq, st):
    """LogOdds.SeqStruct as scan_pair.rows prints it: np.round on the float32 column, round() on Python floats
    (rnascan.py:273), one fp64 addition (rnascan.py:416-434)"""
    lo_seq = np.round(np.asarray(sq, dtype=np.float32), 3).astype(np.float64)
    lo_st = np.array([round(float(x), 3) for x in np.asarray(st, dtype=np.float64)], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return lo_seq + lo_st


def pair_sum_hits(sq, st, thr_seq, thr_struct, thr_sum):
    """positions that pass both single thresholds (strict; NaN / -inf never pass) AND whose printed sum exceeds thr_sum"""
    pos = oracle.stream_hits(sq, st, thr_seq, thr_struct)
    return pos[printed_sum(sq[pos], st[pos]) > thr_sum]


class PairSumOracleEngine(OracleEngine):
    """OracleEngine + ``hits_pair_sum`` as HipEngine has it: scan_pair then takes its decided-by-the-engine branch"""

    calls = 0

    def hits_pair_sum(self, stream, seq_table, struct_table, thr_seq, thr_struct, thr_sum):
        PairSumOracleEngine.calls += 1
        sq = oracle.stream_seq(stream.codes, seq_table)
        st = oracle.stream_letters_f64(stream.codes2, struct_table)
        pos = pair_sum_hits(sq, st, thr_seq, thr_struct, thr_sum)
        return pos, sq[pos], st[pos]


class PairSumLibraryOracleEngine(PairSumOracleEngine):
    """... + the two-FASTA library methods as HipEngine has them (thr_eff restated: finite unless the structure table holds a
    +inf cell / the letter columns a +inf or NaN cell beside thr_seq = -inf)"""

    lib_calls = 0

    def library_letters_sum_thresholds(self, seq_tables, struct_tables, thr_seq, thr_sum):
        from rnascan_amd import _lib
        return _lib.library_letters_sum_thresholds(seq_tables, struct_tables, thr_seq, thr_sum)

    def library_hits_letters_sum(self, stream, seq_tables, struct_tables, thr_seq, thr_struct, thr_sum):
        PairSumLibraryOracleEngine.lib_calls += 1
        parts = []
        for k in range(len(seq_tables)):
            sq = oracle.stream_seq(stream.codes, seq_tables[k])
            st = oracle.stream_letters_f64(stream.codes2, struct_tables[k])
            pos = pair_sum_hits(sq, st, thr_seq, thr_struct, thr_sum)
            parts.append((pos, np.full(pos.size, k, dtype=np.int32), sq[pos], st[pos]))
        pos, mo = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        order = np.lexsort((mo, pos))
        return pos[order], mo[order], np.concatenate([p[2] for p in parts])[order], np.concatenate([p[3] for p in parts])[order]


def table(rng, m, n_letters, neg_inf=0.0, nan=0.0, pos_inf=0.0, scale=1.5, dyadic=False):
    """letter table [m][8]: columns n_letters.. NaN; optionally -inf / NaN / +inf cells; dyadic: multiples of 1/16"""
    T = np.full((m, 8), np.nan)
    v = rng.normal(-0.3, scale, size=(m, n_letters))
    if dyadic:
        v = np.round(v * 16.0) / 16.0
    T[:, :n_letters] = v
    r = rng.random((m, n_letters))
    T[:, :n_letters][r < neg_inf] = -np.inf
    T[:, :n_letters][(r >= neg_inf) & (r < neg_inf + nan)] = np.nan
    T[:, :n_letters][(r >= neg_inf + nan) & (r < neg_inf + nan + pos_inf)] = np.inf
    return T


def streams(rng, lengths, foreign=0.002):
    """(sequence stream, structure stream) of the same records: foreign letters on either side, lower-case structure
    letters (bit 3 of the code)"""
    from rnascan_amd import pack
    c1, c2 = [], []
    for L in lengths:
        a = rng.integers(0, 4, size=L).astype(np.uint8)
        a[rng.random(L) < foreign] = pack.SEP
        b = rng.integers(0, 7, size=L).astype(np.uint8)
        b[rng.random(L) < foreign] = pack.SEP
        low = (rng.random(L) < 0.3) & (b != pack.SEP)
        b[low] |= pack.CASE_BIT
        c1.append(a)
        c2.append(b)
    s1, s2 = pack.pack(c1), pack.pack(c2)
    assert np.array_equal(s1.offsets, s2.offsets) and s1.n_pos == s2.n_pos
    return s1, s2


def lengths_for(rng, n_pos, n_records, m):
    """n_records record lengths (some shorter than m, one empty) whose packed stream has exactly n_pos positions"""
    small = [0, max(m - 1, 0), m][: max(0, min(3, n_records - 1))]       # a record takes its letters + one separator
    rest = n_records - len(small)
    total = n_pos - n_records - sum(small)
    assert total >= rest
    cut = np.sort(rng.choice(np.arange(1, total), size=rest - 1, replace=False)) if rest > 1 else np.zeros(0, dtype=np.int64)
    ls = [int(x) for x in np.diff(np.concatenate([[0], cut, [total]]))]
    ls = ls[:1] + small + ls[1:]
    assert sum(L + 1 for L in ls) == n_pos
    return ls
