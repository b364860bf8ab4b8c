"""TEST-ONLY: the letter-pair counts under hits (pfmscan_site_joint_*, include/pfmscan.h) restated as a plain loop over
hits and columns -- the checker of the kernel and of the command -- and the oracle-backed engine whose ``site_joint`` is
that loop, so that the CPU suite can run ``python -m rnascan_amd.sites`` on FASTA inputs.

    joint[k][j][a][b] = the number of hits of motif k whose column j counts and has (codes[x] & 7) == a and
                        (codes2[x] & 7) == b, x = hit_pos - F + j; a column counts iff x lies inside the hit's record;
                        an absent stream has index 0.
"""
import numpy as np

import background_helpers
import dotbracket_rules
import pairsum_helpers
import sites_helpers
import sites_lib_helpers
from oracle import oracle


def site_joint(codes, codes2, pos, motif, n_motifs, offsets, lengths, m, flank=0):
    """uint64 [n_motifs][W][8][8]; ``motif`` None: one motif.  ValueError for what the entry points reject."""
    W = m + 2 * flank
    offsets, lengths = [int(x) for x in offsets], [int(x) for x in lengths]
    n_pos = len(codes if codes is not None else codes2)
    J = np.zeros((n_motifs, W, 8, 8), dtype=np.uint64)
    off_arr = np.asarray(offsets, dtype=np.int64)
    for h, p in enumerate(int(x) for x in pos):
        k = 0 if motif is None else int(motif[h])
        if not 0 <= k < n_motifs:
            raise ValueError("motif index %d is no motif" % k)
        if not 0 <= p < n_pos:
            raise ValueError("hit %d lies outside the stream" % h)
        r = int(np.searchsorted(off_arr, p, side="right")) - 1       # the last record that starts at or before p
        if r < 0 or p + m > offsets[r] + lengths[r]:
            raise ValueError("the window of hit %d leaves its record" % h)
        for j in range(W):
            x = p - flank + j
            if offsets[r] <= x < offsets[r] + lengths[r]:
                a = int(codes[x]) & 7 if codes is not None else 0
                b = int(codes2[x]) & 7 if codes2 is not None else 0
                J[k, j, a, b] += np.uint64(1)
    return J


def struct_consensus():
    """the most likely letter of every row of the shipped SLBP structure PFM"""
    from rnascan_amd import pssm
    pfm = pssm.read_pfm(sites_lib_helpers.STRUCT_PFM)
    letters = list(pfm)
    rows = np.stack([np.asarray(pfm[c], dtype=np.float64) for c in letters], axis=1)
    return "".join(letters[int(k)] for k in rows.argmax(axis=1))


def write_letter_inputs(tmp_path, n=31, seed=5, reverse=False):
    """the inputs of sites_helpers.write_inputs (records of 20-260 letters with the SLBP site planted) + a structure FASTA
    of the same records: the structure PFM's consensus under every planted site, random letters elsewhere, a third of
    them in lower case, a foreign character at some record ends (flanks reach it, no hit window holds it)
    -> (seqs.fa, structs.fa, profile directory)"""
    from rnascan_amd import fasta
    fa, d, _ = sites_helpers.write_inputs(tmp_path, n=n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    cons = struct_consensus()
    site = sites_helpers.SITE.replace("T", "U")
    recs, out = [(r.id, r.seq) for r in fasta.open_lazy(fa)], []
    for i, (rid, seq) in enumerate(recs):
        st = list("".join(rng.choice(list("EHTBLRM"), size=len(seq))))
        body = seq.upper().replace("T", "U")
        at = body.find(site)
        while at >= 0:
            st[at:at + len(site)] = cons
            at = body.find(site, at + 1)
        for x in np.flatnonzero(rng.random(len(st)) < 0.3):
            st[x] = st[x].lower()
        if i % 8 == 0:
            st[-1] = "N"
        if i % 8 == 4:
            st[0] = "N"
        out.append((rid, "".join(st)))
    if reverse:
        recs, out = recs[::-1], out[::-1]
        fa = str(tmp_path / "seqs_reversed.fa")
        background_helpers.write_fasta(fa, recs)
    sfa = str(tmp_path / ("structs_reversed.fa" if reverse else "structs.fa"))
    background_helpers.write_fasta(sfa, out)
    return fa, sfa, d


def count_table(hits, seqs, structs, names, m, flank):
    """{name: int64 [W][8][8]} from rnascan's own hit table -- ``hits``: (record id, 0-based start, name) -- counted with
    the plain loop over the records' strings; ``seqs`` / ``structs``: {id: string} or None"""
    from rnascan_amd import fasta, pack
    W = m + 2 * flank
    J = dict((name, np.zeros((W, 8, 8), dtype=np.int64)) for name in names)
    code_a = dict((rid, pack.encode_rna(fasta.preprocess_seq(s, True))) for rid, s in seqs.items()) if seqs else None
    code_b = dict((rid, pack.encode_letters(s, fasta.STRUCT, keep_case=True) & 7) for rid, s in structs.items()) if structs else None
    for rid, start, name in hits:
        L = len((seqs or structs)[rid])
        for j in range(W):
            x = start - flank + j
            if 0 <= x < L:
                J[name][j, int(code_a[rid][x]) if code_a else 0, int(code_b[rid][x]) if code_b else 0] += 1
    return J


class _RulesCtx(object):
    """what cli.struct_input asks of an engine's context: the dot-bracket annotation, from tests/dotbracket_rules.py"""

    def dotbracket_annotate_host(self, codes):
        from rnascan_amd import dotbracket, pack
        codes = np.asarray(codes, dtype=np.uint8)
        out = np.full(codes.size, pack.SEP, dtype=np.uint8)
        counts = np.zeros(7, dtype=np.int64)
        start = 0
        for end in np.flatnonzero(codes == pack.SEP):
            body = codes[start:end]
            if np.any(body > dotbracket.CLOSE):
                err = ValueError("character outside '().'")
                err.position = start + int(np.flatnonzero(body > dotbracket.CLOSE)[0])
                raise err
            s = "".join(".()"[c] for c in body)
            try:
                letters = dotbracket_rules.annotate(s)
            except ValueError:
                err = ValueError("unbalanced brackets")
                err.position = start
                raise err
            out[start:end] = [pack.STRUCT_LETTERS.index(ch) for ch in letters]
            counts += dotbracket_rules.count_letters(letters)
            start = int(end) + 1
        return out, counts


class RulesEngine(sites_lib_helpers.RulesEngine, pairsum_helpers.PairSumLibraryOracleEngine):
    """the oracle-backed engine of the site-profile tests + ``site_joint`` from the plain loop (same contract as
    HipEngine.site_joint) + the two-FASTA methods HipEngine has (hits_pair_sum, the letter libraries), so that
    sites.select_letters and scanner.scan_pair / scan_records take the branches they take on the GPU"""

    def __init__(self):
        self.ctx = _RulesCtx()

    def site_joint(self, stream, pos, motif, n_motifs, m, flank=0, first=True, second=True):
        first = bool(first) and stream.codes is not None
        second = bool(second) and getattr(stream, "codes2", None) is not None
        if not first and not second:
            raise ValueError("the stream has neither of the code streams asked for")
        if m + 2 * flank > 4096:
            raise ValueError("width + 2 x flank exceeds PFMSCAN_MAX_WIDTH")
        return site_joint(stream.codes if first else None, stream.codes2 if second else None, pos, motif, n_motifs,
                          stream.offsets, stream.lengths, m, flank)

    def library_hits_letters(self, stream, seq_tables, struct_tables, thr_seq, thr_struct):
        parts = []
        for k in range(len(struct_tables)):
            if seq_tables is None:
                sq, st = None, oracle.stream_letters_f64(stream.codes, struct_tables[k])
                pos = oracle.stream_hits(None, st, -np.inf, thr_struct)
            else:
                sq = oracle.stream_seq(stream.codes, seq_tables[k])
                st = oracle.stream_letters_f64(stream.codes2, struct_tables[k])
                pos = oracle.stream_hits(sq, st, thr_seq, thr_struct)
            parts.append((pos, np.full(pos.size, k, dtype=np.int32), None if sq is None else sq[pos], st[pos]))
        pos, mo = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        order = np.lexsort((mo, pos))
        sq = None if seq_tables is None else np.concatenate([p[2] for p in parts])[order]
        return pos[order], mo[order], sq, np.concatenate([p[3] for p in parts])[order]


class PlainEngine(sites_lib_helpers.RulesEngine):
    """the same without hits_pair_sum and the letter libraries: the host-side branches of scan_pair / select_letters"""

    def __init__(self):
        self.ctx = _RulesCtx()

    site_joint = RulesEngine.site_joint
