"""TEST-ONLY helpers of the library site-profile tests (CPU and GPU): the oracle-backed engine whose ``site_sums_library``
is the Python-int restatement (tests/sites_lib_rules.py), a small multi-PFM library made from the shipped SLBP PFMs, and
the files ``--all-motifs`` must write, assembled from one run of the single-motif command per pair."""
import io
import os

import numpy as np

import sites_helpers
import sites_lib_rules as lrules
import sites_rules as rules
from conftest import DATA_DIR
from rnascan_amd import pssm, sites

SEQ_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")
STRUCT_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt")


def int_limbs(A):
    """A -> normalised uint64 [LIMBS]"""
    out = [(A >> (32 * i)) & 0xffffffff for i in range(lrules.LIMBS - 1)] + [A >> (32 * (lrules.LIMBS - 1))]
    return np.asarray(out, dtype=np.uint64)


class RulesEngine(sites_helpers.RulesEngine):
    """... + site_sums_library from the restated rules (same contract as HipEngine.site_sums_library)"""

    def site_sums_library(self, stream, pos, motif, n_motifs, m, flank=0, letters=True, profile=True):
        letters = bool(letters) and stream.codes is not None
        profile = bool(profile) and stream.profile is not None
        if not letters and not profile:
            raise ValueError("the stream has neither the codes nor the profile asked for")
        pos, motif = np.asarray(pos, dtype=np.int64), np.asarray(motif, dtype=np.int64)
        if profile:                                  # a bad cell under a hit of ANY motif
            bad = rules.first_bad(stream.profile, np.unique(pos), stream.offsets, stream.lengths, m, flank)
            if bad >= 0:
                err = ValueError("bad cell")
                err.element = bad
                raise err
        A, counts, _ = lrules.site_sums_library(stream.profile if profile else None, stream.codes if letters else None, pos, motif,
                                                n_motifs, stream.offsets, stream.lengths, m, flank)
        acc = None
        if A is not None:
            acc = np.zeros((n_motifs, lrules.LIMBS, A.shape[1]), dtype=np.uint64)
            for k in range(n_motifs):
                for e in range(A.shape[1]):
                    acc[k, :, e] = int_limbs(A[k, e])
        return acc, (None if counts is None else counts.astype(np.uint64))


def _write_multi(path, blocks, letters):
    with open(path, "w") as out:
        for name, rows in blocks:
            out.write("#%s\n#PO\t%s\n" % (name, "\t".join(letters)))
            for i, row in enumerate(rows):
                out.write("%d\t%s\n" % (i, "\t".join(repr(float(x)) for x in row)))
            out.write("\n")


def _write_single(path, rows, letters):
    with open(path, "w") as out:
        out.write("PO\t%s\n" % "\t".join(letters))
        for i, row in enumerate(rows):
            out.write("%d\t%s\n" % (i, "\t".join(repr(float(x)) for x in row)))


def write_library(tmp_path, extra=()):
    """multi-PFM libraries of four pairs of two widths (18 and 12) from the shipped SLBP PFMs: the PFMs themselves, a copy
    with its rows rolled by one, the first 12 rows and the last 12; every motif also as a single-PFM file.
    ``extra``: (id, sequence rows, structure rows) appended.  -> (seq library, struct library, [(id, seq file, struct file)])"""
    seq, st = pssm.read_pfm(SEQ_PFM), pssm.read_pfm(STRUCT_PFM)
    sl, tl = list(seq), list(st)
    S, T = np.stack(list(seq.values()), axis=1), np.stack(list(st.values()), axis=1)
    motifs = [("SLBP", S, T), ("head", S[:12], T[:12]), ("rolled", np.roll(S, 1, axis=0), np.roll(T, 1, axis=0)), ("tail", S[6:], T[6:])]
    motifs += list(extra)
    lib_seq, lib_struct = str(tmp_path / "lib_seq.txt"), str(tmp_path / "lib_struct.txt")
    _write_multi(lib_seq, [(n, a) for n, a, _ in motifs], sl)
    _write_multi(lib_struct, [(n, b) for n, _, b in motifs], tl)
    pairs = []
    for n, a, b in sorted(motifs, key=lambda x: x[0]):          # pair order: sorted by id
        fs, ft = str(tmp_path / ("one_%s_seq.txt" % n)), str(tmp_path / ("one_%s_struct.txt" % n))
        _write_single(fs, a, sl)
        _write_single(ft, b, tl)
        pairs.append((n, fs, ft))
    return lib_seq, lib_struct, pairs


def write_library_inputs(tmp_path, n=31, seed=5):
    fa, avg, _ = sites_helpers.write_inputs(tmp_path, n=n, seed=seed)
    lib_seq, lib_struct, pairs = write_library(tmp_path)
    return fa, avg, lib_seq, lib_struct, pairs


def assemble_single_runs(tmp_path, pairs, tail, engine, use_seq=True, use_struct=True, flank=0):
    """one run of the single-motif command per pair -> {".struct.txt": bytes, ".seq.txt": bytes, ".counts.txt": bytes} as
    --all-motifs must write them; a pair whose run writes nothing (no site) is left out of the PFM files and has a
    zero block in the counts"""
    out = {".struct.txt": b"", ".seq.txt": b"", ".counts.txt": b""}
    for name, fs, ft in pairs:
        prefix = str(tmp_path / ("single_" + name))
        argv = (["-p", fs] if use_seq else []) + (["-q", ft] if use_struct else []) + ["-o", prefix] + list(tail)
        rc = sites.main(argv, engine=engine)
        if rc == 0:
            for ext in (".struct.txt", ".seq.txt"):
                if os.path.exists(prefix + ext):
                    out[ext] += b"#" + name.encode() + b"\n#" + open(prefix + ext, "rb").read() + b"\n"
            counts = open(prefix + ".counts.txt", "rb").read().splitlines(True)
        else:
            m = len(pssm.read_pfm(fs if use_seq else ft)["A" if use_seq else "E"])
            W = m + 2 * flank
            text = io.StringIO()
            sites._counts_to(text, np.zeros((W, 7)), np.zeros((W, 8), dtype=np.int64) if use_seq else None, np.zeros(W, dtype=np.int64), 0)
            counts = text.getvalue().encode().splitlines(True)
        if not out[".counts.txt"]:
            out[".counts.txt"] = b"Motif\t" + counts[0]
        out[".counts.txt"] += b"".join(name.encode() + b"\t" + ln for ln in counts[1:])
    return out
