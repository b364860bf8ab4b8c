"""Site profiles on FASTA inputs without a GPU: the letter-pair rule (tests/site_joint_rules.py) against the reference's own
PFM builder (tests/golden/sites/), and ``python -m rnascan_amd.sites`` on letter strings, run on the rules engine, against
files built from ``rnascan``'s own hit table for the same options."""
import gzip
import io
import json
import math
import os

import numpy as np
import pytest

import site_joint_rules as jr
from background_helpers import COLUMNS, as_ranks, write_fasta
from conftest import GOLDEN_DIR
from dotbracket_rules import annotate, random_structure
from sites_lib_helpers import SEQ_PFM, STRUCT_PFM, write_library
from rnascan_amd import cli, fasta, pack, pssm, sites

SUFFIXES = ("struct", "seq", "joint", "counts")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- 1. the rule against the reference's struct_pfm_from_aligned + norm_pfm -----------------------------------------------
@pytest.fixture(scope="module")
def golden_sites():
    with gzip.open(os.path.join(GOLDEN_DIR, "sites", "sites.json.gz")) as f:
        g = json.load(f)
    recs = g["records"]
    st = pack.pack(code_arrays=[pack.encode_rna(s) for _, s, _ in recs])
    st2 = pack.pack(code_arrays=[pack.encode_letters(t, fasta.STRUCT, keep_case=True) for _, _, t in recs])
    stream = pack.Stream(st.codes, None, st.offsets, st.lengths, codes2=st2.codes)
    pos = np.sort(np.asarray([st.offsets[r] + s for r, s in g["sites"]], dtype=np.int64))
    return g, stream, pos


@pytest.mark.parametrize("flank", [0, 3])
def test_rule_gives_the_reference_counts_and_pfm_bit_for_bit(golden_sites, flank, tmp_path):
    g, stream, pos = golden_sites
    m = g["m"]
    assert np.bincount(stream.locate(pos)[0]).max() > 4096 and {m, m + 1} <= set(stream.lengths.tolist())
    J = jr.RulesEngine().site_joint(stream, pos, None, 1, m, flank)
    assert J.shape == (1, m + 2 * flank, 8, 8) and J.dtype == np.uint64
    S, seq_counts, struct_counts, cov = sites.letter_tables(J[0].astype(np.int64), True, True)
    want_counts = np.asarray([g["counts"][str(flank)][c] for c in COLUMNS], dtype=np.int64).T
    assert sites.STRUCT_ORDER == COLUMNS and np.array_equal(struct_counts[:, sites.STRUCT_CODES], want_counts)
    assert np.array_equal(S, want_counts.astype(np.float64)) and not struct_counts[:, 7].any()
    struct, seq, foreign = sites.site_pfms(S, seq_counts)
    want = np.asarray([[float.fromhex(x) for x in g["pfm"][str(flank)][c]] for c in COLUMNS]).T
    assert np.array_equal(bits(struct), bits(want))
    # the file holds those numbers, and rnascan -q reads it back
    path = str(tmp_path / "golden.struct.txt")
    sites.write_pfm(path, sites.STRUCT_ORDER, struct)
    back = pssm.read_pfm(path)
    assert np.array_equal(bits(np.stack([back[c] for c in COLUMNS], axis=1)), bits(want))
    # the other marginal: the nucleotides, counted straight from the strings; coverage from positions and record bounds
    W = m + 2 * flank
    x = pos[:, None] - flank + np.arange(W)
    rec, _ = stream.locate(pos)
    lo = stream.offsets[rec][:, None]
    counted = (x >= lo) & (x < lo + stream.lengths[rec][:, None])
    for k in range(4):
        assert np.array_equal(seq_counts[:, k], ((stream.codes[np.where(counted, x, 0)] == k) & counted).sum(axis=0))
    assert not foreign.any() and np.array_equal(cov, sites.coverage(stream, pos, m, flank)) and np.array_equal(cov, counted.sum(axis=0))


def test_rule_one_stream_alone_and_what_it_rejects():
    codes = np.array([0, 1, 2, 7, 3, 3, 7], dtype=np.uint8)
    codes2 = np.array([6, 6 | 8, 5, 7, 0, 7, 7], dtype=np.uint8)               # bit 3: lower case; a 7 inside the second record
    off, ln = np.array([0, 4]), np.array([3, 2])
    both = jr.site_joint(codes, codes2, [0, 1, 4], [0, 1, 1], 2, off, ln, 2, 1)
    assert both.sum() == 3 + 3 + 2 and both[0, 1, 0, 6] == 1 and both[1, 1, 1, 6] == 1 and both[1, 2, 3, 7] == 1
    assert np.array_equal(jr.site_joint(codes, None, [0, 1, 4], [0, 1, 1], 2, off, ln, 2, 1)[..., 0], both.sum(axis=3))
    assert np.array_equal(jr.site_joint(None, codes2, [0, 1, 4], [0, 1, 1], 2, off, ln, 2, 1)[:, :, 0, :], both.sum(axis=2))
    for pos, mo in (([2], [0]), ([7], [0]), ([0], [2]), ([3], [0])):
        with pytest.raises(ValueError):
            jr.site_joint(codes, codes2, pos, mo, 2, off, ln, 2, 0)


def test_mutual_information():
    assert sites.mutual_information([[0] * 7] * 4) == 0.0
    assert sites.mutual_information([[5, 0, 0, 0, 0, 0, 0], [0, 5, 0, 0, 0, 0, 0], [0] * 7, [0] * 7]) == 1.0
    assert sites.mutual_information([[1, 1, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0], [0] * 7, [0] * 7]) == 0.0
    cells = [[3, 1, 0, 2, 0, 0, 1], [0, 4, 1, 0, 0, 2, 0], [1, 0, 0, 0, 5, 0, 0], [2, 2, 2, 0, 0, 0, 1]]
    n = float(sum(map(sum, cells)))
    want = math.fsum(c / n * math.log2((c / n) / ((sum(cells[a]) / n) * (sum(r[b] for r in cells) / n)))
                     for a in range(4) for b, c in enumerate(cells[a]) if c)
    assert sites.mutual_information(cells) == want and 0.0 < want < 2.0


# ---- 2. the command against rnascan's own hit table -----------------------------------------------------------------------
def _run(argv, engine=None):
    """the command in this process -> (exit code, {suffix: file bytes})"""
    prefix = argv[argv.index("-o") + 1]
    rc = sites.main(list(argv), engine=engine or jr.RulesEngine())
    out = {}
    for suffix in SUFFIXES:
        path = "%s.%s.txt" % (prefix, suffix)
        if os.path.exists(path):
            out[suffix] = open(path, "rb").read()
            os.remove(path)
    return rc, out


def _strings(path):
    return dict((r.id, r.seq) for r in fasta.open_lazy(path))


def _rnascan_hits(argv, engine):
    """rnascan's table for ``argv`` -> [(record id, 0-based start, motif (pair) name)]"""
    out = io.StringIO()
    cli.main(list(argv), engine=engine, out=out)
    lines = out.getvalue().splitlines()
    head = lines[0].split("\t")
    hits = []
    for ln in lines[1:]:
        row = dict(zip(head, ln.split("\t")))
        name = sites.pair_id(row["Motif_ID.Seq"], row["Motif_ID.Struct"]) if "Motif_ID.Seq" in row else row["Motif_ID"]
        hits.append((row["Sequence_ID"], int(row["Start"]) - 1, name))
    return hits


def _expected(hits, widths, seqs, structs, flank, all_motifs):
    """the files the command must write, from rnascan's hits counted with the plain loop; ``widths``: [(name, m)] in
    output order"""
    texts = dict((s, io.StringIO()) for s in SUFFIXES)
    written = 0
    for name, m in widths:
        mine = [(h[0], h[1], name) for h in hits if not all_motifs or h[2] == name]
        J = jr.count_table(mine, seqs, structs, [name], m, flank)[name]
        seq_counts = J.sum(axis=2) if seqs else None
        struct_counts = J.sum(axis=1) if structs else None
        S = struct_counts[:, [pack.STRUCT_LETTERS.index(c) for c in COLUMNS]].astype(np.float64) if structs else None
        parts = {}
        one = io.StringIO()
        sites._letter_counts_to(one, seq_counts, struct_counts, J.sum(axis=(1, 2)), len(mine))
        parts["counts"] = one
        if seqs and structs:
            one = io.StringIO()
            sites._joint_to(one, J)
            parts["joint"] = one
        for suffix, one in parts.items():
            lines = one.getvalue().splitlines(True)
            if not all_motifs:
                texts[suffix].write(one.getvalue())
                continue
            if not texts[suffix].tell():
                texts[suffix].write("Motif\t" + lines[0])
            texts[suffix].write("".join(name + "\t" + ln for ln in lines[1:]))
        if not mine:
            continue
        try:
            struct, seq, _ = sites.site_pfms(S, seq_counts)
        except sites.InputError:
            assert all_motifs
            continue
        for suffix, letters, matrix in (("struct", COLUMNS, struct), ("seq", "ACGU", seq)):
            if matrix is not None:
                if all_motifs:
                    texts[suffix].write("#%s\n#" % name)
                sites._pfm_to(texts[suffix], letters, matrix)
                if all_motifs:
                    texts[suffix].write("\n")
        written += 1
    if not written:
        return {}
    return dict((s, t.getvalue().encode()) for s, t in texts.items() if t.tell())


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("site_joint")
    fa, sfa, d = jr.write_letter_inputs(tmp)
    lib_seq, lib_struct, pairs = write_library(tmp)
    widths = [(n, len(pssm.read_pfm(fs)["A"])) for n, fs, _ in pairs]
    return {"tmp": tmp, "fa": fa, "sfa": sfa, "dir": d, "lib_seq": lib_seq, "lib_struct": lib_struct, "widths": widths}


# form -> (options with the single PFMs, inputs of sites, inputs of rnascan, seq strings?, struct strings?)
FORMS = {
    "seq": (["-p", "SEQ", "-m", "4"], ["fa"], ["fa"], True, False),
    "struct": (["-q", "STRUCT", "-C", "0.05", "-m", "2"], ["sfa"], ["sfa"], False, True),
    "pair": (["-p", "SEQ", "-q", "STRUCT", "-C", "0.05", "-m", "-8"], ["fa", "sfa"], ["fa", "sfa"], True, True),
    "learn": (["-p", "SEQ", "-m", "4"], ["fa", "sfa"], ["fa"], True, True),
}


def _case(inputs, form, library, flank, options=None, engine=None):
    """(exit code, files of the command, files expected from rnascan's table)"""
    opts, files, scan_files, has_seq, has_struct = FORMS[form]
    pfms = {"SEQ": inputs["lib_seq"] if library else SEQ_PFM, "STRUCT": inputs["lib_struct"] if library else STRUCT_PFM}
    opts = [pfms.get(o, o) for o in (options or opts)]
    engine = engine or jr.RulesEngine()
    hits = _rnascan_hits(opts + [inputs[f] for f in scan_files], engine)
    widths = inputs["widths"] if library else [("the one motif", 18)]
    want = _expected(hits, widths, _strings(inputs["fa"]) if has_seq else None, _strings(inputs["sfa"]) if has_struct else None,
                     flank, library)
    argv = opts + (["--all-motifs"] if library else []) + ["--flank", str(flank), "-o", str(inputs["tmp"] / "out")] + [inputs[f] for f in files]
    rc, got = _run(argv, engine)
    return rc, got, want, hits


@pytest.mark.parametrize("flank", [0, 3])
@pytest.mark.parametrize("library", [False, True], ids=["one", "all"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_command_equals_rnascans_own_hits_counted_by_the_plain_loop(inputs, form, library, flank):
    rc, got, want, hits = _case(inputs, form, library, flank)
    assert rc == 0 and len(hits) > 20
    assert sorted(got) == sorted(want) == sorted({"seq": ["counts", "seq"], "struct": ["counts", "struct"]}.get(form, list(SUFFIXES)))
    for suffix in want:
        assert got[suffix] == want[suffix], suffix
    if library:
        assert len({h[2] for h in hits}) >= 3


@pytest.mark.parametrize("engine", [jr.RulesEngine, jr.PlainEngine], ids=["device-side", "host-side"])
@pytest.mark.parametrize("library", [False, True], ids=["one", "all"])
@pytest.mark.parametrize("minscore", ["-30", " -inf"])
def test_min_seqstruct_selects_rnascans_rows(inputs, minscore, library, engine):
    options = ["-p", "SEQ", "-q", "STRUCT", "-C", "0.05", "-m", minscore, "--min-seqstruct", "-20"]
    rc, got, want, hits = _case(inputs, "pair", library, 1, options, engine())
    assert rc == 0 and len(hits) > 50
    assert sorted(got) == sorted(want) == sorted(SUFFIXES)
    for suffix in want:
        assert got[suffix] == want[suffix], suffix


def _case_options(inputs, library, options):
    pfms = {"SEQ": inputs["lib_seq"] if library else SEQ_PFM, "STRUCT": inputs["lib_struct"] if library else STRUCT_PFM}
    return [pfms.get(o, o) for o in options]


def test_struct_pfm_closes_the_loop(inputs):
    """scan -> site PFM -> scan again: rnascan -q reads P.struct.txt, -p reads P.seq.txt"""
    prefix = str(inputs["tmp"] / "loop")
    argv = _case_options(inputs, False, FORMS["pair"][0]) + ["-o", prefix, inputs["fa"], inputs["sfa"]]
    assert sites.main(argv, engine=jr.RulesEngine()) == 0
    assert sorted(s for s in SUFFIXES if os.path.exists("%s.%s.txt" % (prefix, s))) == sorted(SUFFIXES)
    again = _rnascan_hits(["-p", prefix + ".seq.txt", "-q", prefix + ".struct.txt", "-C", "0.05", "-m", "2", inputs["fa"], inputs["sfa"]],
                          jr.RulesEngine())
    assert len(again) > 10
    head = open(prefix + ".joint.txt").readline().rstrip("\n").split("\t")
    assert head == ["PO"] + ["%s.%s" % (a, b) for a in "ACGU" for b in "BEHLMRT"] + ["MI"]
    head = open(prefix + ".counts.txt").readline().rstrip("\n").split("\t")
    assert head == ["PO", "Sites", "Coverage"] + ["Count." + c for c in "ACGUN"] + ["Count." + c for c in "BEHLMRTX"]
    for suffix in SUFFIXES:
        os.remove("%s.%s.txt" % (prefix, suffix))


# ---- 3. invariance --------------------------------------------------------------------------------------------------------
INVARIANT = [(["-p", "SEQ", "-q", "STRUCT", "-C", "0.05", "-m", "-30", "--min-seqstruct", "-20", "--flank", "2"], False),
             (["-p", "SEQ", "-q", "STRUCT", "-C", "0.05", "-m", "-8", "--flank", "2"], True),
             (["-q", "STRUCT", "-C", "0.05", "-m", "2", "--flank", "2"], True)]


@pytest.mark.parametrize("options,library", INVARIANT, ids=["one-pair", "all-pairs", "all-struct"])
def test_bytes_do_not_depend_on_batches_ranks_or_record_order(inputs, options, library, monkeypatch, tmp_path):
    prefix = str(inputs["tmp"] / "inv")
    tail = (["--all-motifs"] if library else []) + ["-o", prefix]

    def files(fa, sfa):
        return [fa, sfa] if "-p" in options else [sfa]
    argv = _case_options(inputs, library, options) + tail + files(inputs["fa"], inputs["sfa"])
    rc, one = _run(argv)
    assert rc == 0 and "counts" in one and "struct" in one
    for batch in ("1", "300", "2000"):
        monkeypatch.setenv("RNASCAN_BATCH_POSITIONS", batch)
        assert _run(argv) == (0, one)
    monkeypatch.delenv("RNASCAN_BATCH_POSITIONS")
    for world in (2, 3):
        def ranked(rank, w, dist):
            return sites.main_letters(jr.RulesEngine(), sites.getoptions(argv), rank, w, dist)
        assert as_ranks(world, ranked) == [0] * world
        got = {}
        for suffix in SUFFIXES:
            path = "%s.%s.txt" % (prefix, suffix)
            if os.path.exists(path):
                got[suffix] = open(path, "rb").read()
                os.remove(path)
        assert got == one
    rfa, rsfa, _ = jr.write_letter_inputs(tmp_path / "rev", reverse=True)
    assert [r.id for r in fasta.open_lazy(rfa)] == [r.id for r in fasta.open_lazy(inputs["fa"])][::-1]
    assert _run(_case_options(inputs, library, options) + tail + files(rfa, rsfa)) == (0, one)


class _Failing(jr.RulesEngine):
    def site_joint(self, *a, **k):
        raise ValueError("this rank's counting failed")


def test_a_failing_rank_hands_its_error_to_every_rank(inputs, tmp_path):
    argv = _case_options(inputs, False, FORMS["pair"][0]) + ["-o", str(tmp_path / "x"), inputs["fa"], inputs["sfa"]]
    got = as_ranks(3, lambda r, w, dist: sites.main_letters(_Failing() if r == 1 else jr.RulesEngine(), sites.getoptions(argv), r, w, dist))
    assert all(isinstance(g, ValueError) and "this rank's counting failed" in str(g) for g in got), got
    assert not os.path.exists(str(tmp_path / "x.counts.txt"))


# ---- 4. edges -------------------------------------------------------------------------------------------------------------
def test_files_that_do_not_pair_name_the_record_and_write_nothing(inputs, tmp_path, capfd):
    seqs, structs = _strings(inputs["fa"]), _strings(inputs["sfa"])
    ids = list(seqs)
    base = _case_options(inputs, False, FORMS["pair"][0]) + ["-o", str(tmp_path / "x"), inputs["fa"]]
    swapped = ids[:3] + [ids[4], ids[3]] + ids[5:]
    cases = {"swapped": ([(i, structs[i]) for i in swapped], ids[3]),
             "missing": ([(i, structs[i]) for i in ids[:-1]], ids[-1]),
             "extra": ([(i, structs[i]) for i in ids] + [("more", "EEEE")], "more"),
             "twice": ([(i, structs[i]) for i in ids[:2] + ids[1:]], ids[2]),
             "short": ([(i, structs[i][:-1] if i == ids[7] else structs[i]) for i in ids], ids[7])}
    for name, (records, culprit) in cases.items():
        path = str(tmp_path / (name + ".fa"))
        write_fasta(path, records)
        capfd.readouterr()
        rc, files = _run(base + [path])
        err = capfd.readouterr().err
        assert rc == 1 and files == {} and culprit in err, (name, err)
        if name == "short":
            assert "letters long" in err
    twice = str(tmp_path / "twice_seq.fa")
    write_fasta(twice, [(i, seqs[i]) for i in ids[:2] + ids[1:]])
    rc, files = _run(base[:-1] + [twice, str(tmp_path / "twice.fa")])
    assert rc == 1 and files == {} and "more than once" in capfd.readouterr().err


def test_dot_bracket_structures_equal_their_annotated_letters(tmp_path, capfd):
    rng = np.random.default_rng(11)
    seqs = [("d%02d" % i, "".join(rng.choice(list("ACGU"), size=int(rng.integers(30, 200))))) for i in range(12)]
    db = [(rid, random_structure(rng, len(s))) for rid, s in seqs]
    fa, dbfa, sfa = str(tmp_path / "seqs.fa"), str(tmp_path / "db.fa"), str(tmp_path / "letters.fa")
    write_fasta(fa, seqs)
    write_fasta(dbfa, db)
    write_fasta(sfa, [(rid, annotate(s)) for rid, s in db])
    for options, both in ((["-q", STRUCT_PFM, "-C", "0.05", "-m", "-12"], False),
                          (["-p", SEQ_PFM, "-q", STRUCT_PFM, "-C", "0.05", "-m", "-16", "--flank", "2"], True)):
        base = options + ["-o", str(tmp_path / "x")] + ([fa] if both else [])
        rc, want = _run(base + [sfa])
        assert rc == 0 and len(want) == (4 if both else 2)
        capfd.readouterr()
        assert _run(base + [dbfa]) == (0, want)
        assert "Annotating dot-bracket structures" in capfd.readouterr().err
        assert _run(["--struct-format", "dotbracket"] + base + [dbfa]) == (0, want)
    with pytest.raises(SystemExit):
        sites.getoptions(["-q", STRUCT_PFM, "-o", "x", "--struct-format", "fragments", dbfa])


def test_lower_case_structure_letters_count_under_their_letter(inputs, tmp_path):
    structs = _strings(inputs["sfa"])
    assert any(s != s.upper() for s in structs.values())
    upper = str(tmp_path / "upper.fa")
    write_fasta(upper, [(i, s.upper()) for i, s in structs.items()])
    # -u: the computed structure background counts the letters as written (rnascan.py:444-457), the scores do not
    base = _case_options(inputs, False, FORMS["pair"][0]) + ["-u", "--flank", "2", "-o", str(tmp_path / "x"), inputs["fa"]]
    rc, want = _run(base + [upper])
    assert rc == 0 and _run(base + [inputs["sfa"]]) == (0, want)


def test_foreign_characters_in_flanks_are_counted_apart(tmp_path, capfd):
    cons = jr.struct_consensus()
    site = "AAAGGCUCUUUUCAGAGC"
    fa, sfa = str(tmp_path / "s.fa"), str(tmp_path / "t.fa")
    write_fasta(fa, [("a", "N" + site + "NG"), ("b", "CC" + site + "CC")])
    write_fasta(sfa, [("a", "?" + cons + "Ee"), ("b", "ee" + cons.lower() + "hh")])
    rc, files = _run(["-p", SEQ_PFM, "-q", STRUCT_PFM, "-u", "-C", "0.05", "-m", "6", "--flank", "2", "-o", str(tmp_path / "x"), fa, sfa])
    err = capfd.readouterr().err
    assert rc == 0 and "Found 2 sites" in err
    assert "Foreign letters under the sites, left out of the sequence PFM: 2 (per column: 0 1 " in err
    assert "Foreign structure characters under the sites, left out of the structure PFM: 1 (per column: 0 1 0 " in err
    rows = [ln.split("\t") for ln in files["counts"].decode().splitlines()]
    col = dict((name, [int(r[k]) for r in rows[1:]]) for k, name in enumerate(rows[0]))
    W = 18 + 4
    assert col["Sites"] == [2] * W and col["Coverage"] == [1] + [2] * 21
    assert col["Count.N"] == [0, 1] + [0] * 18 + [1, 0] and col["Count.X"] == [0, 1] + [0] * 20
    assert col["Count.G"][-1] == 1 and col["Count.E"][-2:] == [1, 1]
    assert sum(col["Count." + c][5] for c in "ACGU") == 2 == sum(col["Count." + c][5] for c in "BEHLMRT")
    joint = [ln.split("\t") for ln in files["joint"].decode().splitlines()]
    assert sum(int(x) for x in joint[2][1:-1]) == 1 and float(joint[2][-1]) == 0.0          # the foreign pair is no known cell
    assert sum(int(x) for x in joint[3][1:-1]) == 2


def test_zero_sites_and_an_uncovered_column(inputs, tmp_path, capfd):
    rc, files = _run(["-p", SEQ_PFM, "-m", "50", "-o", str(tmp_path / "none"), inputs["fa"], inputs["sfa"]])
    assert rc == 1 and files == {} and "Found 0 sites" in capfd.readouterr().err
    fa = str(tmp_path / "s.fa")
    write_fasta(fa, [("a", "AAAGGCUCUUUUCAGAGC")])
    rc, files = _run(["-p", SEQ_PFM, "-u", "-m", "2", "--flank", "1", "-o", str(tmp_path / "x"), fa])
    assert rc == 1 and files == {} and "column 0" in capfd.readouterr().err


def test_a_directory_still_takes_the_profile_route(inputs, tmp_path, monkeypatch):
    def never(*a, **k):
        raise AssertionError("the FASTA route was taken")
    monkeypatch.setattr(jr.RulesEngine, "site_joint", never)
    rc, files = _run(["-p", SEQ_PFM, "-m", "4", "--flank", "2", "-o", str(tmp_path / "x"), inputs["fa"], inputs["dir"]])
    assert rc == 0 and sorted(files) == ["counts", "seq", "struct"]
    assert files["counts"].startswith(b"PO\tSites\tCoverage\tSum.B\t")
    rc, files = _run(["-p", SEQ_PFM, "-m", "4", "-o", str(tmp_path / "x"), inputs["fa"], str(tmp_path / "nothing_here")])
    assert rc == 1 and files == {}


def test_a_library_too_large_for_its_tables_is_refused(inputs, tmp_path, monkeypatch, capfd):
    monkeypatch.setattr(sites, "ACC_LIMIT", 2 * 18 * 64 * 8 - 1)
    rc, files = _run(["-p", inputs["lib_seq"], "-m", "4", "--all-motifs", "-o", str(tmp_path / "x"), inputs["fa"]])
    assert rc == 1 and files == {} and "split the library" in capfd.readouterr().err
