"""Dot-bracket structure input, host side (no GPU): the restatement of the annotation rules against the reference
parser's output (tests/golden/dotbracket/, made by make_dotbracket_golden.py), file detection, the code LUT and the
stream position -> record mapping."""
import gzip
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from dotbracket_rules import annotate, count_letters, partners, random_structure

DB_DIR = os.path.join(GOLDEN_DIR, "dotbracket")


def load_fixtures():
    """(structures, reference letters): the committed fixture pair, one structure per line"""
    def read(name):
        with gzip.open(os.path.join(DB_DIR, name), "rt") as f:
            return f.read().split("\n")[:-1]
    s, r = read("structures.txt.gz"), read("reference.txt.gz")
    assert len(s) == len(r)
    return s, r


def test_fixtures_cover_what_they_claim():
    s, r = load_fixtures()
    assert len(s) >= 2000
    for hand in ("(((...)))", "..((..))..((..))..", "((..((...))..((...))..))", "(.(...).)", "((.(...)))", "(((...)).)", ".",
                 "...", "(...)((...))"):
        assert hand in s
    assert all("." in x for x in s)                                  # the reference's main skips lines without a dot
    assert max(len(x) for x in s) > 10000
    depth = max(max(np.cumsum([1 if c == "(" else -1 if c == ")" else 0 for c in x])) for x in s if "(" in x)
    assert depth >= 500
    span = max(max((q - i) for i, q in enumerate(partners(x)) if q > i) for x in s if "(" in x)
    assert span > 10000
    assert set("".join(r)) == set("EHTBLRM")


def test_restatement_equals_every_fixture():
    s, r = load_fixtures()
    bad = [i for i, (x, want) in enumerate(zip(s, r)) if annotate(x) != want]
    assert not bad, "restatement differs from the reference on %d structures, first #%d" % (len(bad), bad[0])


def test_hand_cases():
    assert annotate("(((...)))") == "LLLHHHRRR"
    assert annotate("..((..))..((..))..") == "EELLHHRREELLHHRREE"
    assert annotate("(.(...).)") == "LTLHHHRTR"
    assert annotate("((.(...)))") == "LLBLHHHRRR"
    assert annotate(".") == "E" and annotate("...") == "EEE" and annotate("") == ""
    assert annotate("(())") == "LLRR"                                  # dot-free records: L and R only
    with pytest.raises(ValueError):
        annotate("(()")
    with pytest.raises(ValueError):
        annotate("())")
    with pytest.raises(ValueError):
        annotate("((..[..]))")


def test_random_structures_are_balanced_and_annotated():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 3, 17, 300, 3000):
        s = random_structure(rng, n)
        assert len(s) == n
        out = annotate(s)
        assert len(out) == n and set(out) <= set("EHTBLRM")
        assert count_letters(out).sum() == n


def _write(path, records):
    with open(path, "w") as f:
        for head, body in records:
            f.write(">%s\n%s\n" % (head, body))
    return str(path)


def test_detect(tmp_path):
    from rnascan_amd import dotbracket
    letters = _write(tmp_path / "letters.fa", [("a x", "EEHHTTBBLLRRMM"), ("b", "eehh"), ("c", "")])
    db = _write(tmp_path / "db.fa", [("a", "((..))"), ("b", ""), ("c", "...")])
    dots = _write(tmp_path / "dots.fa", [("a", "...."), ("b", ".")])
    energy = _write(tmp_path / "energy.fa", [("a", "((..)).. (-1.20)"), ("b", "(...)")])
    head = _write(tmp_path / "head.fa", [("a (pairs) ((", "EEHHLLRR"), ("b ()", "MMT")])
    head_db = _write(tmp_path / "head_db.fa", [("a (pairs) ((", "..((...))")])
    mixed = _write(tmp_path / "mixed.fa", [("a", "EE((..))")])
    assert dotbracket.detect(letters) == "letters"
    assert dotbracket.detect(db) == "dotbracket"
    assert dotbracket.detect(dots) == "letters"                        # no '(': the letters path (all E either way)
    assert dotbracket.detect(energy) == "dotbracket"                   # then rejected by record
    assert dotbracket.detect(head) == "letters"                        # headers are not record bodies
    assert dotbracket.detect(head_db) == "dotbracket"
    assert dotbracket.detect(mixed) == "letters"
    assert not dotbracket.has_brackets(letters) and dotbracket.has_brackets(mixed)
    # a FASTA wrapped over several lines and a compressed one: the rule reads the bodies the same way
    wrapped = tmp_path / "wrapped.fa"
    wrapped.write_text(">a\n((..\n))..\n>b\n.(.)\n")
    assert dotbracket.detect(str(wrapped)) == "dotbracket"
    gz = tmp_path / "db.fa.gz"
    with gzip.open(gz, "wt") as f:
        f.write(">a\n((..))\n")
    assert dotbracket.detect(str(gz)) == "dotbracket"
    assert dotbracket.is_dotbracket_string("((..))") and not dotbracket.is_dotbracket_string("EEHH")
    assert not dotbracket.is_dotbracket_string("....")


def test_lut():
    from rnascan_amd import dotbracket, pack
    lut = dotbracket.LUT
    assert lut.shape == (256,) and lut.dtype == np.uint8
    assert lut[ord(".")] == 0 and lut[ord("(")] == 1 and lut[ord(")")] == 2
    others = [b for b in range(256) if chr(b) not in "()."]
    assert np.all(lut[others] == 3)
    assert pack.SEP not in lut                                        # a separator only ever comes from the packer


def test_packed_stream_and_record_of(tmp_path):
    """the FASTA packer with the dot-bracket LUT gives the kernels' input; a stream position maps back to its record
    (a record's separator belongs to it)"""
    from rnascan_amd import dotbracket, fasta
    path = _write(tmp_path / "db.fa", [("r0", "((..))"), ("r1", ""), ("r2", ".(.)[")])
    lazy = fasta.open_lazy(path)
    codes, offsets, lengths = lazy[0:3].pack_letters(dotbracket.LUT)
    assert codes.tolist() == [1, 1, 0, 0, 2, 2, 7, 7, 0, 1, 0, 2, 3, 7]
    assert offsets.tolist() == [0, 7, 8] and lengths.tolist() == [6, 0, 5]
    assert [dotbracket.record_of(offsets, p) for p in (0, 5, 6, 7, 8, 12, 13)] == [0, 0, 0, 1, 2, 2, 2]


def test_cli_option_is_registered():
    from rnascan_amd import cli
    args = cli.getoptions(["-q", "x.pfm", "s.fa"])
    assert args.struct_format == "auto"
    args = cli.getoptions(["-q", "x.pfm", "--struct-format", "dotbracket", "s.fa"])
    assert args.struct_format == "dotbracket"
    with pytest.raises(SystemExit):
        cli.getoptions(["-q", "x.pfm", "--struct-format", "vienna", "s.fa"])


def test_letters_mode_never_needs_the_device(tmp_path, capsys):
    """--struct-format letters and auto on a letters file: no annotation (no device is touched); a letters-mode file
    that holds brackets gets one hint line on stderr"""
    from rnascan_amd import cli
    db = _write(tmp_path / "db.fa", [("a", "((..))")])
    args = cli.getoptions(["-q", "x.pfm", "--struct-format", "letters", db])

    def no_engine():
        raise AssertionError("letters mode must not annotate")
    cli.struct_input(args, "SS", None, no_engine)
    assert args.fastafiles == [db]
    err = capsys.readouterr().err
    assert "--struct-format dotbracket" in err and err.count("\n") == 1
    letters = _write(tmp_path / "l.fa", [("a", "EEHH")])
    args = cli.getoptions(["-q", "x.pfm", letters])
    cli.struct_input(args, "SS", None, no_engine)
    assert args.fastafiles == [letters] and capsys.readouterr().err == ""
