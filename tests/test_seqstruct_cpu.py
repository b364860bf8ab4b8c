"""``--min-seqstruct T`` on a GPU-less host: the CLI's joint threshold on the printed LogOdds.SeqStruct through every
combined mode (scores from the TEST-ONLY OracleEngine), and the arithmetic the device relies on for it -- the float32
restatement of ``np.round(x, 3)`` and the cheap superset test that keeps the float division off the fast path
(rnascan_amd/csrc/pfmscan_exact.hpp), both by brute force."""
import io
import os
import re
import shutil

import numpy as np
import pytest

from conftest import DATA_DIR, REPO
from engines import OracleEngine
from oracle import oracle
from rnascan_amd import cli

SEQ_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")
STRUCT_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt")
HIST_FA = os.path.join(DATA_DIR, "HIST2H3C_3p_end.fa")
HIST_PROFILE = os.path.join(DATA_DIR, "HIST2H3C_3p_end_structure.txt")
TEST_FA = os.path.join(DATA_DIR, "test.fa")
TEST_SEQ_PFM = os.path.join(DATA_DIR, "test_seq_pfm.txt")
TEST_STRUCT_PFM = os.path.join(DATA_DIR, "test_struct_pfm.txt")


class SumOracleEngine(OracleEngine):
    """OracleEngine + ``hits_sum`` as the issue defines it: the scanner then takes its decided-on-the-device branch"""

    calls = 0

    def hits_sum(self, stream, letter_table, struct_pssm, thr_seq, thr_struct, thr_sum, one_shot=True):
        SumOracleEngine.calls += 1
        sq, st = self.scan(stream, letter_table, struct_pssm)
        want_sum = np.round(sq, 3).astype(np.float64) + st
        pos = oracle.stream_hits(sq, st, thr_seq, thr_struct)
        pos = pos[want_sum[pos] > thr_sum]
        return pos, sq[pos], st[pos]


def _run(argv, engine=None):
    out = io.StringIO()
    cli.main(argv, engine=engine or OracleEngine(), out=out)
    return out.getvalue()


def _filtered(text, T):
    """the rows of a combined table whose printed LogOdds.SeqStruct exceeds T, Match_ID renumbered"""
    lines = text.splitlines()
    cols = lines[0].split("\t")
    at = cols.index("LogOdds.SeqStruct")
    assert cols[-1] == "Match_ID"
    kept = [l.split("\t") for l in lines[1:] if float(l.split("\t")[at]) > T]
    return "\n".join([lines[0]] + ["\t".join(f[:-1] + [str(k + 1)]) for k, f in enumerate(kept)]) + "\n"


def _sums(text):
    lines = text.splitlines()
    at = lines[0].split("\t").index("LogOdds.SeqStruct")
    return np.array([float(l.split("\t")[at]) for l in lines[1:]])


def _profile_file(path, prof):
    with open(path, "w") as f:
        f.write("PO\t" + "\t".join("BEHLMRT") + "\n")
        for k, row in enumerate(prof):
            f.write(str(k) + "\t" + "\t".join(str(float(x)) for x in row) + "\n")


def _records(path):
    from rnascan_amd import fasta
    return list(fasta.parse_sequences(path))


@pytest.fixture()
def inputs(tmp_path):
    """argv tails of every combined mode, for the SLBP pair on the HIST2H3C example and for the test pair on test.fa"""
    from rnascan_amd import store
    rng = np.random.default_rng(17)
    sets = {}
    for name, fa, p, q in (("slbp", HIST_FA, SEQ_PFM, STRUCT_PFM), ("test", TEST_FA, TEST_SEQ_PFM, TEST_STRUCT_PFM)):
        recs = _records(fa)
        d = tmp_path / (name + "_avg")
        d.mkdir()
        sfa = tmp_path / (name + "_struct.fa")
        with open(sfa, "w") as f:
            for r in recs:
                if name == "slbp":
                    shutil.copyfile(HIST_PROFILE, d / ("structure.%s.txt" % r.id))
                else:
                    _profile_file(d / ("structure.%s.txt" % r.id), rng.dirichlet(np.full(7, 0.4), size=len(r.seq)))
                f.write(">%s\n%s\n" % (r.description, "".join(rng.choice(list("EHTBLRM"), size=len(r.seq)))))
        sdir = str(tmp_path / (name + "_store"))
        assert store.main([str(d), sdir]) == 0
        head = ["-p", p, "-q", q, "-C", "0.01", "-u"]
        r0 = recs[0]
        sets[name] = {
            "directory": head + [fa, str(d)],
            "store": head + [fa, sdir],
            "two-fasta": head + [fa, str(sfa)],
            "testseq": ["-p", p, "-q", q, "-C", "0.01",
                        "-t", r0.seq + "," + "".join(rng.choice(list("EHTBLRM"), size=len(r0.seq)))],
        }
    return sets


@pytest.mark.parametrize("minscore", ["6", " -inf"])
@pytest.mark.parametrize("mode", ["directory", "store", "two-fasta", "testseq"])
@pytest.mark.parametrize("which", ["slbp", "test"])
def test_cli_keeps_the_rows_whose_printed_sum_exceeds_T(inputs, which, mode, minscore):
    argv = inputs[which][mode]
    base = _run(["-m", minscore] + argv)
    sums = _sums(base)
    if minscore == " -inf":
        assert sums.size >= 13, "every window is a row at -inf"
    if sums.size == 0:                                  # nothing above -m 6 in this input: the option changes nothing
        assert _run(["-m", minscore, "--min-seqstruct", "0"] + argv) == base
        return
    on = float(np.sort(sums)[sums.size // 2])          # T ON a printed value: strict, that row goes
    below = float(np.nextafter(on, -np.inf))           # just below it: that row stays
    for T in (on, below, float(sums.min()) - 1.0, float(sums.max())):
        want = _filtered(base, T)
        for engine in (OracleEngine(), SumOracleEngine()):          # rows filtered on the host / decided by the engine
            got = _run(["-m", minscore, "--min-seqstruct", repr(T)] + argv, engine)
            assert got == want, (which, mode, minscore, T, type(engine).__name__)
    n_on, n_below = len(_filtered(base, on).splitlines()), len(_filtered(base, below).splitlines())
    assert n_below == n_on + int((sums == on).sum())


def test_profile_modes_reach_the_engine_and_the_fallbacks_do_not(inputs):
    """directory / store: one hits_sum call per batch and pair (also at -m ' -inf'); two-FASTA and -t: rows filtered on the host"""
    for mode, expect in (("directory", True), ("store", True), ("two-fasta", False), ("testseq", False)):
        SumOracleEngine.calls = 0
        _run(["-m", " -inf", "--min-seqstruct", "-3"] + inputs["slbp"][mode], SumOracleEngine())
        assert (SumOracleEngine.calls > 0) == expect, mode


def test_library_of_pairs_is_one_engine_call_per_pair(tmp_path):
    """several motif pairs of mixed widths: the per-pair loop gives the rows of the library scan whose printed sum passes"""
    from test_scanner_cpu import _library_inputs
    lib_s, lib_t, fa, d = _library_inputs(tmp_path, n_pairs=5)
    argv = ["-p", lib_s, "-q", lib_t, "-u", "-C", "0.01", fa, d]
    for minscore in ("-2", " -inf"):
        base = _run(["-m", minscore] + argv)
        sums = _sums(base)
        assert sums.size > 10
        T = float(np.sort(sums)[sums.size // 2])
        SumOracleEngine.calls = 0
        assert _run(["-m", minscore, "--min-seqstruct", repr(T)] + argv, SumOracleEngine()) == _filtered(base, T)
        assert SumOracleEngine.calls >= 5
        assert _run(["-m", minscore, "--min-seqstruct", repr(T)] + argv) == _filtered(base, T)


def test_option_needs_both_pfms(capsys):
    with pytest.raises(SystemExit):
        cli.main(["-p", SEQ_PFM, "-u", "--min-seqstruct", "3", HIST_FA], engine=OracleEngine(), out=io.StringIO())
    with pytest.raises(SystemExit):
        cli.main(["-q", STRUCT_PFM, "-u", "--min-seqstruct", "3", HIST_FA], engine=OracleEngine(), out=io.StringIO())
    assert "--min-seqstruct" in capsys.readouterr().err


# ---- the device's arithmetic, restated in numpy -------------------------------------------------------------------
def _header_constant(name):
    text = open(os.path.join(REPO, "rnascan_amd", "csrc", "pfmscan_exact.hpp")).read()
    return float(re.search(r"constexpr double %s = ([0-9.e+-]+);" % name, text).group(1))


ROUND3_C = _header_constant("ROUND3_C")
ROUND3_SAFE = _header_constant("ROUND3_SAFE")


def round3(x):
    """the device's three operations (__fmul_rn, rintf, __fdiv_rn), each IEEE float32"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        y = x * np.float32(1000.0)
        assert y.dtype == np.float32
        return np.rint(y) / np.float32(1000.0)


def sum_maybe(x, st_fast, thr_sum, band):
    """the cheap superset test (sum_maybe): fl(fl(x + margin(x)) + st) > thr_sum, skipped where 1000 x may overflow"""
    margin0 = (0.0005 + band) * (1.0 + 2.0 ** -50)
    xd = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        mg = np.abs(xd) * (ROUND3_C * 2.0 ** -24) + margin0      # the product is exact (a power of two): one rounding, as the fma
        return ~(np.abs(xd) <= ROUND3_SAFE) | ((xd + mg) + st_fast > thr_sum)


@pytest.fixture(scope="module")
def samples():
    rng = np.random.default_rng(2024)
    parts = [
        rng.integers(0, 2 ** 32, size=6_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32),     # every exponent, NaNs, infs
        (rng.normal(0, 12, size=3_000_000)).astype(np.float32),                                           # what scores look like
        (rng.normal(0, 2e-3, size=1_000_000)).astype(np.float32),                                         # around the rounding unit
        ((np.arange(-300_000, 300_000, dtype=np.float64) + 0.5) / 1000.0).astype(np.float32),             # half-way cases ...
        np.nextafter(((np.arange(-300_000, 300_000, dtype=np.float64) + 0.5) / 1000.0).astype(np.float32), np.float32(np.inf)),
        np.nextafter(((np.arange(-300_000, 300_000, dtype=np.float64) + 0.5) / 1000.0).astype(np.float32), np.float32(-np.inf)),
        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.4e38, -3.4e38, 3.4028234e35, 3.4028236e35, 3.5e35, -3.5e35, 2.9e35,
                  8388.607, 8388.608, 8388.609, 16777.216, 1e-45, -1e-45, 1.17549435e-38, 0.0005, 0.00049999997, 0.00050000002,
                  0.0015, 0.0025], dtype=np.float32),
        (rng.uniform(2.5e35, 3.4e38, size=200_000) * rng.choice([-1, 1], size=200_000)).astype(np.float32),   # 1000 x overflows
    ]
    x = np.concatenate(parts)
    assert x.size >= 10_000_000
    return x


def test_round3_restatement_is_numpy_round_bit_for_bit(samples):
    with np.errstate(over="ignore", invalid="ignore"):
        want = np.round(samples, 3)
    got = round3(samples)
    assert got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    assert np.isinf(got[np.abs(samples) > 3.5e35]).all()              # the overflow np.round has too


def test_round3_error_bound(samples):
    """|round3(x) - x| <= 0.0005 + ROUND3_C 2^-24 |x| wherever 1000 x stays finite (the bound beside struct_band)"""
    x = samples[np.abs(samples) <= np.float32(ROUND3_SAFE)]
    xd, z = x.astype(np.float64), round3(x).astype(np.float64)
    assert (np.abs(z - xd) <= 0.0005 + ROUND3_C * 2.0 ** -24 * np.abs(xd)).all()
    # ... and the relative term is needed: half a rounding unit alone is exceeded
    assert (np.abs(z - xd) > 0.0005).any()


@pytest.mark.parametrize("struct_band", [0.0, 3e-10])
def test_superset_margin_loses_no_passing_window(samples, struct_band):
    """no x with round3(x) + st > T fails the cheap test -- with the structure score the compare ends up using (st) and
    with a fast score anywhere inside the band of it; T is put where it is hardest: one ulp under the printed sum"""
    rng = np.random.default_rng(5)
    x = samples[~np.isnan(samples)]
    z = round3(x).astype(np.float64)
    for scale in (0.0, 10.0, 1e6):
        st = rng.normal(0, 1, size=x.size) * scale
        with np.errstate(invalid="ignore", over="ignore"):
            s = z + st
            T = np.nextafter(s, -np.inf)
        ok = np.isfinite(s) | (s == np.inf)
        T = np.where(np.isfinite(T), T, np.finfo(np.float64).max)       # s = +inf passes every finite T
        passes = ok & (s > T)
        assert passes.sum() > 0.9 * x.size
        band = struct_band * (1.0 + 2.0 ** -40) + 2.0 ** -51 * np.abs(T)           # sum_band, per T
        for delta in sorted({0.0, struct_band, -struct_band}):
            maybe = sum_maybe(x, st + delta, T, band)
            assert maybe[passes].all(), (scale, delta, int((~maybe[passes]).sum()))
    # the test is not vacuous: it rejects what lies clearly below
    far = sum_maybe(x[np.abs(x) < 100], 0.0, 200.0, 0.0)
    assert not far.any()
