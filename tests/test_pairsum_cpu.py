"""``--min-seqstruct T`` on two FASTA files, on a GPU-less host: the arithmetic the device decides the printed
LogOdds.SeqStruct with -- ``round3d`` (Python's ``round(x, 3)`` of a double without strings) and the cheap superset test in
front of it (rnascan_amd/csrc/pfmscan_exact.hpp, host builds of the very functions the kernels call) -- by brute force,
and ``scan_pair``'s route through an engine that has ``hits_pair_sum`` against the finished-rows filter, byte for byte."""
import io
import os

import numpy as np
import pytest

from conftest import DATA_DIR
from pairsum_helpers import PairSumLibraryOracleEngine, PairSumOracleEngine, printed_sum
from rnascan_amd import _lib, cli

TEST_FA = os.path.join(DATA_DIR, "test.fa")
TEST_SEQ_PFM = os.path.join(DATA_DIR, "test_seq_pfm.txt")
TEST_STRUCT_PFM = os.path.join(DATA_DIR, "test_struct_pfm.txt")
HIST_FA = os.path.join(DATA_DIR, "HIST2H3C_3p_end.fa")
SEQ_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_seq.txt")
STRUCT_PFM = os.path.join(DATA_DIR, "SLBP_pfm_assembled_normalized_struct.txt")


def _py_round3(x):
    return np.array([round(v, 3) for v in x.tolist()], dtype=np.float64)


def _same_bits(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def _check_round3d(x):
    """round3d against pfmscan_round_decimals everywhere (that is what the rows print), and against Python's round
    wherever round3d rounds by itself (|1000 x| < 2^52) or nothing is left to round (>= 2^53).  In between the host
    function hands x back unchanged, and so does round3d: the device must decide on the PRINTED value."""
    got = _lib.debug_round3d(x)
    assert _same_bits(got, _lib.round_decimals(x, 3))
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.abs(x * 1000.0)
    py = ~((y >= 2.0 ** 52) & (y < 2.0 ** 53))
    assert _same_bits(got[py], _py_round3(x[py]))
    return got


def test_round3d_random_doubles_over_the_exponent_range():
    rng = np.random.default_rng(77)
    bits = rng.integers(0, 2 ** 63, size=5_000_000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=5_000_000, dtype=np.uint64)
    x1 = bits.view(np.float64)                                                   # every exponent, NaNs, infs, subnormals
    x2 = rng.uniform(-1, 1, size=5_000_000) * 2.0 ** rng.integers(-40, 56, size=5_000_000)     # where rounding does something
    assert x1.size + x2.size >= 10_000_000
    _check_round3d(x1)
    got = _check_round3d(x2)
    assert (got != x2).mean() > 0.5                                              # not vacuous: most of these are changed


def test_round3d_on_the_decimal_grid_and_around_it():
    k = np.arange(-100_000, 100_001, dtype=np.float64)
    x = k / 1000.0
    parts = [x]
    up, dn = x, x
    for _ in range(2):
        up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        parts += [up, dn]
    _check_round3d(np.concatenate(parts))
    # a value of the grid is a fixed point, to the bit
    assert _same_bits(_lib.debug_round3d(x), x)
    # half-way points of the grid are not doubles (except the dyadic ones below): their two neighbours go apart
    h = (k + 0.5) / 1000.0
    parts = [h]
    up, dn = h, h
    for _ in range(2):
        up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        parts += [up, dn]
    _check_round3d(np.concatenate(parts))


def test_round3d_exact_ties():
    """odd / 16 = ....0625 exactly: 1000 x ends in .5, a TRUE tie of the exact binary value -> the even neighbour"""
    odd = np.arange(-200_001, 200_002, 2, dtype=np.float64)
    x = odd / 16.0
    assert np.array_equal(np.mod(np.abs(x * 1000.0), 1.0), np.full(x.size, 0.5))
    got = _check_round3d(x)
    r = np.rint(got * 1000.0)
    assert np.array_equal(np.mod(r, 2.0), np.zeros(x.size))                      # ties to even
    for d in (1, 2):                                                             # one and two ulps off the tie: decided by the sign
        up, dn = x, x
        for _ in range(d):
            up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        _check_round3d(np.concatenate([up, dn]))
    # larger ties, where fl(1000 x) itself is rounded: odd multiples of 1/16 up to 2^40
    big = (np.arange(1, 400_001, 2, dtype=np.float64) + 2.0 ** np.repeat(np.arange(20, 40), 10_000)[:200_000] * 16.0) / 16.0
    _check_round3d(np.concatenate([big, -big]))


def test_round3d_edges():
    lim = 2.0 ** 51 / 1000.0
    x = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, -1e-310, 0.0005, -0.0005, 0.0015, 0.0025, 0.00049999999999999999,
                  lim, np.nextafter(lim, 0), np.nextafter(lim, np.inf), -lim, 2 * lim, np.nextafter(2 * lim, 0), np.nextafter(2 * lim, np.inf),
                  4 * lim, 1e15, 1e16, 1e300, -1e300, 1.7976931348623157e308, np.inf, -np.inf, np.nan, 2251799813685.2485, 2251799813685.2495,
                  1125899906842.6245, 1125899906842.624], dtype=np.float64)
    got = _check_round3d(x)
    assert np.signbit(got[1]) and not np.signbit(got[0]) and np.signbit(got[3]) and got[3] == 0.0       # round(-5e-324, 3) == -0.0
    assert np.isnan(got[27]) and got[25] == np.inf and got[26] == -np.inf
    rng = np.random.default_rng(3)
    near = rng.uniform(0.25, 4.0, size=400_000) * lim * rng.choice([-1.0, 1.0], size=400_000)            # at and beyond 2^51 / 1000
    _check_round3d(near)


# ---- the cheap test and the exact predicate behind it ----------------------------------------------------------------
def _seq_samples(rng):
    half = ((np.arange(-40_000, 40_000, dtype=np.float64) + 0.5) / 1000.0).astype(np.float32)          # float32 round3 half-way cases
    return np.concatenate([
        rng.normal(0, 8, size=400_000).astype(np.float32), half, np.nextafter(half, np.float32(np.inf)), np.nextafter(half, np.float32(-np.inf)),
        rng.normal(0, 2e-3, size=50_000).astype(np.float32), (rng.normal(0, 1, size=50_000) * 1e6).astype(np.float32),
        np.array([0.0, -0.0, 3e35, -3e35, 3.1e35, 3.4e38, np.inf, 8388.608, 16777.216], dtype=np.float32)])


def test_joint_decision_is_the_printed_sum_and_the_cheap_test_loses_nothing():
    """for thr_sum ON the printed sum, one ulp either side of it, and on the 0.001 grid next to it: the exact step is
    `printed > thr_sum` bit for bit, and no window that passes it fails the cheap test in front of it"""
    rng = np.random.default_rng(11)
    f = _seq_samples(rng)
    n_pass = n_all = 0
    for scale in (0.0, 6.0, 1e5):
        st = rng.normal(0, 1, size=f.size) * scale
        st[::7] = np.round(st[::7] * 16.0) / 16.0 + 1.0 / 16.0                    # structure sums on (or next to) odd/16 ties
        with np.errstate(over="ignore", invalid="ignore"):
            printed = printed_sum(f, st)
        fin = np.isfinite(printed)
        grid = np.round(printed[fin], 3)
        for make in (lambda p: p, lambda p: np.nextafter(p, -np.inf), lambda p: np.nextafter(p, np.inf)):
            # one thr_sum per window is what "planted on the printed sum" means; the export takes one thr_sum per call, so
            # windows are grouped by a few hundred planted values and every window is tested against each of them
            T_all = make(printed[fin])
            for T in rng.choice(T_all, size=40, replace=False).tolist() + rng.choice(grid, size=10, replace=False).tolist():
                maybe, passes, m0 = _lib.debug_pair_sum_test(f, st, T)
                with np.errstate(invalid="ignore"):
                    want = printed > T
                assert np.array_equal(passes, want), (scale, T, int((passes != want).sum()))
                assert maybe[want].all()
                assert m0 >= 0.001 and m0 <= 0.001 + 1e-15 + 2.0 ** -49 * abs(T)
                n_pass += int(want.sum())
                n_all += want.size
        # the windows whose own printed sum IS the threshold, and its two neighbours: each against its own T
        idx = rng.choice(np.flatnonzero(fin), size=600, replace=False)
        for i in idx:
            for T in (printed[i], np.nextafter(printed[i], -np.inf), np.nextafter(printed[i], np.inf)):
                maybe, passes, _ = _lib.debug_pair_sum_test(f[i:i + 1], st[i:i + 1], T)
                assert bool(passes[0]) == bool(printed[i] > T) and (maybe[0] or not passes[0])
    assert 0.05 < n_pass / n_all < 0.95


def test_cheap_test_is_not_vacuous_and_its_margin_is_tight():
    rng = np.random.default_rng(12)
    f = rng.normal(0, 8, size=200_000).astype(np.float32)
    st = rng.normal(0, 6, size=f.size)
    T = 3.0
    maybe, passes, m0 = _lib.debug_pair_sum_test(f, st, T)
    raw = f.astype(np.float64) + st
    assert not maybe[raw < T - 0.0011].any()                  # more than the two half units (+ ulps) below: rejected at once
    assert maybe[raw > T].all()
    assert passes.mean() < 0.5 and maybe.sum() - passes.sum() < 0.001 * f.size
    # thr_sum = +inf: nothing passes; NaN is refused
    assert not _lib.debug_pair_sum_test(f, st, np.inf)[1].any()
    assert _lib.debug_pair_sum_test(f, st, -np.inf)[1].all()
    with pytest.raises(ValueError):
        _lib.debug_pair_sum_test(f, st, np.nan)


# ---- scan_pair: decided by the engine == filtered on finished rows -----------------------------------------------------
class NoPairSumEngine(PairSumOracleEngine):
    """the same engine with the method deleted: scan_pair's hasattr fall-back (finished rows through keep_seqstruct)"""

    def __getattribute__(self, name):
        if name == "hits_pair_sum":
            raise AttributeError(name)
        return object.__getattribute__(self, name)


def _run(argv, engine):
    out = io.StringIO()
    cli.main(argv, engine=engine, out=out)
    return out.getvalue()


def _sums(text):
    lines = text.splitlines()
    at = lines[0].split("\t").index("LogOdds.SeqStruct")
    return np.array([float(l.split("\t")[at]) for l in lines[1:]])


def _struct_fasta(path, fa, rng):
    from rnascan_amd import fasta
    with open(path, "w") as f:
        for r in fasta.parse_sequences(fa):
            f.write(">%s\n%s\n" % (r.description, "".join(rng.choice(list("EHTBLRMehtblrm"), size=len(r.seq)))))


@pytest.mark.parametrize("minscore", ["6", "-2", " -inf"])
@pytest.mark.parametrize("which", ["slbp", "test"])
def test_single_pair_goes_through_hits_pair_sum_and_prints_the_same_bytes(tmp_path, which, minscore):
    assert not hasattr(NoPairSumEngine(), "hits_pair_sum") and hasattr(PairSumOracleEngine(), "hits_pair_sum")
    rng = np.random.default_rng(5)
    fa, p, q = (HIST_FA, SEQ_PFM, STRUCT_PFM) if which == "slbp" else (TEST_FA, TEST_SEQ_PFM, TEST_STRUCT_PFM)
    sfa = str(tmp_path / "structs.fa")
    _struct_fasta(sfa, fa, rng)
    argv = ["-p", p, "-q", q, "-C", "0.01", "-u", fa, sfa]
    base = _run(["-m", minscore] + argv, NoPairSumEngine())
    sums = _sums(base)
    if sums.size == 0:                                  # nothing above this -m in this input: the engine is asked all the same
        Ts = [0.0]
    else:
        on = float(np.sort(sums)[sums.size // 2])
        Ts = [on, float(np.nextafter(on, -np.inf)), float(np.nextafter(on, np.inf)), float(sums.min()) - 1.0, float(sums.max())]
    for T in Ts:
        PairSumOracleEngine.calls = 0
        got = _run(["-m", minscore, "--min-seqstruct", repr(T)] + argv, PairSumOracleEngine())
        assert PairSumOracleEngine.calls == 1, "the new route was not taken"
        assert got == _run(["-m", minscore, "--min-seqstruct", repr(T)] + argv, NoPairSumEngine()), (which, minscore, T)
    # without the option nothing changes: the engine is not asked
    PairSumOracleEngine.calls = 0
    assert _run(["-m", minscore] + argv, PairSumOracleEngine()) == base and PairSumOracleEngine.calls == 0


def test_libraries_of_pairs_at_minus_inf_go_pair_by_pair(tmp_path):
    """several pairs of mixed widths: at -m ' -inf' every pair is one hits_pair_sum call; at a finite -m a width group of
    several pairs keeps the library kernel and the finished-rows filter -- the same bytes either way"""
    from test_scanner_cpu import _library_inputs
    lib_s, lib_t, fa, _ = _library_inputs(tmp_path, n_pairs=5)
    rng = np.random.default_rng(9)
    sfa = str(tmp_path / "structs.fa")
    _struct_fasta(sfa, fa, rng)
    argv = ["-p", lib_s, "-q", lib_t, "-u", "-C", "0.01", fa, sfa]
    for minscore in ("-2", " -inf"):
        base = _run(["-m", minscore] + argv, NoPairSumEngine())
        sums = _sums(base)
        assert sums.size > 10
        T = float(np.sort(sums)[sums.size // 2])
        PairSumOracleEngine.calls = 0
        got = _run(["-m", minscore, "--min-seqstruct", repr(T)] + argv, PairSumOracleEngine())
        assert got == _run(["-m", minscore, "--min-seqstruct", repr(T)] + argv, NoPairSumEngine())
        assert len(got.splitlines()) < len(base.splitlines())
        if minscore == " -inf":
            assert PairSumOracleEngine.calls >= 5


def test_libraries_of_pairs_take_the_library_route(tmp_path):
    """an engine that HAS the library methods: every width group of several pairs is one library_hits_letters_sum call, at a
    finite -m and at -m ' -inf' -- the bytes of the finished-rows filter"""
    from test_scanner_cpu import _library_inputs
    lib_s, lib_t, fa, _ = _library_inputs(tmp_path, n_pairs=7)
    rng = np.random.default_rng(10)
    sfa = str(tmp_path / "structs.fa")
    _struct_fasta(sfa, fa, rng)
    argv = ["-p", lib_s, "-q", lib_t, "-u", "-C", "0.01", fa, sfa]
    for minscore in ("-2", " -inf"):
        base = _run(["-m", minscore] + argv, NoPairSumEngine())
        sums = _sums(base)
        for T in (float(np.sort(sums)[sums.size // 2]), float(np.sort(sums)[-5])):
            PairSumLibraryOracleEngine.lib_calls = 0
            got = _run(["-m", minscore, "--min-seqstruct", repr(T)] + argv, PairSumLibraryOracleEngine())
            assert PairSumLibraryOracleEngine.lib_calls >= 1, "the library route was not taken"
            assert got == _run(["-m", minscore, "--min-seqstruct", repr(T)] + argv, NoPairSumEngine())
            assert 1 < len(got.splitlines()) < len(base.splitlines())
