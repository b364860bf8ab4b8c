"""Every structure-scoring path against the EXACT score: |score - exact| <= gamma(7 m) A (precision_rules.py), not 1e-6.

The bound is the rounding error any fp64 evaluation of the window's 7 m products can make, so a kernel that narrows a
load, keeps a float temporary, drops or doubles a term at a tile edge or applies a wrong row rule has no room in it
(test_precision_cpu.py shows each of those rejected on the CPU).  One test per path, float32 and float64 rows, a finite
PSSM (the chained form) and one with -inf cells (the per-row nan_to_num form) on inputs in which most windows stay
finite; the share of such windows is asserted BEFORE the GPU's numbers are looked at.  Each test prints its largest
error / bound (pytest -s); the threshold is 1."""
import numpy as np
import pytest

import precision_rules as pr
import test_gpu_parity
from test_gpu_parity import rand_table

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
assert pr.FIXED_WIDTHS == test_gpu_parity.FIXED_WIDTHS


def _report(path, m, dtype, with_inf, worst):
    print("precision %-28s m=%-4d %s %s  max error/bound %.4f" % (path, m, np.dtype(dtype).name, "-inf" if with_inf else "finite", worst))


def _case(m, dtype, with_inf, **kw):
    """the case, its tight share checked from the rules alone, and the reference-order scores of its tight in-record windows"""
    s, P, mask = pr.precision_case(m, dtype, with_inf, **kw)
    if P.ndim == 2:
        share, ref = pr.tight_share(s.profile, P, mask)
        assert share >= pr.MIN_TIGHT_SHARE, share
        return s, P, mask, ref
    refs = []
    for k in range(P.shape[0]):
        share, ref = pr.tight_share(s.profile, P[k], mask)
        assert share >= pr.MIN_TIGHT_SHARE, (k, share)
        refs.append(ref)
    return s, P, mask, refs


def _all_scores(ctx, path, s, P, mask, m, dtype, with_inf, codes=None, T=None):
    motif = ctx.motif(T, P)
    _, got = ctx.scan_host(motif, codes, s.profile)
    motif.close()
    pos = pr.sample_positions(s.n_pos, m, np.random.default_rng(m))
    worst, share = pr.assert_struct_tight(got if pos is None else got[pos], s.profile, P, positions=pos,
                                          in_record=mask if pos is None else mask[pos])
    assert share >= pr.MIN_TIGHT_SHARE
    _report(path, m, dtype, with_inf, worst)
    return got


def _hits_tight(path, pos, st, s, P, ref, thr, m, dtype, with_inf, eligible=None):
    """every reported structure score inside the bound; about as many hits as the reference order has above the threshold
    (hit SETS are test_gpu_threshold_exact's business)"""
    with np.errstate(invalid="ignore"):
        want = (ref > thr) if eligible is None else ((ref > thr) & eligible)
    assert want.sum() >= 20 and abs(len(pos) - int(want.sum())) <= 2 + want.sum() // 100, (len(pos), int(want.sum()))
    worst, share = pr.assert_struct_tight(st, s.profile, P, positions=pos)
    assert share == 1.0                                   # a saturated window scores -DBL_MAX-sized: never above a median
    _report(path, m, dtype, with_inf, worst)


@pytest.mark.parametrize("with_inf", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", pr.GENERIC_WIDTHS + [12])
def test_generic_profile_kernel_all_scores(ctx, monkeypatch, m, dtype, with_inf):
    """k_profile<V>: the widths without an unrolled instantiation, and w = 12 with the fixed-width kernels switched off"""
    if m == 12:
        monkeypatch.setenv("PFMSCAN_PROFILE_GENERIC", "1")
    s, P, mask, _ = _case(m, dtype, with_inf)
    _all_scores(ctx, "k_profile", s, P, mask, m, dtype, with_inf)


@pytest.mark.parametrize("with_inf", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("has_seq", [False, True])
@pytest.mark.parametrize("m", pr.FIXED_WIDTHS)
def test_fixed_width_profile_kernel_all_scores(ctx, monkeypatch, m, has_seq, dtype, with_inf):
    """k_profile_fixed, every width, with and without a letter table beside the profile"""
    monkeypatch.setenv("PFMSCAN_PROFILE_FIXED_MIN", "0")
    s, P, mask, _ = _case(m, dtype, with_inf, with_codes=True)
    T = rand_table(np.random.default_rng(m), m) if has_seq else None
    _all_scores(ctx, "k_profile_fixed", s, P, mask, m, dtype, with_inf, codes=s.codes if has_seq else None, T=T)


@pytest.mark.parametrize("with_inf", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [12, 24])
@pytest.mark.parametrize("extra", pr.TAIL_EXTRAS)
def test_stream_tails_all_scores(ctx, m, extra, dtype, with_inf):
    """one-record streams of a tile +- 1 row and of a few rows: the zero-filled staging of the last tile"""
    streams, P = pr.tail_case(m, dtype, with_inf, extra)
    motif = ctx.motif(None, P)
    worst = 0.0
    for s in streams:
        _, got = ctx.scan_host(motif, None, s.profile)
        w, _ = pr.assert_struct_tight(got, s.profile, P)
        worst = max(worst, w)
    motif.close()
    _report("tails +%d" % extra, m, dtype, with_inf, worst)


@pytest.mark.parametrize("with_inf", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [7, 12, 24])
def test_fused_hits_report_tight_scores(oracle, monkeypatch, m, dtype, with_inf):
    """hit_struct of the fused pass (k_profile / k_profile_fixed with HITS), threshold at the median"""
    from rnascan_amd import _lib
    monkeypatch.setenv("PFMSCAN_TWO_PHASE", "0")
    s, P, mask, ref = _case(m, dtype, with_inf, with_codes=True)
    thr = float(np.nanmedian(ref))
    T = rand_table(np.random.default_rng(m), m)
    with _lib.Context(0) as c:
        for codes, table in ((None, None), (s.codes, T)):
            motif = c.motif(table, P)
            pos, _, st = c.hits_host(motif, codes, s.profile, thr_seq=-np.inf, thr_struct=thr)
            motif.close()
            ok = None if codes is None else np.isfinite(oracle.stream_seq(s.codes, T))
            _hits_tight("fused hits" + ("" if codes is None else " + letters"), pos, st, s, P, ref, thr, m, dtype, with_inf, ok)


@pytest.mark.parametrize("with_inf", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [8, 12])
def test_two_phase_hits_report_tight_scores(oracle, monkeypatch, m, dtype, with_inf):
    """k_struct_at: the structure score at the letters pass's hits (a selective letter threshold keeps the two-phase route)"""
    from rnascan_amd import _lib
    monkeypatch.setenv("PFMSCAN_TWO_PHASE", "1")
    s, P, mask, ref = _case(m, dtype, with_inf, with_codes=True)
    T = rand_table(np.random.default_rng(m), m)
    want_seq = oracle.stream_seq(s.codes, T)
    thr_seq = float(np.quantile(want_seq[np.isfinite(want_seq)], 0.985))
    thr = float(np.nanquantile(ref, 0.25))
    with _lib.Context(0) as c:
        motif = c.motif(T, P)
        pos, _, st = c.hits_host(motif, s.codes, s.profile, thr_seq=thr_seq, thr_struct=thr)
        motif.close()
    _hits_tight("k_struct_at", pos, st, s, P, ref, thr, m, dtype, with_inf, want_seq > thr_seq)


@pytest.mark.parametrize("with_inf", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", pr.WIDE_WIDTHS + [100])
def test_wide_kernel_all_scores_and_hits(ctx, monkeypatch, m, dtype, with_inf):
    """k_wide: PFMs wider than k_profile takes, and w = 100 with k_profile switched off"""
    if m == 100:
        monkeypatch.setenv("PFMSCAN_WIDE_PLAIN", "1")
    s, P, mask, ref = _case(m, dtype, with_inf)
    _all_scores(ctx, "k_wide", s, P, mask, m, dtype, with_inf)
    thr = float(np.nanmedian(ref))
    motif = ctx.motif(None, P)
    pos, _, st = ctx.hits_host(motif, None, s.profile, thr_seq=-np.inf, thr_struct=thr)
    motif.close()
    _hits_tight("k_wide hits", pos, st, s, P, ref, thr, m, dtype, with_inf)


@pytest.mark.parametrize("with_inf", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 9, 25])
def test_library_phase_b_reports_tight_scores(ctx, oracle, n, dtype, with_inf):
    """k_library phase B: letters + structure, per-motif thresholds"""
    m = 12
    s, LP, mask, refs = _case(m, dtype, with_inf, n_motifs=n, with_codes=True)
    rng = np.random.default_rng(n)
    LT = np.stack([rand_table(rng, m) for _ in range(n)])
    want_seq = [oracle.stream_seq(s.codes, LT[k]) for k in range(n)]
    thr_seq = np.array([np.quantile(w[np.isfinite(w)], 0.9) for w in want_seq])
    thr_st = np.array([np.nanmedian(r) for r in refs])
    lib = ctx.library(LT, LP)
    pos, mot, _, st = ctx.library_hits_host(lib, s.codes, s.profile, thr_seq, thr_st)
    lib.close()
    for k in range(n):
        sel = mot == k
        _hits_tight("k_library[%d of %d]" % (k, n), pos[sel], st[sel], s, LP[k], refs[k], thr_st[k], m, dtype, with_inf, want_seq[k] > thr_seq[k])


@pytest.mark.parametrize("with_inf", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 16, 33])
def test_structure_library_reports_tight_scores(ctx, n, dtype, with_inf):
    """k_profile_lib: structure PFMs alone (the median as threshold for one or two motifs, the upper decile beyond: the
    exact sums of 33 x 8 000 hits would be most of this file's time)"""
    m = 12
    s, LP, mask, refs = _case(m, dtype, with_inf, n_motifs=n)
    thr_st = np.array([np.nanquantile(r, 0.5 if n <= 2 else 0.9) for r in refs])
    lib = ctx.library(None, LP)
    pos, mot, _, st = ctx.library_hits_host(lib, None, s.profile, None, thr_st)
    lib.close()
    for k in range(n):
        sel = mot == k
        _hits_tight("k_profile_lib[%d of %d]" % (k, n), pos[sel], st[sel], s, LP[k], refs[k], thr_st[k], m, dtype, with_inf)


@pytest.mark.parametrize("with_inf", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [12, 24])
def test_chunked_pipeline_reports_tight_scores(ctx, oracle, m, dtype, with_inf):
    """hits_pipeline_host at 4096 positions per chunk: the windows of a chunk's overhang are in it"""
    s, P, mask, ref = _case(m, dtype, with_inf, with_codes=True)
    thr = float(np.nanmedian(ref))
    T = rand_table(np.random.default_rng(m), m)
    for codes, table in ((None, None), (s.codes, T)):
        motif = ctx.motif(table, P)
        pos, _, st = ctx.hits_pipeline_host(motif, codes, s.profile, -np.inf, thr, 4096)
        motif.close()
        ok = None if codes is None else np.isfinite(oracle.stream_seq(s.codes, T))
        _hits_tight("pipeline" + ("" if codes is None else " + letters"), pos, st, s, P, ref, thr, m, dtype, with_inf, ok)
