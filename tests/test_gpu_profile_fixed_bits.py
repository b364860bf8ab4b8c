"""k_profile_fixed against the width-generic k_profile, bit for bit.

The fixed-width kernel stages a tile's codes as table offsets, addresses the letter table by its place in LDS, tests its five
sums for a non-finite one behind a single branch and has its own output path for interior tiles; none of that may change a
bit of either output.  The generic kernel (PFMSCAN_PROFILE_GENERIC=1, read at every launch) is the reference: the existing
parity tests tie it to the oracle.  Every case compares float32 sequence scores as uint32 and float64 structure scores as
uint64 (NaN payloads, infinities and the sign of zero included), all scores and the fused hits pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnascan_amd import pack  # noqa: E402

WIDTHS = list(range(9, 19))          # the widths the launcher gives to k_profile_fixed


def _stream(rng, m, dtype):
    """Six tiles of 1280 positions and a ragged end: interior tiles and the stream's last ones, records shorter than the PFM
    (also empty ones) between long ones, foreign letters (the separator's code 7, and bytes above 7: only bits 0..2 of a code
    select the table column), and profile rows that are NaN, +-inf, all zero, or hold a negative zero."""
    lengths = [2600, m - 1, 0, 1, 1900, m - 2, m, 3, 2311, m + 1, 5, 777]
    codes, profs = [], []
    for L in lengths:
        c = rng.integers(0, 4, size=L).astype(np.uint8)
        p = rng.dirichlet(np.full(7, 0.3), size=L) if L else np.zeros((0, 7))
        if L:
            p[p < 0.02] = 0.0
        if L > 100:
            c[rng.integers(0, L, size=6)] = pack.SEP
            c[rng.integers(0, L, size=6)] = rng.integers(8, 256, size=6).astype(np.uint8)
            rows = rng.integers(0, L, size=10)
            p[rows[0], rng.integers(0, 7)] = np.nan
            p[rows[1], rng.integers(0, 7)] = np.inf
            p[rows[2], rng.integers(0, 7)] = -np.inf
            p[rows[3]] = np.nan
            p[rows[4:7]] = 0.0                          # exact-zero rows: 0 * -inf in an `inf` style PSSM
            p[rows[7], rng.integers(0, 7)] = -0.0
            p[rows[8]] = -0.0
            p[rows[9], :3] = [np.inf, -np.inf, np.nan]
        codes.append(c)
        profs.append(p.astype(dtype))
    return pack.pack(codes, profs, profile_dtype=dtype)


def _pssms(rng, m, style):
    T = np.full((m, 8), np.nan)
    T[:, :4] = rng.normal(0, 2, size=(m, 4))
    P = rng.normal(-1, 2.5, size=(m, 7))
    if style == "inf":
        # a few -inf cells, not a share of them: every window whose row is non-zero at such a cell sums to -inf, and the fast
        # path and the fused hits need finite windows to work on as well
        T[rng.integers(0, m), rng.integers(0, 4)] = -np.inf
        P[rng.integers(0, m, size=2), rng.integers(0, 7, size=2)] = -np.inf
    else:
        P[rng.integers(0, m), rng.integers(0, 7)] = 0.0          # finite PSSMs with an exact zero and a negative zero
        P[rng.integers(0, m), rng.integers(0, 7)] = -0.0
    return T, P


@pytest.mark.parametrize("m", WIDTHS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("style", ["finite", "inf"])
@pytest.mark.parametrize("has_seq", [True, False])
def test_fixed_profile_kernel_has_the_generic_kernels_bits(ctx, monkeypatch, m, dtype, style, has_seq):
    rng = np.random.default_rng(7919 * m + 4 * (dtype == np.float64) + 2 * (style == "inf") + int(has_seq))
    s = _stream(rng, m, dtype)
    T, P = _pssms(rng, m, style)
    motif = ctx.motif(T if has_seq else None, P)
    codes = s.codes if has_seq else None
    monkeypatch.delenv("PFMSCAN_PROFILE_GENERIC", raising=False)
    monkeypatch.delenv("PFMSCAN_PROFILE_FIXED_MIN", raising=False)
    fixed_seq, fixed_st = ctx.scan_host(motif, codes, s.profile)
    monkeypatch.setenv("PFMSCAN_PROFILE_GENERIC", "1")
    gen_seq, gen_st = ctx.scan_host(motif, codes, s.profile)
    assert fixed_st.dtype == np.float64 and fixed_st.shape == gen_st.shape == (s.n_pos,)
    assert np.array_equal(fixed_st.view(np.uint64), gen_st.view(np.uint64))
    assert np.isfinite(gen_st).sum() > 100 and (~np.isfinite(gen_st)).sum() > 0       # both paths of the finite check ran
    if has_seq:
        assert fixed_seq.dtype == np.float32 and fixed_seq.shape == gen_seq.shape
        assert np.array_equal(fixed_seq.view(np.uint32), gen_seq.view(np.uint32))
    else:
        assert fixed_seq is None and gen_seq is None
    # the fused hits pass (seq > thr && struct > thr in the profile kernel): thresholds that about a third of the windows pass
    fin = gen_st[np.isfinite(gen_st)]
    thr_t = float(np.quantile(fin, 0.4))
    thr_s = -np.inf
    if has_seq:
        fs = gen_seq[np.isfinite(gen_seq)].astype(np.float64)
        thr_s = float(np.quantile(fs, 0.3))
    gen_hits = ctx.hits_host(motif, codes, s.profile, thr_s, thr_t)
    monkeypatch.delenv("PFMSCAN_PROFILE_GENERIC")
    fixed_hits = ctx.hits_host(motif, codes, s.profile, thr_s, thr_t)
    motif.close()
    assert len(gen_hits[0]) > 50
    assert np.array_equal(fixed_hits[0], gen_hits[0])
    assert np.array_equal(fixed_hits[2].view(np.uint64), gen_hits[2].view(np.uint64))
    if has_seq:
        assert np.array_equal(fixed_hits[1].view(np.uint32), gen_hits[1].view(np.uint32))
