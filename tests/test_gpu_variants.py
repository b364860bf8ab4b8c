"""k_variants on the GPU: a list of variants x a library of letter tables equals the dense map of each motif at
[pos][alt] and [pos][codes[pos]], and equals the rule."""
import numpy as np
import pytest

import mutation_rules as rules
from conftest import assert_f32_bits_equal

pytestmark = pytest.mark.gpu

LDS_CELLS = 1024       # VAR_LDS_DOUBLES / 4 of csrc/pfmscan_mutation.hip: a motif chunk holds 1024 / m motifs
FIXED_MAX = 20         # MUT_FIXED_MAX: the dense map changes kernel behind this width


def chunk(m):
    return LDS_CELLS // m


def stream_for(rng, m):
    return rules.stream(rng, [1, m - 1, m, m + 1, 2 * m - 1, 150, 90], foreign=0.02)


def expected(oracle, codes, tables, pos, alt):
    """the rule, entry by entry of the motifs' maps"""
    n_var, n_mo = len(pos), len(tables)
    ref_s, alt_s = np.full((n_var, n_mo), np.nan, np.float32), np.full((n_var, n_mo), np.nan, np.float32)
    ref_w, alt_w = np.full((n_var, n_mo), -1, np.int8), np.full((n_var, n_mo), -1, np.int8)
    pos, alt = np.asarray(pos, dtype=np.int64), np.asarray(alt, dtype=np.int64)
    ok = np.flatnonzero((pos >= 0) & (pos < codes.size) & (alt < 4))
    ok = ok[codes[pos[ok]] < 4]
    maps = []
    for q, T in enumerate(tables):
        best, where = rules.mutmap(oracle, codes, T)
        maps.append((best, where))
        c = codes[pos[ok]]
        ref_s[ok, q], ref_w[ok, q] = best[pos[ok], c], where[pos[ok], c]
        alt_s[ok, q], alt_w[ok, q] = best[pos[ok], alt[ok]], where[pos[ok], alt[ok]]
    return (ref_s, alt_s, ref_w, alt_w), maps


def compare(got, want):
    assert_f32_bits_equal(got[0], want[0])
    assert_f32_bits_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])


@pytest.mark.parametrize("m", [1, 2, 3, 8, 12, 18, FIXED_MAX, FIXED_MAX + 1, 63, 64])
def test_widths_and_odd_variants(ctx, oracle, m):
    """duplicates, unsorted positions, alt == ref; positions on code 7, at -1 and at n_pos, alt = 7: NaN / -1, and the rows
    next to them stay right.  Also against the GPU's own dense map of each motif."""
    rng = np.random.default_rng(m)
    codes = stream_for(rng, m)
    n = codes.size
    tables = np.stack([rules.table(rng, m), rules.table(rng, m, "neginf")])
    pos = rng.integers(0, n, size=300)
    alt = rng.integers(0, 4, size=300).astype(np.uint8)
    pos[:40] = pos[40:80]                                       # duplicates, unsorted
    letters = np.flatnonzero(codes < 4)
    pos[100:120] = letters[rng.integers(0, letters.size, size=20)]
    alt[100:120] = codes[pos[100:120]]                          # alt == ref
    pos[130:140] = rng.choice(np.flatnonzero(codes == 7), size=10)   # on code 7
    pos[150], pos[151], pos[152] = -1, n, n + 5
    alt[160:165] = 7
    alt[165] = 4
    pos[200], pos[201] = 0, n - 2                               # the stream's first letter and its last
    ctx.stage(codes)
    got = ctx.variants_staged(tables, pos, alt)
    want, _ = expected(oracle, codes, tables, pos, alt)
    compare(got, want)
    assert np.isnan(got[0][[130, 150, 151, 152, 160, 165]]).all() and (got[2][[130, 150, 151, 152, 160, 165]] == -1).all()
    assert_f32_bits_equal(got[0][100:120], got[1][100:120])    # alt == ref: the ref columns twice
    assert np.array_equal(got[2][100:120], got[3][100:120])
    for q in range(2):                                          # the GPU's dense map of the same motif
        mo = ctx.motif(tables[q])
        best, where = ctx.mutmap_staged(mo)
        mo.close()
        ok = np.flatnonzero((pos >= 0) & (pos < n) & (alt < 4))
        ok = ok[codes[pos[ok]] < 4]
        assert_f32_bits_equal(got[1][ok, q], best[pos[ok], alt[ok]])
        assert_f32_bits_equal(got[0][ok, q], best[pos[ok], codes[pos[ok]]])
        assert np.array_equal(got[3][ok, q], where[pos[ok], alt[ok]]) and np.array_equal(got[2][ok, q], where[pos[ok], codes[pos[ok]]])


@pytest.mark.parametrize("n_var", [0, 1, 63, 64, 65, 3000])
def test_list_lengths(ctx, oracle, n_var):
    m = 6
    rng = np.random.default_rng(n_var)
    codes = stream_for(rng, m)
    tables = np.stack([rules.table(rng, m) for _ in range(3)])
    pos = rng.integers(-1, codes.size + 1, size=n_var)
    alt = rng.integers(0, 4, size=n_var).astype(np.uint8)
    ctx.stage(codes)
    got = ctx.variants_staged(tables, pos, alt)
    assert got[0].shape == (n_var, 3)
    compare(got, expected(oracle, codes, tables, pos, alt)[0])


@pytest.mark.parametrize("m, n_motifs", [(12, 1), (12, 2), (12, chunk(12)), (12, chunk(12) + 1), (64, chunk(64) + 1), (3, chunk(3) + 1),
                                         (64, 2 * chunk(64) + 1)])
def test_library_sizes_and_chunks(ctx, oracle, m, n_motifs):
    rng = np.random.default_rng(m + n_motifs)
    codes = rules.stream(rng, [m, 2 * m, 40], foreign=0.02)
    tables = np.stack([rules.table(rng, m) for _ in range(n_motifs)])
    pos = rng.integers(0, codes.size, size=70)
    alt = rng.integers(0, 4, size=70).astype(np.uint8)
    ctx.stage(codes)
    compare(ctx.variants_staged(tables, pos, alt), expected(oracle, codes, tables, pos, alt)[0])


def test_device_pointer_form_and_errors(ctx, oracle):
    import torch
    from rnascan_amd import _lib
    m = 9
    rng = np.random.default_rng(9)
    codes = stream_for(rng, m)
    tables = np.stack([rules.table(rng, m) for _ in range(5)])
    pos = rng.integers(-2, codes.size + 2, size=500)
    alt = rng.integers(0, 5, size=500).astype(np.uint8)
    want, _ = expected(oracle, codes, tables, pos, alt)
    d_codes, d_pos, d_alt = torch.from_numpy(codes).cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(alt).cuda()
    outs = [torch.full((500, 5), 3.0, dtype=torch.float32, device="cuda") for _ in range(2)] + \
           [torch.full((500, 5), 77, dtype=torch.int8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    ctx.variants_dev(tables, d_codes.data_ptr(), codes.size, d_pos.data_ptr(), d_alt.data_ptr(), 500, *[o.data_ptr() for o in outs])
    ctx.synchronize()
    compare([o.cpu().numpy() for o in outs], want)
    for o in outs[:2]:
        o.fill_(3.0)
    torch.cuda.synchronize()
    ctx.variants_dev(tables, d_codes.data_ptr(), codes.size, d_pos.data_ptr(), d_alt.data_ptr(), 500, outs[0].data_ptr(), outs[1].data_ptr())
    ctx.synchronize()
    assert_f32_bits_equal(outs[0].cpu().numpy(), want[0])       # without the where arrays
    assert_f32_bits_equal(outs[1].cpu().numpy(), want[1])

    def rc_and_message(rc):
        return rc, ctx._L.pfmscan_last_error(ctx._h).decode()

    ctx.stage(codes)
    p, a = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.uint8)
    r = np.zeros((1, 1), dtype=np.float32)
    wide = np.ascontiguousarray(rules.table(rng, _lib.MAX_M + 1)[None])
    rc, msg = rc_and_message(ctx._L.pfmscan_variants_staged(ctx._h, _lib._ptr(wide), 1, _lib.MAX_M + 1, _lib._ptr(p), _lib._ptr(a), 1,
                                                            _lib._ptr(r), _lib._ptr(r.copy()), None, None))
    assert rc == _lib.E_BADSHAPE and "PFMSCAN_MAX_M" in msg
    rc, msg = rc_and_message(ctx._L.pfmscan_variants_staged(ctx._h, None, 1, 8, _lib._ptr(p), _lib._ptr(a), 1, _lib._ptr(r), _lib._ptr(r.copy()), None, None))
    assert rc == _lib.E_BADSHAPE and "no letters part" in msg
    ok = np.ascontiguousarray(tables[:1])
    rc, msg = rc_and_message(ctx._L.pfmscan_variants_staged(ctx._h, _lib._ptr(ok), 1, m, _lib._ptr(p), None, 1, _lib._ptr(r), _lib._ptr(r.copy()), None, None))
    assert rc == _lib.E_BADARG and "NULL variant list or output" in msg
