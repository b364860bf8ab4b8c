"""k_mutmap on the GPU against the rule (tests/mutation_rules.py over the pinned oracle): dense best bit for bit and where
exactly, in the staged and the device-pointer form; the events form; argument errors."""
import ctypes

import numpy as np
import pytest

import mutation_rules as rules
from conftest import assert_f32_bits_equal

pytestmark = pytest.mark.gpu

TILE = 1024            # MUT_TILE of csrc/pfmscan_mutation.hip: positions per workgroup
FIXED_MAX = 20         # MUT_FIXED_MAX: widths up to here run k_mutmap<M>, wider ones k_mutmap_rolled
WIDTHS = [1, 2, 3, 8, 12, 18, FIXED_MAX - 1, FIXED_MAX, FIXED_MAX + 1, FIXED_MAX + 2, 32, 63, 64]


def staged(ctx, codes, T, where=True):
    ctx.stage(np.ascontiguousarray(codes, dtype=np.uint8))
    mo = ctx.motif(T)
    try:
        return ctx.mutmap_staged(mo, where)
    finally:
        mo.close()


def check(ctx, oracle, codes, T):
    want_b, want_w = rules.mutmap(oracle, codes, T)
    got_b, got_w = staged(ctx, codes, T)
    assert_f32_bits_equal(got_b, want_b)
    assert np.array_equal(got_w, want_w)
    return want_b, want_w


def record_mix(rng, m):
    """records of every length at which the cover of a position changes shape, foreign letters at a record's first and
    last letter and m - 1 (and m) apart, and enough letters to lay records over two tile edges"""
    lengths = [1, m - 1, m, m + 1, max(2 * m - 2, 0), 2 * m - 1, 300, 700, 5, 333, 300, 300, 300, 400]
    parts = []
    for k, L in enumerate(lengths):
        c = rng.integers(0, 4, size=L).astype(np.uint8)
        if k == 10:
            c[0] = 7
        if k == 11:
            c[-1] = 7
        if k == 12:
            c[100] = c[100 + m - 1] = 7
            c[200] = c[min(200 + m, L - 1)] = 7
        parts += [c, np.asarray([7], dtype=np.uint8)]
    return np.concatenate(parts)


@pytest.mark.parametrize("m", WIDTHS)
def test_dense_map_equals_rule(ctx, oracle, m):
    rng = np.random.default_rng(m)
    codes = record_mix(rng, m)
    assert codes.size > 2 * TILE + m and codes[-1] == 7
    check(ctx, oracle, codes, rules.table(rng, m))


@pytest.mark.parametrize("m", [3, 12, FIXED_MAX + 1])
@pytest.mark.parametrize("kind", ["neginf", "bothinf", "negzero", "halves"])
def test_special_tables(ctx, oracle, m, kind):
    rng = np.random.default_rng(7 * m + len(kind))
    codes = rules.stream(rng, [m, 2 * m - 1, 150, 1, 90], foreign=0.02)
    T = rules.table(rng, m, kind)
    best, where = check(ctx, oracle, codes, T)
    if kind == "halves" and m > 2:                             # distinct windows do tie, and the lowest start wins (the largest where)
        assert (where > 0).any()
    if kind == "bothinf":
        assert np.isnan(best[codes < 4]).any() and np.isfinite(best).any()


@pytest.mark.parametrize("m", [1, 5, 12, FIXED_MAX + 3, 64])
def test_tiny_streams(ctx, oracle, m):
    rng = np.random.default_rng(m)
    T = rules.table(rng, m)
    b, w = staged(ctx, np.zeros(0, dtype=np.uint8), T)
    assert b.shape == (0, 4) and w.shape == (0, 4)
    check(ctx, oracle, np.asarray([2], dtype=np.uint8), T)
    check(ctx, oracle, np.asarray([7], dtype=np.uint8), T)
    check(ctx, oracle, rng.integers(0, 4, size=m).astype(np.uint8), T)            # n_pos = m, no separator: one window
    check(ctx, oracle, rng.integers(0, 4, size=2 * m).astype(np.uint8), T)        # the stream ends inside a record


@pytest.mark.parametrize("m", [8, FIXED_MAX, FIXED_MAX + 1, 64])
@pytest.mark.parametrize("n_pos", [TILE - 1, TILE, TILE + 1, 2 * TILE + 37])
def test_one_record_over_the_tile_edges(ctx, oracle, m, n_pos):
    """no separator near an edge: every position within m - 1 of it, on both sides, has windows in both tiles"""
    rng = np.random.default_rng(n_pos + m)
    codes = rng.integers(0, 4, size=n_pos).astype(np.uint8)
    codes[-1] = 7
    best, _ = check(ctx, oracle, codes, rules.table(rng, m))
    for edge in range(TILE, n_pos - m, TILE):
        assert np.isfinite(best[edge - m + 1:edge + m]).all()


def test_fixed_and_rolled_kernel_agree(ctx, oracle, monkeypatch):
    m = 12
    rng = np.random.default_rng(12)
    codes = record_mix(rng, m)
    T = rules.table(rng, m, "neginf")
    fixed = staged(ctx, codes, T)
    monkeypatch.setenv("PFMSCAN_MUTMAP_ROLLED", "1")
    rolled = staged(ctx, codes, T)
    monkeypatch.delenv("PFMSCAN_MUTMAP_ROLLED")
    want = rules.mutmap(oracle, codes, T)
    for got in (fixed, rolled):
        assert_f32_bits_equal(got[0], want[0])
        assert np.array_equal(got[1], want[1])


@pytest.mark.parametrize("m", [8, FIXED_MAX + 1])
def test_device_pointer_form(ctx, oracle, m):
    import torch
    rng = np.random.default_rng(m)
    codes = record_mix(rng, m)
    T = rules.table(rng, m)
    want_b, want_w = rules.mutmap(oracle, codes, T)
    d_codes = torch.from_numpy(codes).cuda()
    d_best = torch.full((codes.size, 4), 7.0, dtype=torch.float32, device="cuda")
    d_where = torch.full((codes.size, 4), 99, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    mo = ctx.motif(T)
    ctx.mutmap_dev(mo, d_codes.data_ptr(), codes.size, d_best.data_ptr(), d_where.data_ptr())
    ctx.synchronize()
    assert_f32_bits_equal(d_best.cpu().numpy(), want_b)
    assert np.array_equal(d_where.cpu().numpy(), want_w)
    d_best.fill_(7.0)
    torch.cuda.synchronize()
    ctx.mutmap_dev(mo, d_codes.data_ptr(), codes.size, d_best.data_ptr(), None)    # without where
    ctx.synchronize()
    assert_f32_bits_equal(d_best.cpu().numpy(), want_b)
    mo.close()


# ---- events ----------------------------------------------------------------------------------------------------------------
def events_case(oracle, m, seed=0):
    rng = np.random.default_rng(seed + m)
    codes = np.concatenate([record_mix(rng, m), rules.stream(rng, [200, 200], foreign=0.03)])
    T = rules.table(rng, m)
    best, _ = rules.mutmap(oracle, codes, T)
    return codes, T, best


def planted_thresholds(codes, best):
    """thr on a ref best, on an alt best, and one float32 ulp either side of each; -inf; a few ordinary ones"""
    ok = np.flatnonzero(codes < 4)
    ref = best[ok, codes[ok]]
    ref_v = np.float32(np.sort(ref[np.isfinite(ref)])[-20])
    alt = best[ok]
    alt_v = np.float32(np.sort(alt[np.isfinite(alt)])[-300])
    out = [-np.inf, 0.0, 3.0]
    for v in (ref_v, alt_v):
        out += [float(np.nextafter(v, np.float32(-np.inf))), float(v), float(np.nextafter(v, np.float32(np.inf)))]
    return out


@pytest.mark.parametrize("m", [8, FIXED_MAX + 1])
def test_events_equal_rule(ctx, oracle, m):
    codes, T, best = events_case(oracle, m)
    ctx.stage(codes)
    mo = ctx.motif(T)
    for thr in planted_thresholds(codes, best):
        want_k, want_r, want_a = rules.events(codes, best, thr)
        key, ref, alt = ctx.mutmap_events_staged(mo, thr)
        assert np.array_equal(key, want_k), thr
        assert_f32_bits_equal(ref, want_r)
        assert_f32_bits_equal(alt, want_a)
        if thr == -np.inf:                                     # only "no window -> a finite window" can be a gain
            assert key.size == 0 or (np.isnan(ref) | np.isneginf(ref) | np.isnan(alt) | np.isneginf(alt)).all()
    key, ref, alt = ctx.mutmap_events_staged(mo, np.inf)       # nothing passes: no event
    assert key.size == 0 and ref.size == 0 and alt.size == 0
    mo.close()


def test_events_capacity(ctx, oracle):
    from rnascan_amd import _lib
    m = 8
    codes, T, best = events_case(oracle, m, seed=1)
    thr = 3.0
    want_k, want_r, want_a = rules.events(codes, best, thr)
    n = want_k.size
    assert n > 10
    ctx.stage(codes)
    mo = ctx.motif(T)
    key, ref, alt = ctx.mutmap_events_staged(mo, thr, capacity=n)          # exact capacity
    assert np.array_equal(key, want_k)
    k_ = np.full(n, -5, dtype=np.int64)
    r_ = np.full(n, 9.0, dtype=np.float32)
    a_ = np.full(n, 9.0, dtype=np.float32)
    cnt = ctypes.c_int64(0)
    rc = ctx._L.pfmscan_mutmap_events_staged(ctx._h, mo._h, thr, n - 1, _lib._ptr(k_), _lib._ptr(r_), _lib._ptr(a_), ctypes.byref(cnt))
    assert rc == _lib.E_CAPACITY and cnt.value == n
    assert (k_ == -5).all() and (r_ == 9.0).all() and (a_ == 9.0).all()    # nothing written
    with pytest.raises(_lib.CapacityError) as e:
        ctx.mutmap_events_staged(mo, thr, capacity=n - 1)
    assert e.value.required == n
    mo.close()


@pytest.mark.parametrize("m", [8, FIXED_MAX + 1])
def test_events_device_pointer_form(ctx, oracle, m):
    import torch
    codes, T, best = events_case(oracle, m, seed=2)
    thr = 2.5
    want_k, want_r, want_a = rules.events(codes, best, thr)
    n = want_k.size
    mo = ctx.motif(T)
    d_codes = torch.from_numpy(codes).cuda()
    for cap in (n + 7, n // 2):
        d_key = torch.full((max(cap, 1) + 4,), -1, dtype=torch.int64, device="cuda")
        d_ref = torch.zeros(max(cap, 1) + 4, dtype=torch.float32, device="cuda")
        d_alt = torch.zeros(max(cap, 1) + 4, dtype=torch.float32, device="cuda")
        d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.mutmap_events_dev(mo, d_codes.data_ptr(), codes.size, thr, cap, d_key.data_ptr(), d_ref.data_ptr(), d_alt.data_ptr(), d_cnt.data_ptr())
        ctx.synchronize()
        assert int(d_cnt.item()) == n                          # the total, stored or not
        key = d_key.cpu().numpy()
        assert (key[cap:] == -1).all()                         # nothing beyond the capacity
        stored = min(cap, n)
        order = np.argsort(key[:stored])
        key, ref, alt = key[:stored][order], d_ref.cpu().numpy()[:stored][order], d_alt.cpu().numpy()[:stored][order]
        at = np.searchsorted(want_k, key)
        assert np.array_equal(want_k[at], key) and np.unique(key).size == stored
        assert_f32_bits_equal(ref, want_r[at])
        assert_f32_bits_equal(alt, want_a[at])
    mo.close()


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    from rnascan_amd import _lib
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 4, size=200).astype(np.uint8)
    ctx.stage(codes)
    best = np.empty((200, 4), dtype=np.float32)

    def rc_and_message(rc):
        return rc, ctx._L.pfmscan_last_error(ctx._h).decode()

    struct_only = ctx.motif(None, rng.normal(size=(6, 7)))
    rc, msg = rc_and_message(ctx._L.pfmscan_mutmap_staged(ctx._h, struct_only._h, _lib._ptr(best), None))
    assert rc == _lib.E_BADSHAPE and "no letters part" in msg
    k = ctypes.c_int64(0)
    rc, msg = rc_and_message(ctx._L.pfmscan_mutmap_events_staged(ctx._h, struct_only._h, 1.0, 0, None, None, None, ctypes.byref(k)))
    assert rc == _lib.E_BADSHAPE and "no letters part" in msg
    struct_only.close()
    wide = ctx.motif(rules.table(rng, _lib.MAX_M + 1))
    rc, msg = rc_and_message(ctx._L.pfmscan_mutmap_staged(ctx._h, wide._h, _lib._ptr(best), None))
    assert rc == _lib.E_BADSHAPE and "exceeds PFMSCAN_MAX_M" in msg
    wide.close()
    mo = ctx.motif(rules.table(rng, 6))
    rc, msg = rc_and_message(ctx._L.pfmscan_mutmap_staged(ctx._h, mo._h, None, None))
    assert rc == _lib.E_BADARG and "best is NULL" in msg
    rc, msg = rc_and_message(ctx._L.pfmscan_mutmap_events_staged(ctx._h, mo._h, float("nan"), 0, None, None, None, ctypes.byref(k)))
    assert rc == _lib.E_BADARG and "NaN threshold" in msg
    rc, msg = rc_and_message(ctx._L.pfmscan_mutmap_events_staged(ctx._h, mo._h, 1.0, 4, None, None, None, ctypes.byref(k)))
    assert rc == _lib.E_BADARG and "bad event buffers" in msg
    rc, msg = rc_and_message(ctx._L.pfmscan_mutmap_events_dev(ctx._h, mo._h, None, 0, 1.0, 0, None, None, None, None, None))
    assert rc == _lib.E_BADARG and "bad event buffers" in msg
    with pytest.raises(ValueError):
        ctx.mutmap_events_staged(mo, float("nan"))
    mo.close()
