"""k_expp_blocks past 2^31 profile elements and 2^32 bytes, in a file of its own that runs AFTER
tests/test_gpu_parity.py, as tests/test_gpu_past_2_31_occupancy_profile.py does: it holds 9 GB for a moment and gives torch's
cache back."""
import numpy as np
import pytest

import expect_profile_rules as rules
import occupancy_profile_rules as prules
import occupancy_rules as orules

pytestmark = pytest.mark.gpu


def test_past_2_31(ctx):
    """float32 rows on an untouched allocation: three records, one across float32 element 2^31 (row 306 783 378), one
    across byte offset 2^32 (row 153 391 689), one at the end, named by a subset record table (_dev form); the three forms"""
    import torch
    from rnascan_amd import _lib
    free = torch.cuda.mem_get_info()[0]
    if free < 12e9:
        pytest.skip("needs 12 GB of free HBM, %.1f GB are free" % (free / 1e9))
    rng = np.random.default_rng(53)
    m, n_mo = 12, 2
    n_pos = 306783378 + 2000
    assert 153391689 * 28 < 2 ** 32 < 153391690 * 28 and 306783378 * 7 <= 2 ** 31 < 306783379 * 7    # both inside a record below
    lens = np.asarray([700, 900, 300], dtype=np.int64)
    off = np.asarray([153391690 - 350, 306783378 - 500, n_pos - 301], dtype=np.int64)
    d_prof = torch.empty((n_pos, 7), dtype=torch.float32, device="cuda")
    d_codes = torch.empty(n_pos, dtype=torch.uint8, device="cuda")
    small_codes, small_prof, soff, _ = prules.stream(rng, lens, np.float32, foreign=0.01)
    for o, so, n in zip(off, soff, lens):
        d_prof[int(o):int(o + n)] = torch.from_numpy(small_prof[so:so + n]).cuda()
        d_prof[int(o + n)] = float("nan")                               # the separator row
        d_codes[int(o):int(o + n)] = torch.from_numpy(small_codes[so:so + n]).cuda()
    st = np.stack([prules.struct_table(rng, m) for _ in range(n_mo)])
    sq = np.stack([orules.table(rng, m) for _ in range(n_mo)])
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    for a, b in ((st, None), (st, sq), (None, sq)):
        want = rules.expected(small_prof, soff, lens, a, small_codes, b, rules.POSTERIOR)
        d_st = torch.full((3, n_mo, m, 8), -7.0, dtype=torch.float64, device="cuda")
        d_sq = torch.full((3, n_mo, m, 8), -7.0, dtype=torch.float64, device="cuda")
        d_occ = torch.full((3, n_mo), -7.0, dtype=torch.float64, device="cuda")
        d_win = torch.full((3,), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.expect_profile_dev(a, b, rules.POSTERIOR, d_codes.data_ptr(), d_prof.data_ptr(), _lib.PROFILE_F32, n_pos, d_off.data_ptr(),
                               d_len.data_ptr(), 3, d_st.data_ptr(), d_sq.data_ptr() if b is not None else None, d_occ.data_ptr(), d_win.data_ptr())
        ctx.synchronize()
        got = (d_st.cpu().numpy(), d_sq.cpu().numpy() if b is not None else None, d_occ.cpu().numpy(), d_win.cpu().numpy())
        assert rules.same(got, want)
    del d_prof, d_codes
    torch.cuda.empty_cache()
