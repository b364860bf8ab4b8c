"""k_exp_blocks past stream position 2^31, in a file of its own that runs after tests/test_gpu_parity.py, as
tests/test_gpu_past_2_31_occupancy_profile.py does: it holds 2 GB for a moment and gives torch's cache back."""
import numpy as np
import pytest

import expect_rules as rules
import occupancy_rules as orules

pytestmark = pytest.mark.gpu


def test_past_2_31(ctx):
    """codes on an untouched allocation of 2^31 + 2000 bytes: three short records named by a subset record table, one near
    the start, one across position 2^31, one that ends with the stream (_dev form)"""
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < 4e9:
        pytest.skip("needs 4 GB of free HBM, %.1f GB are free" % (free / 1e9))
    rng = np.random.default_rng(47)
    m, n_mo = 12, 2
    n_pos = 2 ** 31 + 2000
    lens = np.asarray([700, 900, 300], dtype=np.int64)
    off = np.asarray([4097, 2 ** 31 - 500, n_pos - 300], dtype=np.int64)
    assert off[1] < 2 ** 31 < off[1] + lens[1] and off[2] + lens[2] == n_pos
    d_codes = torch.empty(n_pos, dtype=torch.uint8, device="cuda")
    small, soff, _ = orules.stream(rng, lens, 4, foreign=0.01)
    for o, so, n in zip(off, soff, lens):
        d_codes[int(o):int(o + n)] = torch.from_numpy(small[so:so + n]).cuda()
    tables = np.stack([orules.table(rng, m, 4, 0.5, 2.0) for _ in range(n_mo)])
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    for mode in (rules.RATIO, rules.POSTERIOR):
        want = rules.expected(small, soff, lens, tables, 4, mode)
        d_exp = torch.full((3, n_mo, m, 8), -7.0, dtype=torch.float64, device="cuda")
        d_occ = torch.full((3, n_mo), -7.0, dtype=torch.float64, device="cuda")
        d_win = torch.full((3,), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.expect_dev(tables, 4, mode, d_codes.data_ptr(), n_pos, d_off.data_ptr(), d_len.data_ptr(), 3, d_exp.data_ptr(), d_occ.data_ptr(),
                       d_win.data_ptr())
        ctx.synchronize()
        assert rules.same_bits(d_exp.cpu().numpy(), want[0]) and rules.same_bits(d_occ.cpu().numpy(), want[1])
        assert np.array_equal(d_win.cpu().numpy(), want[2])
    del d_codes
    torch.cuda.empty_cache()
