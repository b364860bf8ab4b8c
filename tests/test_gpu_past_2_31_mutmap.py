"""k_mutmap where 4 p passes 2^31.  A file of its own that sorts behind test_gpu_parity.py, whose placed-array test
decides from the free device memory: this test holds 11 GB for a moment and gives it back with torch.cuda.empty_cache()."""
import numpy as np
import pytest

import mutation_rules as rules
from conftest import assert_f32_bits_equal

pytestmark = pytest.mark.gpu


def test_past_2_31(ctx, oracle):
    """4 p passes 2^31 at p = 2^29: the outputs either side of the crossing and at the stream's end"""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 16 << 30:
        pytest.skip("needs 16 GB of free device memory, %.1f GB are free" % (free / 2 ** 30))
    m, cross, span = 8, 1 << 29, 3000
    n_pos = cross + 5000
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    d_codes = torch.randint(0, 4, (n_pos,), dtype=torch.uint8, device="cuda", generator=gen)
    d_codes[cross - 100] = 7
    d_codes[cross + 40] = 7
    d_codes[n_pos - 1] = 7
    d_best = torch.empty((n_pos, 4), dtype=torch.float32, device="cuda")
    d_where = torch.empty((n_pos, 4), dtype=torch.int8, device="cuda")
    T = rules.table(np.random.default_rng(1), m)
    torch.cuda.synchronize()
    mo = ctx.motif(T)
    ctx.mutmap_dev(mo, d_codes.data_ptr(), n_pos, d_best.data_ptr(), d_where.data_ptr())
    ctx.synchronize()
    mo.close()
    for lo, hi, at_end in ((cross - span, cross + span, False), (n_pos - span, n_pos, True)):
        codes = d_codes[lo:hi].cpu().numpy()
        want_b, want_w = rules.mutmap(oracle, codes, T)
        keep = slice(m, codes.size if at_end else codes.size - m)        # the slice's own ends cut windows the stream has
        assert_f32_bits_equal(d_best[lo:hi].cpu().numpy()[keep], want_b[keep])
        assert np.array_equal(d_where[lo:hi].cpu().numpy()[keep], want_w[keep])
    del d_best, d_where, d_codes
    torch.cuda.empty_cache()
