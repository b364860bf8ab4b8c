"""The drivers of the occupancy family taking turns on ONE context.  They share one pass frame (csrc/pfmscan_occ.hpp) and the
context's occ_* buffers -- occ_cnt holds int window counts for one driver and int64 workgroup records for another, occ_idx
two or three prefix tables, occ_tab one or two kinds of tables -- so each call must leave nothing the next one trips over.
Every result is compared bit for bit (NaN == NaN, equal Windows) with the rules modules; there is no tolerance."""
import numpy as np
import pytest

import expect_profile_rules as eprules
import expect_rules as erules
import occupancy_profile_rules as prules
import occupancy_rules as orules
import pair_rules

pytestmark = pytest.mark.gpu

M, N_MOTIFS = 5, 3
# no window, one window, two blocks, 33 blocks in two groups
LENGTHS = [M - 1, M, 40, 32 * 32 + M + 5]


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(58)
    codes, codes2, off, lens = pair_rules.streams(rng, LENGTHS, case=True)
    n_win = np.maximum(lens - M + 1, 0)
    assert [int((n + 31) // 32) for n in n_win] == [0, 1, 2, 33]
    p = int(off[-1]) + 700                                         # one foreign position, in the last record, in both streams
    codes[p], codes2[p] = 7, 7
    profile = np.full((codes.size, 7), np.nan, dtype=np.float32)   # the separator rows hold NaN
    for o, n in zip(off, lens):
        profile[o:o + n] = prules.rows(rng, int(n), np.float32)
    R = np.stack([orules.table(rng, M, 4, 0.6, 1.7) for _ in range(N_MOTIFS)])
    S = np.stack([orules.table(rng, M, 7, 0.6, 1.7) for _ in range(N_MOTIFS)])
    T = np.stack([prules.struct_table(rng, M, 0.5, 2.0) for _ in range(N_MOTIFS)])
    # (name, scratch cap or None, the call, what the rules say)
    calls = [
        ("expect_pair", "50", lambda c: c.expect_pair_staged(R, S, pair_rules.POSTERIOR, off, lens),
         pair_rules.expected(codes, codes2, off, lens, R, S, pair_rules.POSTERIOR)),
        ("occupancy", None, lambda c: c.occupancy_staged(R, 4, off, lens), orules.occupancy(codes, off, lens, R, 4)),
        ("expect_profile", "50", lambda c: c.expect_profile_staged(T, R, eprules.POSTERIOR, off, lens),
         eprules.expected(profile, off, lens, T, codes, R, eprules.POSTERIOR)),
        ("occupancy_pair", None, lambda c: c.occupancy_pair_staged(R, S, off, lens), pair_rules.occupancy(codes, codes2, off, lens, R, S)),
        ("expect", None, lambda c: c.expect_staged(S, 7, erules.RATIO, off, lens, 1), erules.expected(codes2, off, lens, S, 7, erules.RATIO)),
        ("occupancy_profile", None, lambda c: c.occupancy_profile_staged(T, None, off, lens), prules.occupancy(profile, off, lens, T)),
    ]
    return codes, codes2, profile, calls


def test_drivers_take_turns_on_one_context(ctx, case, monkeypatch):
    codes, codes2, profile, calls = case
    ctx.stage(codes, profile)
    ctx.stage_codes2(codes2)
    for name, cap, call, want in calls + calls[::-1]:
        if cap is None:
            monkeypatch.delenv("PFMSCAN_OCC_SCRATCH_DOUBLES", raising=False)
        else:
            monkeypatch.setenv("PFMSCAN_OCC_SCRATCH_DOUBLES", cap)
        got = call(ctx)
        assert len(got) == len(want), name
        for i, (g, w) in enumerate(zip(got, want)):
            if np.asarray(w).dtype == np.int64:
                assert g.dtype == np.int64 and np.array_equal(g, w), "%s: Windows differ" % name
            else:
                assert orules.same_bits(g, w), "%s: output %d differs in its bits" % (name, i)
    assert want is calls[0][3] and name == "expect_pair"           # the reverse order ended where the forward one began
