"""The squelched FM receive bank without a GPU: csdr_amd_fmrx_squelch_plan (a host function) against its restatement, the composition of the two plans
against the sizes of the object's carries, the decidability of every block of the inputs the GPU tests use (so that those may demand exact flags), and the
exported symbols."""
import numpy as np
import pytest

import fmrx_model as fm
import fmrx_squelch_model as fsm
import squelch_model as sm

FMRX_CARRY = 2048                      # fmrx.hip: bytes per channel and plane of a carry buffer, the most filter input an object may hold
SYMBOLS = ("create_squelched", "process_squelched", "squelch_plan", "set_squelch_level", "get_squelch_level", "squelch_held", "squelch_block_index")


def test_fmrx_squelch_symbols_exported():
    import csdr_amd
    L = csdr_amd.lib()
    for name in SYMBOLS:
        assert hasattr(L, "csdr_amd_fmrx_" + name), name
    for name in ("fmrx_squelch_plan",):
        assert callable(getattr(csdr_amd, name))
    for name in ("process_squelched", "set_squelch_level", "get_squelch_level", "squelch_held", "squelch_block_index"):
        assert callable(getattr(csdr_amd.FmRx, name)), name


def test_fmrx_squelch_plan_matches_restatement():
    import csdr_amd
    for B in (1, 2, 5, 300, 301, 1024, 65536):
        helds = sorted(h for h in {0, 1, B // 2, B - 2, B - 1} if 0 <= h < B)
        for held in helds:
            complete = B - held                                          # the n_in that completes the block under way
            for n_in in {0, 1, max(complete - 1, 0), complete, complete + 1, complete + 3 * B, complete + 3 * B + 5, 7 * B - 1}:
                got = csdr_amd.fmrx_squelch_plan(held, n_in, B)
                assert got == fsm.squelch_plan(held, n_in, B), (B, held, n_in, got)
                assert got[0] % B == 0 and got[0] + got[1] == held + n_in and 0 <= got[1] < B
    assert csdr_amd.fmrx_squelch_plan(0, 0, 1024) == (0, 0) and csdr_amd.fmrx_squelch_plan(1023, 0, 1024) == (0, 1023)      # calls without input
    for bad in ((-1, 0, 1024), (0, -1, 1024), (0, 0, 0), (1024, 0, 1024)):
        with pytest.raises(csdr_amd.CsdrAmdError, match="fmrx: squelch_plan"):
            csdr_amd.fmrx_squelch_plan(*bad)


@pytest.mark.parametrize("B", [1, 300, 1024, 65536])
def test_fmrx_squelch_plans_composed_stay_within_the_carries(B):
    """chains of calls through both plans: the squelch holds fewer than B samples, the filter no more than a carry row, a call hands the chain at most
    max_samples_per_call + B - 1 samples and writes no more than the plan of that many on the fullest object (csdr_amd_fmrx_max_output's rule), and the
    chain sums to the one call"""
    import csdr_amd
    rng = np.random.default_rng(B)
    for rate in fm.RATES:
        ld = fm.taps_of(rate).size
        for block in (16, 1024, 1536):
            for _ in range(10):
                max_n = int(rng.integers(1, 3 * max(B, block)))
                calls = rng.integers(0, max_n + 1, size=rng.integers(1, 12))
                fill, held, total, blocks = fm.PREFIX, 0, 0, 0
                for k in calls:
                    m, held = csdr_amd.fmrx_squelch_plan(held, int(k), B)
                    ne, fill = csdr_amd.fmrx_plan(fill, m, ld, block)
                    assert held <= B - 1 and fill <= FMRX_CARRY and m <= max_n + B - 1
                    assert ne <= fm.plan(max(fm.PREFIX, ld + block - 1), (int(k) + B - 1) // B * B, ld, block)[0]
                    total += ne; blocks += m // B
                m_all, held_all = fsm.squelch_plan(0, int(calls.sum()), B)
                assert (total, fill) == fm.plan(fm.PREFIX, m_all, ld, block) and held == held_all and blocks == m_all // B
                assert fsm.plan(fm.PREFIX, 0, int(calls.sum()), ld, block, B) == (total, fill, held, blocks)


def test_fmrx_squelch_inputs_have_no_undecidable_block():
    """every (channel, block) of the GPU tests' inputs at their levels is decided by a margin beyond any float32 evaluation's error, and the levels do what
    the model's docstring says: some blocks close and some stay open at LEVEL, none opens at ALL_CLOSED"""
    for seed, n_ch, n in ((0, 33, fsm.N), (3, 3, fsm.N), (5, 16, fm.n_for_blocks(24, fm.taps_of(48000).size))):
        x = fsm.make_input(n_ch, n, seed)
        lv = fsm.levels(n_ch)
        for B in (1024, 300, 301, 64):
            for d in (1, 3):
                for c in range(n_ch):
                    for level in {float(lv[c]), fsm.LEVEL, fsm.ALL_CLOSED}:          # (the level tests move channels between these)
                        assert fsm.undecidable_blocks(x[c], B, d, level) == [], (seed, B, d, c, level)
                    _, pw, fl = fsm.gated(x[c], B, d, fsm.LEVEL)
                    assert 0 < fl.sum() < fl.size, (B, d, c, fl)
                    assert not fsm.gated(x[c], B, d, fsm.ALL_CLOSED)[2].any() and fsm.gated(x[c], B, d, 0.0)[2].all()
                    for k in range(pw.size):
                        P = sm.power64(x[c, k * B:(k + 1) * B], d)
                        assert abs(float(pw[k]) - P) <= sm.bound(B, d, P)
