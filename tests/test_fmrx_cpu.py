"""The FM receive bank without a GPU: csdr_amd_fmrx_plan (the framing rule, a host function) against its restatement, and the fairness of the oracle gates
for the inputs the GPU tests use: the kernels' fixed-point de-emphasis (csdr_amd_debug_nfm_deemph_tile) between the oracle's own stages has to pass them."""
import numpy as np
import pytest

import fmrx_model as fm

f32 = np.float32


def test_fmrx_plan_matches_restatement():
    import csdr_amd
    for rate in fm.RATES:
        ld = fm.taps_of(rate).size
        for block in (16, 512, 1024, 1536):
            for fill in list(range(ld, ld + block)) + [fm.PREFIX]:
                complete = max(ld + block - fill, 0)                     # the n_in that completes the next block
                for n_in in {0, 1, max(complete - 1, 0), complete, complete + 1, complete + 3 * block, complete + 3 * block + 5}:
                    got = csdr_amd.fmrx_plan(fill, n_in, ld, block)
                    assert got == fm.plan(fill, n_in, ld, block), (rate, block, fill, n_in, got)
                    assert got[0] % block == 0 and got[0] + got[1] == fill + n_in
                    assert got[0] == 0 or ld <= got[1] < ld + block


def test_fmrx_plan_first_calls():
    import csdr_amd
    ld = fm.taps_of(48000).size
    assert csdr_amd.fmrx_plan(fm.PREFIX, 0, ld, 1024) == (0, fm.PREFIX)
    assert csdr_amd.fmrx_plan(fm.PREFIX, ld, ld, 1024) == (1024, ld)       # a first call of exactly the taps: one block
    assert csdr_amd.fmrx_plan(fm.PREFIX, ld - 1, ld, 1024) == (0, fm.PREFIX + ld - 1)
    assert csdr_amd.fmrx_plan(ld + 1023, 1, ld, 1024) == (1024, ld)


@pytest.mark.parametrize("block", [16, 512, 1024, 1536])
def test_fmrx_plan_chain_of_calls_sums_to_one_call(block):
    import csdr_amd
    rng = np.random.default_rng(block)
    for rate in fm.RATES:
        ld = fm.taps_of(rate).size
        for _ in range(20):
            calls = rng.integers(0, 3 * block, size=rng.integers(1, 12))
            fill, total = fm.PREFIX, 0
            for k in calls:
                ne, fill = csdr_amd.fmrx_plan(fill, int(k), ld, block)
                total += ne
            one, left = csdr_amd.fmrx_plan(fm.PREFIX, int(calls.sum()), ld, block)
            assert total == one and fill == left, (rate, block, list(calls))


def test_fmrx_plan_rejects_bad_arguments():
    import csdr_amd
    for bad in ((-1, 0, 201, 1024), (0, -1, 201, 1024), (0, 0, 0, 1024), (0, 0, 201, 0)):
        with pytest.raises(csdr_amd.CsdrAmdError, match="fmrx"):
            csdr_amd.fmrx_plan(*bad)


@pytest.mark.parametrize("rate,blocks", [(48000, 7), (44100, 6), (8000, 6), (11025, 6)])
def test_fmrx_inputs_are_fair_to_the_gates(port, rate, blocks):
    """Every input kind at every rate the GPU test uses: oracle demodulator and limiter, the fixed-point de-emphasis tile by tile, oracle fastagc_ff and
    convert_f_s16, against the oracle's own float chain under the GPU test's gates.  (What differs on the GPU besides is the demodulator's reciprocal.)"""
    taps = fm.taps_of(rate)
    x = fm.make_input(len(fm.KINDS), fm.n_for_blocks(blocks, taps.size))
    for k, kind in enumerate(fm.KINDS):
        lim = fm.limited(port, x[k])
        if kind == "limit":
            assert (lim == 1.0).sum() >= 20 and (lim == -1.0).sum() >= 20          # the limiter sits at both ends
        if kind == "zeros":
            assert np.all(lim[fm.ZERO_RUNS[0][0]:fm.ZERO_RUNS[0][1]] == 0)
        de = fm.deemph_tiles(rate, lim, taps.size)
        agc = port.fastagc_ff(de, 1024, 1.0)
        want_s16, want_af = fm.expected(port, x[k], taps)
        assert want_af.size == blocks * 1024
        if kind == "agc" and rate == 48000:                                          # (the 8000 and 11025 tables have gains far from 1: no clamp there)
            de_ref = port.deemphasis_nfm_ff_cli(lim, taps)
            assert 0 < 50 * np.abs(de_ref[:3 * 1024]).max() < 1 < 50 * np.abs(de_ref[3 * 1024:4 * 1024]).max()      # three blocks at the gain clamp, then a loud one
            assert np.array_equal(want_af[2048:3072], (de_ref[:1024] * f32(50)).astype(f32)) and np.abs(want_af[4096:]).max() > 0.5
        fm.assert_gates(port.convert_f_s16(agc), agc, want_s16, want_af, what="%s @ %d" % (kind, rate))
