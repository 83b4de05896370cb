"""The squelched WFM receive bank without a GPU: csdr_amd_wfmrx_squelch_plan (a host function) against its restatement, the composition of the two plans
against check values computed with the model, the decidability of every block of the inputs the GPU tests use (so that those may demand exact flags), the
fairness of the oracle gates on the gated streams, and the exported symbols.

Only the symbol, signature and plan tests run code of the library's squelched bank (they fail without it).  The decidability, flag-pattern, fairness,
compiled-reference and long-tail-input tests touch the Python models and the oracle alone: they pass whatever the library does and are no coverage of it.
They are here because the GPU tests' demands rest on them: exact flags need every block decidable, and the gates need the reference itself to pass them."""
import inspect

import numpy as np
import pytest

import squelch_model as sm
import wfmrx_model as wm
import wfmrx_squelch_model as wsm

SYMBOLS = ("create_squelched", "process_squelched", "squelch_plan", "set_squelch_level", "get_squelch_level", "squelch_held", "squelch_block_index")
BD = [(1024, 1), (1024, 3), (300, 1), (300, 3), (301, 1)]              # the (squelch block, use_every_nth) pairs of the GPU tests
GPU_CASES = [(5, 12), (2.5, 12), (5.2083335, 12), (3.3, 12), (5, 4)]   # their (rate, num_poly_points)


def test_wfmrx_squelch_symbols_exported():
    import csdr_amd
    L = csdr_amd.lib()
    for name in SYMBOLS:
        assert hasattr(L, "csdr_amd_wfmrx_" + name), name
    assert callable(csdr_amd.wfmrx_squelch_plan)
    for name in ("process_squelched", "process_squelched_dev", "set_squelch_level", "get_squelch_level", "squelch_held", "squelch_block_index"):
        assert callable(getattr(csdr_amd.WfmRx, name)), name
    for f in (csdr_amd.WfmRx.__init__, csdr_amd.Context.wfm_rx):
        p = inspect.signature(f).parameters
        assert (p["squelch_block"].default, p["use_every_nth"].default, p["levels"].default) == (0, 1, None)
    assert list(inspect.signature(csdr_amd.WfmRx.process_squelched_dev).parameters) == list(inspect.signature(csdr_amd.FmRx.process_squelched_dev).parameters)
    assert list(inspect.signature(csdr_amd.WfmRx.process_squelched).parameters) == list(inspect.signature(csdr_amd.FmRx.process_squelched).parameters)


def test_wfmrx_squelch_plan_matches_restatement():
    import csdr_amd
    for B in (1, 2, 5, 300, 301, 1024, 65536):
        helds = sorted(h for h in {0, 1, B // 2, B - 2, B - 1} if 0 <= h < B)
        for held in helds:
            complete = B - held                                          # the n_in that completes the block under way
            for n_in in {0, 1, max(complete - 1, 0), complete, complete + 1, complete + 3 * B, complete + 3 * B + 5, 7 * B - 1}:
                got = csdr_amd.wfmrx_squelch_plan(held, n_in, B)
                assert got == wsm.squelch_plan(held, n_in, B), (B, held, n_in, got)
                assert got[0] % B == 0 and got[0] + got[1] == held + n_in and 0 <= got[1] < B
    assert csdr_amd.wfmrx_squelch_plan(0, 0, 1024) == (0, 0) and csdr_amd.wfmrx_squelch_plan(1023, 0, 1024) == (0, 1023)      # calls without input
    for bad in ((-1, 0, 1024), (0, -1, 1024), (0, 0, 0), (1024, 0, 1024)):
        with pytest.raises(csdr_amd.CsdrAmdError, match="wfmrx: squelch_plan"):
            csdr_amd.wfmrx_squelch_plan(*bad)


def chain(calls, B, rate=5, P=12, W=1024):
    """the library's two plans over a chain of calls on a fresh object -> [(m, outputs, floats held, squelch samples held)] per call"""
    import csdr_amd
    where, held, sq, out = wm.fresh_where(P), 0, 0, []
    for k in calls:
        m, sq = csdr_amd.wfmrx_squelch_plan(sq, k, B)
        n_out, where, held = csdr_amd.wfmrx_plan(rate, P, 0, W, where, held, m)
        out.append((m, n_out, held, sq))
    return out


def test_wfmrx_squelch_plans_composed_check_values():
    """rate 5, 12 points, windows of 1024, a fresh object; the values were computed with the model (wfmrx_model.plan behind squelch_plan)"""
    N = wsm.N
    assert chain([N], 1024) == [(7168, 1414, 99, 37)]
    assert chain([N], 300) == [(7200, 1414, 131, 5)]
    assert chain([N], 301) == [(6923, 1212, 864, 282)]
    calls = wsm.RAGGED + [N - sum(wsm.RAGGED)]
    at_1024 = [(0, 0, 0, 341), (0, 0, 0, 341), (0, 0, 0, 342), (2048, 404, 29, 347), (5120, 1010, 99, 37)]
    at_300 = [(300, 0, 300, 41), (0, 0, 300, 41), (0, 0, 300, 42), (1800, 404, 81, 295), (5100, 1010, 131, 5)]
    assert chain(calls, 1024) == at_1024 and chain(calls, 300) == at_300
    assert sum(c[1] for c in at_1024) == sum(c[1] for c in at_300) == 1414
    for B in (1024, 300, 301):                                           # the restatement says the same
        where, held, sq = wm.fresh_where(12), 0, 0
        for k, want in zip(calls, chain(calls, B)):
            n_out, where, held, sq, blocks = wsm.plan(5, 12, 0, 1024, where, held, sq, k, B)
            assert (blocks * B, n_out, held, sq) == want


@pytest.mark.parametrize("B", [1, 300, 1024, 65536])
def test_wfmrx_squelch_plans_composed_stay_within_the_carries(B):
    """chains of random calls through both plans: the squelch holds fewer than B samples, the decimator fewer than a window, a call hands the chain at most
    max_samples_per_call + B - 1 samples and writes no more than csdr_amd_wfmrx_max_output's rule allows, and the chain sums to the one call"""
    import csdr_amd
    rng = np.random.default_rng(B)
    W = 1024
    for rate, P in GPU_CASES:
        for _ in range(10):
            max_n = int(rng.integers(1, 3 * max(B, W)))
            calls = [int(k) for k in rng.integers(0, max_n + 1, size=rng.integers(1, 12))]
            got = chain(calls, B, rate, P)
            for k, (m, n_out, held, sq) in zip(calls, got):
                assert sq <= B - 1 and held <= W - 1 and m <= max_n + B - 1
                assert n_out <= int(np.floor((W + k + B - 1) / float(np.float32(rate)))) + 2
            m_all, sq_all = wsm.squelch_plan(0, sum(calls), B)
            one = wm.plan(rate, P, 0, W, wm.fresh_where(P), 0, m_all)
            assert sum(c[1] for c in got) == one[0] and got[-1][3] == sq_all and sum(c[0] for c in got) == m_all
            if m_all:
                assert [c[2] for c in got if c[0]][-1] == one[2]


def bits(fl):
    return "".join(str(int(v)) for v in fl)


def test_wfmrx_squelch_inputs_have_no_undecidable_block():
    """every (channel, block) of the GPU tests' inputs at their levels is decided by a margin beyond any float32 evaluation's error, and the flags are the
    ones the issue states: open -> closed and closed -> open edges, a closed block across a window boundary and across a call seam"""
    nearest = np.inf
    for n_ch in (1, 5, 17):
        x, lv = wsm.make_input(n_ch), wsm.levels(n_ch)
        for B in (1024, 300, 301):
            for d in (1, 3):
                for c in range(n_ch):
                    kind = wm.KINDS[c % 4]
                    for level in {float(lv[c]), wsm.ALL_CLOSED}:         # (the level tests move channels between these and 0)
                        assert wsm.undecidable_blocks(x[c], B, d, level) == [], (n_ch, B, d, c, level)
                    _, pw, fl = wsm.gated(x[c], B, d, lv[c])
                    for k in range(pw.size):
                        P = sm.power64(x[c, k * B:(k + 1) * B], d)
                        assert abs(float(pw[k]) - P) <= sm.bound(B, d, P)
                        if lv[c] > 0 and P > 0:
                            nearest = min(nearest, max(P / float(lv[c]), float(lv[c]) / P))
                    if c == 4 or kind == "allzero":
                        assert not fl.any()
                    elif c == 5:
                        assert fl.all()
                    elif B == 1024:
                        assert bits(fl) == "1011011", (c, d)
                    elif B == 300:
                        assert bits(fl) == "111000011111110001111111", (c, d)
                    else:
                        assert 0 < fl.sum() < fl.size
    print("the nearest block power is a factor %.3f from its level" % nearest)
    assert nearest > 1.02


def long_tail_input():
    """one fm channel with the samples from 1024 on scaled by 0.05: at B = 1024 and LEVEL one open block, then closed ones"""
    x = wm.make_input(1, wsm.N).copy()
    x[:, 1024:] *= np.float32(0.05)
    return x


def test_wfmrx_squelch_long_tail_input():
    x = long_tail_input()
    assert wsm.undecidable_blocks(x[0], 1024, 1, wsm.LEVEL) == [] and bits(wsm.gated(x[0], 1024, 1, wsm.LEVEL)[2]) == "1000000"


@pytest.mark.parametrize("rate,P", GPU_CASES)
def test_wfmrx_squelch_inputs_are_fair_to_the_gates(port, rate, P):
    """Every input kind at every rate, P and (B, d) the GPU tests use: the oracle's chain on the model's gated stream with the kernels' reciprocal-multiply
    demodulator in place of its own passes the GPU tests' gates against the plain oracle chain."""
    x, lv = wsm.make_input(len(wm.KINDS)), wsm.levels(len(wm.KINDS))
    worst = (0.0, 0, 0.0)
    for B, d in BD:
        for k, kind in enumerate(wm.KINDS):
            g, _, fl = wsm.gated(x[k], B, d, lv[k])
            want_s16, want_af = wm.expected(port, g, rate, P)
            assert want_af.size == wm.plan(rate, P, 0, wm.W, wm.fresh_where(P), 0, g.size)[0] > 1000
            if not fl.any():
                assert not want_af.any()
                continue
            got_s16, got_af = wm.tail(port, wm.demod_rcp_model(g), rate, P)
            fig = wm.gate_figures(got_s16, got_af, want_s16, want_af)
            worst = tuple(max(a, b) for a, b in zip(worst, fig))
            wm.assert_gates(got_s16, got_af, want_s16, want_af, what="model %s @ %g / %d, B %d d %d" % (kind, rate, P, B, d))
    print("worst: relrms %.3g, %d LSB, %.4f %% differing" % (worst[0], worst[1], 100 * worst[2]))


@pytest.mark.parametrize("rate,P", GPU_CASES)
def test_wfmrx_squelch_compiled_reference_passes_the_gates(port, ref, rate, P):
    x, lv = wsm.make_input(len(wm.KINDS)), wsm.levels(len(wm.KINDS))
    for B, d in BD:
        for k, kind in enumerate(wm.KINDS):
            g, _, fl = wsm.gated(x[k], B, d, lv[k])
            if not fl.any():
                continue
            want_s16, want_af = wm.expected(port, g, rate, P)
            dem, _ = ref.fmdemod_quadri_cf(g)
            got_s16, got_af = wm.tail(ref, dem, rate, P)
            wm.assert_gates(got_s16, got_af, want_s16, want_af, what="reference %s @ %g / %d, B %d d %d" % (kind, rate, P, B, d))
