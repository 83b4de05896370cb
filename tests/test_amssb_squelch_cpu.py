"""CPU checks of the gated AM / SSB receive bank (csdr_amd_amssb_enable_squelch): the zero-run function against plain iteration of agc_ff's zero-sample map bit
for bit, that it does take its shortcut, agc_call_step on zero samples against the map, the decidability of the GPU tests' inputs, and the interfaces."""
import ctypes as C
import inspect
import numpy as np
import pytest

import amssb_model as mm
import amssb_squelch_model as qm

f32, c64 = np.float32, np.complex64

ALPHAS = (0.999, 0.99, 0.9, 0.5, 0.0129, 0.0013)
MAX_GAINS = (3.0, 100.0, 65536.0)
STARTS = (0.0, -0.0, 0.003, 1.0, 65536.0, 1e6, 3e38, -1.0, np.inf, np.nan)
NS = (0, 1, 2, 63, 1023, 20000, 10 ** 6)


def _params(csdr_amd, mode, B, alpha, max_gain):
    agc = list(mm.AGC_DEFAULT); agc[4] = max_gain; agc[6] = alpha
    return csdr_amd.amssb_params(mode, B, tuple(agc))


@pytest.fixture(scope="module")
def plain():
    """z applied one by one, 10^6 times, for the whole grid at once (numpy float32 arrays: the same operations as qm.z, element by element), read at every n of
    NS -> {n: gains [alpha, max_gain, start]}"""
    A, M, G = np.meshgrid(np.array(ALPHAS, f32), np.array(MAX_GAINS, f32), np.array(STARTS, f32), indexing="ij")
    zero = np.zeros_like(G)
    out, g = {}, G.copy()
    with np.errstate(all="ignore"):
        for k in range(max(NS) + 1):
            if k in NS:
                out[k] = g.copy()
            g2 = np.where(g > M, M, g)
            g2 = np.where(g2 < 0, zero, g2)
            g = (g2 + g) - A * g
    return out


def test_grid_iteration_is_qm_z(plain):
    """the array form of the plain iteration against the scalar qm.z, where that is affordable"""
    for ia, im, ig in ((0, 2, 3), (1, 2, 5), (3, 0, 2), (5, 1, 7), (0, 2, 1), (2, 1, 8), (4, 0, 9)):
        for n in (0, 1, 2, 63, 1023):
            mm.assert_bits(plain[n][ia, im, ig:ig + 1], np.array([qm.iterate(ALPHAS[ia], MAX_GAINS[im], STARTS[ig], n)], f32), "n %d" % n)


def test_zero_run_against_plain_iteration(plain):
    """the hook at every (alpha, max_gain, start, n) against z applied n times, by bits (a NaN equals a NaN)"""
    import csdr_amd
    for ia, alpha in enumerate(ALPHAS):
        for im, max_gain in enumerate(MAX_GAINS):
            P = _params(csdr_amd, "ssb", 64, alpha, max_gain)
            for ig, g0 in enumerate(STARTS):
                for n in NS:
                    got, it = csdr_amd.amssb_zero_run(P, g0, n)
                    assert 0 <= it <= n
                    mm.assert_bits(np.array([got], f32), plain[n][ia, im, ig:ig + 1], "alpha %g max_gain %g start %r n %d" % (alpha, max_gain, g0, n))


def test_zero_run_takes_the_shortcut():
    """CLI defaults, start 1e6, n = 10^6: fewer than n / 100 steps are taken one by one (the cycle of period 2 is entered after 3)"""
    import csdr_amd
    P = csdr_amd.amssb_params("am", 1024)
    n = 10 ** 6
    got, it = csdr_amd.amssb_zero_run(P, 1e6, n)
    print("steps iterated: %d of %d" % (it, n))
    assert it < n / 100
    assert got in (f32(65601.59375), f32(65601.6015625))


@pytest.mark.parametrize("mode", ["am", "ssb"])
@pytest.mark.parametrize("agc", ["default", "alt"])
def test_call_step_on_zero_samples_is_z(mode, agc):
    """csdr_amd_debug_amssb_walk on a block of +0 and of -0 samples: the gain behind it is z iterated B - 1 times on last_gain, and every s16 is 0, for finite,
    infinite and NaN last_gain"""
    import csdr_amd
    B = 256
    A = mm.AGC_SETS[agc]
    P = csdr_amd.amssb_params(mode, B, A)
    for zero in (0.0, -0.0):
        x = np.full(B, complex(zero, zero), c64)
        for g0 in (1.0, 0.003, 1e6, 3e38, -1.0, np.inf, np.nan):
            st = csdr_amd.AmSsbChan(0.0, g0)
            s16, pre = csdr_amd.amssb_debug_walk(P, x, st)
            assert not s16.any(), "s16 behind last_gain %r" % g0
            if mode == "am" or zero == 0.0 and not np.signbit(zero):
                assert not pre.any() and not np.signbit(pre).any()
            want = qm.iterate(A[6], A[4], g0, B - 1)
            mm.assert_bits(np.array([st.last_gain], f32), np.array([want], f32), "gain behind a zero block from %r" % g0)
            got, _ = csdr_amd.amssb_zero_run(P, g0, B - 1)
            mm.assert_bits(np.array([got], f32), np.array([want], f32), "zero_run from %r" % g0)


@pytest.mark.parametrize("mode", ["am", "ssb"])
def test_gpu_inputs_are_decidable(mode):
    """no (channel, block) of the GPU tests' inputs is within the float32 power's reach of a level those tests use: they may demand exact flags"""
    for n_ch, B, d in qm.GPU_SHAPES:
        x = qm.make_input(mode, n_ch, qm.NB, B)
        for ch in range(n_ch):
            for level in qm.GPU_LEVELS:
                assert qm.undecidable_blocks(x[ch], B, d, level) == [], (n_ch, B, d, ch, level)


def test_inputs_reach_the_three_ways():
    """the input maker: at LEVEL an AM channel closes with last_dc != 0 (a ramp block) and stays closed behind it (a zero block), and reopens"""
    B = 64
    x = qm.make_input("am", 5, qm.NB, B)
    for ch in (0, 3, 4):
        _, _, fl = qm.gated(x[ch], B, 1, qm.LEVEL)
        means = np.abs(x[ch]).reshape(-1, B).mean(axis=1)
        ways = qm.classify("am", fl, means)
        assert {"open", "ramp", "zero"} <= set(ways), ways
        k = ways.index("zero")
        assert "open" in ways[k:], ways
    assert set(qm.classify("ssb", [1, 0, 0, 1], None)) == {"open", "zero"}


def test_symbols_and_signatures():
    import csdr_amd
    L = csdr_amd.lib()
    for name in ("enable_squelch", "process_squelched", "set_squelch_level", "get_squelch_level", "squelch_block_index"):
        assert hasattr(L, "csdr_amd_amssb_" + name), name
    assert hasattr(L, "csdr_amd_debug_amssb_zero_run")
    init = inspect.signature(csdr_amd.AmSsb.__init__).parameters
    assert init["squelch"].default is False and init["use_every_nth"].default == 1 and init["levels"].default is None
    for name in ("process_squelched", "process_squelched_dev", "set_squelch_level", "get_squelch_level", "squelch_block_index"):
        assert callable(getattr(csdr_amd.AmSsb, name)), name
    assert list(inspect.signature(csdr_amd.AmSsb.process_squelched_dev).parameters)[1:] == [
        "d_in", "in_pitch", "n_in", "d_s16", "d_pre", "out_pitch", "d_power", "power_pitch", "d_flags"]
    assert list(inspect.signature(csdr_amd.amssb_zero_run).parameters) == ["params", "gain", "n"]
    # the host-side refusals that need no device
    assert L.csdr_amd_amssb_enable_squelch(None, 1, None) == -3
    assert L.csdr_amd_amssb_set_squelch_level(None, 0, C.c_float(1.0)) == -3
    assert L.csdr_amd_amssb_squelch_block_index(None) == -3
