"""The WFM chain's de-emphasis rule (csdr_amd_wfm_deemph_exact, host arithmetic) against its restatement in Python, and the fairness of
tests/test_wfm_deemph_gpu.py: on that file's own inputs a CPU model of the kernels' fixed warm-up breaks +-1 LSB wherever the rule sends an object to the exact
route with b^W >= 1.2e-4, and stays within +-1 LSB wherever it leaves the kernels alone.  No GPU."""
import numpy as np
import pytest
import wfm_deemph_model as m


@pytest.fixture(scope="module")
def L():
    import csdr_amd
    return csdr_amd.lib()


# the issue's table: (tau, audio_rate) -> b^48, b^64 to two digits
TABLE = {(50e-6, 48000): (5.5e-8, 2.1e-10), (75e-6, 48000): (7.8e-6, 1.5e-7), (50e-6, 96000): (1.1e-4, 5.5e-6),
         (75e-6, 96000): (1.9e-3, 2.4e-4), (75e-6, 192000): (4.0e-2, 1.4e-2), (1e-3, 48000): (0.37, 0.27)}


def test_left_over_table():
    """the Python restatement reproduces the table the rule was designed from"""
    for (tau, ar), want in TABLE.items():
        for W, w in zip((48, 64), want):
            got = m.left_over(tau, ar, W)
            assert abs(got - w) <= 0.05 * w, (tau, ar, W, got, w)


def test_rule_against_restatement(L):
    """every pair of the table and of the GPU cases at W = 48 and 64, then tau 1e-7 .. 1e-1 x rates 8000 .. 384000 x W 1 .. 4096; the values the design names"""
    assert L.csdr_amd_wfm_deemph_exact(50e-6, 48000, 48) == 0 and L.csdr_amd_wfm_deemph_exact(50e-6, 48000, 64) == 0
    assert L.csdr_amd_wfm_deemph_exact(75e-6, 48000, 64) == 0 and L.csdr_amd_wfm_deemph_exact(75e-6, 48000, 48) == 1
    for tau, ar in list(TABLE) + m.TR:
        for W in (48, 64):
            assert L.csdr_amd_wfm_deemph_exact(tau, ar, W) == m.rule(tau, ar, W), (tau, ar, W)
    taus = np.concatenate([np.logspace(-7, -1, 97), [50e-6, 75e-6, 1e-3]])
    rates = [8000, 11025, 22050, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 384000]
    n_exact = 0
    for tau in taus:
        for ar in rates:
            for W in (1, 16, 48, 64, 100, 4096):
                got = L.csdr_amd_wfm_deemph_exact(float(tau), ar, W)
                # a power within a few ulp of the bound may fall on either side in another libm: none of these does
                assert abs(m.left_over(float(np.float32(tau)), ar, W) / m.BOUND - 1) > 1e-9
                assert got == m.rule(float(np.float32(tau)), ar, W), (tau, ar, W)
                n_exact += got
    assert 0 < n_exact < taus.size * len(rates) * 6


def test_rule_monotone(L):
    """a longer tau, a higher rate or a shorter warm-up never turns 1 into 0"""
    taus = np.logspace(-7, -1, 241)
    for ar in (8000, 44100, 48000, 96000, 192000, 384000):
        for W in (16, 48, 64):
            r = [L.csdr_amd_wfm_deemph_exact(float(t), ar, W) for t in taus]
            assert all(a <= b for a, b in zip(r, r[1:])), (ar, W)
    for tau in (1e-6, 50e-6, 75e-6, 1e-3):
        for W in (16, 48, 64):
            r = [L.csdr_amd_wfm_deemph_exact(tau, ar, W) for ar in range(8000, 384001, 2000)]
            assert all(a <= b for a, b in zip(r, r[1:])), (tau, W)
        for ar in (48000, 192000):
            r = [L.csdr_amd_wfm_deemph_exact(tau, ar, W) for W in range(1, 400)]
            assert all(a >= b for a, b in zip(r, r[1:])), (tau, ar)


def test_warm_samples_are_the_codes(L):
    """the W of every path as the library reports it from its constants: two steps of 4 SEQ_TPG = 24 samples in the chain kernel, WARM in k_wfm_back, the
    smaller of the chain kernel's and RES_WARM for the ring.  The model's segment geometry (wfm_deemph_model) was read from the same code at these values."""
    assert L.csdr_amd_wfm_deemph_warm_samples(0) == m.W_CHAIN == 48
    assert L.csdr_amd_wfm_deemph_warm_samples(1) == m.W_FALLBACK == 48
    assert L.csdr_amd_wfm_deemph_warm_samples(2) == m.W_RING == 48
    assert L.csdr_amd_wfm_deemph_warm_samples(3) < 0


def test_model_is_the_recurrence_without_seams(port):
    """one segment as long as the stream = the oracle's de-emphasis, bit for bit: the model differs from it by its seams alone"""
    a = m.pre_audio(port, "shared")[0]
    for tau, ar in ((50e-6, 48000), (1e-3, 48000)):
        want = m.oracle_audio(port, "shared", tau, ar)[0][1]
        assert np.array_equal(m.fixed_warmup(a, tau, ar, a.size, 48).view(np.uint32), want.view(np.uint32))


CASES = [("shared", m.SEG_SHARED, m.W_CHAIN, m.TR), ("ps", m.SEG_PS, m.W_CHAIN, m.TR), ("shared", m.SEG_FALLBACK, m.W_FALLBACK, m.TR_FALLBACK)]


@pytest.mark.parametrize("which,seg,warm,pairs", CASES, ids=["shared", "per-stream", "fallback"])
def test_gpu_cases_are_fair(port, which, seg, warm, pairs):
    """On the GPU tests' own inputs and segment geometry: a case on the exact route with b^W >= 1.2e-4 would have failed the +-1 LSB gate under the fixed warm-up
    (so the GPU test notices a library that does not take the route), a case the rule leaves to the kernels stays within it."""
    seen_exact = seen_fast = 0
    for tau, ar in pairs:
        worst = m.model_worst_lsb(port, which, tau, ar, seg, warm)
        left = m.left_over(tau, ar, warm)
        print("%s tau %g rate %d: b^%d = %.2e, rule %d, modelled fixed warm-up %d LSB" % (which, tau, ar, warm, left, m.rule(tau, ar, warm), worst))
        if m.rule(tau, ar, warm):
            if left >= 1.2e-4:
                assert worst > 1, (tau, ar, worst)
                seen_exact += 1
        else:
            assert worst <= 1, (tau, ar, worst)
            seen_fast += 1
    assert seen_exact >= 2 and seen_fast >= 1
