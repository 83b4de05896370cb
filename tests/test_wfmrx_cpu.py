"""The WFM receive bank without a GPU: csdr_amd_wfmrx_plan (the framing rule, a host function) against its restatement and against check values measured with
the oracle; the fairness of the oracle gates for the inputs the GPU tests use; and the claim that the object writes what the four reference commands write."""
import os
import subprocess

import numpy as np
import pytest

import wfmrx_model as wm

f32 = np.float32
RATES = (5, 2.5, 5.2083335, 3.3)
# (rate, P) of the GPU tests, the rows of the stream they use (channels = kinds) and its length
GPU_CASES = [(5, 12, 7300), (2.5, 12, 6200), (5.2083335, 12, 6200), (3.3, 12, 6200), (5, 4, 6200)]


def test_wfmrx_plan_matches_restatement():
    import csdr_amd
    for rate in RATES:
        for P in (4, 12):
            for taps in (0, 133):
                for W in (1024, 256):
                    wheres = {wm.fresh_where(P)}
                    where = wm.fresh_where(P)
                    for _ in range(3):                                   # positions a stream really reaches: behind one, two, three windows
                        _, where, _ = wm.plan(rate, P, taps, W, where, 0, W)
                        wheres.add(where)
                    for where in sorted(wheres):
                        for held in range(W):
                            complete = W - held                          # the n_in that completes the next window
                            for n_in in {0, 1, complete - 1, complete, complete + 1, complete + 3 * W}:
                                got = csdr_amd.wfmrx_plan(rate, P, taps, W, where, held, n_in)
                                want = wm.plan(rate, P, taps, W, where, held, n_in)
                                assert got == want, (rate, P, taps, W, where, held, n_in, got, want)
                                assert 0 <= got[2] < max(W, held + 1) and (got[0] > 0) == (n_in >= complete and n_in > 0)


def test_wfmrx_plan_check_values():
    """measured with oracle.port().fractional_decimator_ff(d, rate, 12, None, bufsize=1024) on streams of every length: the first outputs appear at a total of
    1024 input samples, the cumulative count then steps at the totals below"""
    import csdr_amd
    table = {5: [(1024, 202), (2033, 404), (3043, 606), (4053, 808)], 2.5: [(1024, 403), (2031, 806), (3038, 1209), (4046, 1612)],
             5.2083335: [(1024, 194), (2034, 388), (3044, 581), (4050, 775)], 3.3: [(1024, 305), (2030, 610), (3036, 915), (4043, 1220)]}
    for rate, steps in table.items():
        before = 0
        for total, cumulative in steps:
            assert csdr_amd.wfmrx_plan(rate, 12, 0, 1024, 5.0, 0, total - 1)[0] == before, (rate, total)
            assert csdr_amd.wfmrx_plan(rate, 12, 0, 1024, 5.0, 0, total)[0] == cumulative, (rate, total)
            assert csdr_amd.wfmrx_plan(rate, 12, 0, 0, 5.0, 0, total)[0] == cumulative                       # window 0: 1024
            before = cumulative


def test_wfmrx_plan_agrees_with_the_oracle(port):
    rng = np.random.default_rng(2)
    d = rng.uniform(-0.2, 0.2, 5000).astype(f32)
    for rate in RATES:
        for P, taps in ((12, None), (4, None), (12, wm.prefilter_taps(rate))):
            nt = 0 if taps is None else taps.size
            for n in (1023, 1024, 3000, 5000):
                want = port.fractional_decimator_ff(d[:n], rate, P, taps, bufsize=1024).size
                assert wm.plan(rate, P, nt, 1024, wm.fresh_where(P), 0, n)[0] == want, (rate, P, nt, n)


@pytest.mark.parametrize("W", [1024, 256])
def test_wfmrx_plan_chain_of_calls_sums_to_one_call(W):
    import csdr_amd
    rng = np.random.default_rng(W)
    for rate in RATES:
        for P, taps in ((12, 0), (4, 0), (12, 133)):
            for _ in range(10):
                calls = rng.integers(0, 3 * W, size=rng.integers(1, 12))
                where, held, total = wm.fresh_where(P), 0, 0
                for k in calls:
                    n_out, where, held = csdr_amd.wfmrx_plan(rate, P, taps, W, where, held, int(k))
                    total += n_out
                one = csdr_amd.wfmrx_plan(rate, P, taps, W, wm.fresh_where(P), 0, int(calls.sum()))
                assert (total, where, held) == one, (rate, P, taps, list(calls))


def test_wfmrx_plan_rejects_bad_arguments():
    import csdr_amd
    good = dict(rate=5, num_poly_points=12, taps_length=0, window=1024, where=5.0, held=0, n_in=100)
    for bad in (dict(rate=1.0), dict(rate=0.5), dict(num_poly_points=11), dict(num_poly_points=0), dict(num_poly_points=66), dict(window=18),
                dict(window=150, taps_length=133), dict(held=-1), dict(n_in=-1), dict(where=-1.0), dict(taps_length=-1), dict(rate=30.0, num_poly_points=4)):
        with pytest.raises(csdr_amd.CsdrAmdError, match="wfmrx: "):
            csdr_amd.wfmrx_plan(**dict(good, **bad))
    got = csdr_amd.wfmrx_plan(5, 12, 0, 19, 5.0, 0, 19)                   # the shortest window the condition admits: it advances
    assert got == wm.plan(5, 12, 0, 19, 5.0, 0, 19) and got[0] == 1 and got[2] < 19


@pytest.mark.parametrize("rate,P,n", GPU_CASES)
def test_wfmrx_inputs_are_fair_to_the_gates(port, rate, P, n):
    """Every input kind at every rate and P the GPU tests use: the oracle's chain with the kernels' reciprocal-multiply demodulator in place of its own passes the
    GPU tests' gates against the plain oracle chain."""
    x = wm.make_input(len(wm.KINDS), n)
    for k, kind in enumerate(wm.KINDS):
        dem, _ = port.fmdemod_quadri_cf(x[k])
        assert np.abs(dem).max() <= 0.21
        if kind == "zeros":
            assert all(np.all(dem[a:b + 1] == 0) for a, b in wm.ZERO_RUNS)
        want_s16, want_af = wm.expected(port, x[k], rate, P)
        assert want_af.size == wm.plan(rate, P, 0, wm.W, wm.fresh_where(P), 0, n)[0] >= 5 * int(1000 / rate)
        if kind == "allzero":
            assert not want_af.any()
        got_s16, got_af = wm.tail(port, wm.demod_rcp_model(x[k]), rate, P)
        wm.assert_gates(got_s16, got_af, want_s16, want_af, what="model %s @ %g / %d" % (kind, rate, P))


@pytest.mark.parametrize("rate,P,n", GPU_CASES)
def test_wfmrx_compiled_reference_passes_the_gates(port, ref, rate, P, n):
    x = wm.make_input(len(wm.KINDS), n)
    for k, kind in enumerate(wm.KINDS):
        want_s16, want_af = wm.expected(port, x[k], rate, P)
        dem, _ = ref.fmdemod_quadri_cf(x[k])
        got_s16, got_af = wm.tail(ref, dem, rate, P)
        wm.assert_gates(got_s16, got_af, want_s16, want_af, what="reference %s @ %g / %d" % (kind, rate, P))


def test_wfmrx_prefilter_case_is_fair(port, ref):
    rate, n = 5.2083335, 6200
    taps = wm.prefilter_taps(rate)
    assert taps.size == 133
    x = wm.make_input(len(wm.KINDS), n)
    for k, kind in enumerate(wm.KINDS):
        want_s16, want_af = wm.expected(port, x[k], rate, 12, taps)
        got_s16, got_af = wm.tail(port, wm.demod_rcp_model(x[k]), rate, 12, taps)
        wm.assert_gates(got_s16, got_af, want_s16, want_af, what="model %s, prefilter" % kind)
        dem, _ = ref.fmdemod_quadri_cf(x[k])
        got_s16, got_af = wm.tail(ref, dem, rate, 12, taps)
        wm.assert_gates(got_s16, got_af, want_s16, want_af, what="reference %s, prefilter" % kind)


@pytest.mark.parametrize("rate", [5, 5.2083335, 2.5])
def test_wfmrx_model_is_what_the_reference_commands_write(port, rate):
    """`csdr fmdemod_quadri_cf | csdr fractional_decimator_ff <rate> | csdr deemphasis_wfm_ff 48000 50e-6 | csdr convert_f_s16` of the compiled reference on a
    20 000-sample stream: the model's samples are a prefix of what it writes (it goes on to re-emit stale blocks at EOF), within the gates."""
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "csdr")
    if not os.path.exists(cli):
        pytest.skip("oracle/_ref/csdr not built")
    x = wm.channel("fm", 77, 20000)
    data = x.tobytes()
    for cmd in (["fmdemod_quadri_cf"], ["fractional_decimator_ff", repr(rate)], ["deemphasis_wfm_ff", "48000", "50e-6"], ["convert_f_s16"]):
        p = subprocess.run(["timeout", "-k", "5", "60", cli] + cmd, input=data, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=90)
        assert p.returncode == 0, cmd
        data = p.stdout
    got = np.frombuffer(data[:len(data) // 2 * 2], np.int16)
    want, _ = wm.expected(port, x, rate)
    assert want.size == wm.plan(rate, 12, 0, 1024, 5.0, 0, 20000)[0] > 3000
    print("rate %g: the reference wrote %d samples, the model %d" % (rate, got.size, want.size))
    assert got.size >= want.size
    d = np.abs(got[:want.size].astype(np.int32) - want.astype(np.int32))
    print("largest difference %d, differing %.4f %%" % (d.max(), 100 * (d > 0).mean()))
    assert d.max() <= 1 and (d > 0).mean() < wm.S16_FRACTION
