"""Pins the models of tests/audio_model.py to the oracle (and, where it is built, to the compiled reference) at the shapes test_audio_blocks_gpu.py runs,
establishes the gates -- kappa = 4 x the float32 oracle's worst ratio to the structural bound of the float64 run -- and shows that planted defects fail them.
`python tests/test_audio_blocks_cpu.py` writes the measured ratios and the constants to profiles/audio_blocks_gates.md (the GPU section of that file is kept
as it is); the suite itself writes nothing."""
import os
import sys
import warnings
import numpy as np
import pytest

import audio_model as am
from audio_model import f32, c64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATES_MD = os.path.join(ROOT, "profiles", "audio_blocks_gates.md")
GPU_MARK = "## On the GPU"
MEASURED = {}                          # block -> (worst oracle ratio, note): what the measuring tests found, for write_record()


def _denormals_live_now():
    """False once the compiled reference (built with -ffast-math) has been loaded into this process: the pins that need live denormals cannot run then, and
    say so in the warnings summary.  Flush-to-zero from any other cause is an error."""
    if bool(f32(1e-38) * f32(0.5) != 0):
        return True
    import oracle
    assert am.DENORMALS_LIVE and oracle._ref is not None, "the process flushes denormals, and not because the compiled reference was loaded"
    warnings.warn("the compiled reference has switched this process to flush-to-zero: the denormal pins of this test did not run (they run when this file "
                  "runs before any test that uses `ref`)")
    return False


def _kappa_holds(block, worst):
    """the constant carries the factor 4 over the measured worst ratio (and is not more than twice that: a bound that slack would hide a changed model)"""
    k = am.KAPPA[block]
    print("KAPPA", block, "worst %.4f" % worst, "kappa", k)
    assert 4 * worst <= k <= 8 * worst, "%s: worst float32 ratio %.3f, kappa %.2f" % (block, worst, k)


# ------------------------------------------------------------------ the helpers and the dispatch rules
def test_bit_compare_tells_signed_zeros_and_nan_positions():
    a = np.array([0.0, -0.0, np.nan, 1.0, np.nan], f32)
    assert am.bit_mismatches(a, a.copy()).size == 0
    assert list(am.bit_mismatches(a, np.array([-0.0, -0.0, np.nan, 1.0, 2.0], f32))) == [0, 4]
    other_nan = np.array([0.0, -0.0, -np.nan, 1.0, np.nan], f32)
    assert am.bit_mismatches(a, other_nan).size == 0
    with pytest.raises(AssertionError):
        am.assert_bits(a, np.array([0.0, -0.0, np.nan, np.nextafter(f32(1), f32(2)), np.nan], f32), "x")


def test_dispatch_rules():
    for tau, fs, M in am.DEEMPH_TAUS:
        assert am.deemph_run_in(tau, fs, 1, 2048) == M and am.deemph_run_in(tau, fs, 31, 2048) == M
        assert am.deemph_run_in(tau, fs, 32, 4096) == 0 and am.deemph_run_in(tau, fs, 1, 2047) == 0 and am.deemph_run_in(tau, fs, 1, 5000, in_place=True) == 0
    for s, n, _, want in am.AGC_SHAPES:
        assert am.agc_path(s, n) == want
    for rate, P, T, buf, cls in am.FRACDEC_CASES:
        where0 = float((P // 2) - 1)
        assert am.fracdec_exact(where0, rate, am.FRACDEC_CALLS[0], P, T, buf) == (cls == "exact"), (rate, P)
    assert not am.fracdec_exact(5.0, 5.0, 2 ** 24, 12, 0)             # positions past 2^24 are not exact any more
    m = am.FracdecPath(5.0, 12, 0)
    assert [m.path(5.0, 100), m.path(5.0, 100), m.path(5.0, 101), m.path(2.0, 101)] == ["fracdec:exact", "fracdec:cached", "fracdec:exact", "fracdec:exact"]


# ------------------------------------------------------------------ deemphasis_wfm_ff
def test_deemph_model_is_the_oracle(port):
    rng = np.random.default_rng(1)
    for tau, fs, _ in am.DEEMPH_TAUS:
        x = rng.uniform(-1, 1, 3000).astype(f32)
        for last in am.DEEMPH_STATES:
            y, _ = am.deemph_serial(x, am.deemph_alpha(tau, fs), f32(last))
            w, wl = port.deemphasis_wfm_ff(x, tau, fs, float(f32(last)))
            am.assert_bits(y, w, "deemph_serial tau %g" % tau); am.assert_bits(y[-1:], [wl], "state")
    if _denormals_live_now():
        for tau, fs, x, last, want in am.DEEMPH_DENORMAL:
            for r in range(x.shape[0]):
                am.assert_bits(want[r], port.deemphasis_wfm_ff(x[r], tau, fs, float(last[r]))[0], "denormal inputs")


def test_deemph_repair_inputs_reach_the_repair():
    """ordinary input: every chunk arrives with the serial state (the repair has nothing to do); the repair inputs: at least one does not"""
    counts = {}
    for tau, fs, M in am.DEEMPH_TAUS:
        if not M:
            continue
        alpha = am.deemph_alpha(tau, fs)
        x = np.random.default_rng(M).uniform(-1, 1, 6000).astype(f32)
        assert am.deemph_spec_mismatches(x, alpha, M, 0.37) == 0 and am.deemph_spec_mismatches(x, alpha, M, np.nan) == 0
        if M == 4:
            continue
        for kind in ("1e30", "nan", "inf"):
            rng = np.random.default_rng(M)
            for r, last in enumerate((0.0, 0.37)):
                c = am.deemph_spec_mismatches(am.deemph_repair_input(rng, 6000, kind), alpha, M, last)
                assert c > 0, (kind, M, r)
                counts[(kind, M, r)] = c
    MEASURED["deemph_repair"] = counts


# ------------------------------------------------------------------ dcblock_ff
def _dc_ratios(port, x, a, y64, B, st64, state=(0.0, 0.0), emulate_rows=4):
    wo = we = 0.0
    for r in range(x.shape[0]):
        y, st = port.dcblock_ff(x[r], a, state)
        wo = max(wo, am.gate_ratio(y, y64[r], B[r]), abs(st[1] - st64[1][r]) / B[r, -1])
        assert st[0] == x[r, -1]
        if r < emulate_rows:
            y, st = am.dcblock_emulate(x[r], a, state)
            we = max(we, am.gate_ratio(y, y64[r], B[r]), abs(float(st[1]) - st64[1][r]) / B[r, -1])
            assert st[0] == x[r, -1]
    return wo, we


def test_dcblock_gate_and_planted_faults(port):
    wo = we = 0.0
    for ci, (s, n, a) in enumerate(am.DC_CASES):
        x, y64, B, st64 = am.dc_case(ci)
        o, e = _dc_ratios(port, x, a, y64, B, st64)
        wo, we = max(wo, o), max(we, e)
    MEASURED["dcblock_ff"] = (wo, "float32 oracle; the three-pass emulation: %.3f" % we)
    _kappa_holds("dcblock_ff", max(wo, we))
    k = am.KAPPA["dcblock_ff"]
    margins = {}
    for a in (0.5, 0.95):
        for n in (33, 8193, 20011):
            x = am.dc_input(2, n, n)
            y64, B, st64, _ = am.dcblock_f64(x, a)
            for fault in ("prev0", "ragged", "last"):
                worst = np.inf
                for r in range(2):
                    y, st = am.dcblock_emulate(x[r], a, (0.0, 0.0), fault)
                    g = max(am.gate_ratio(y, y64[r], B[r], k), abs(float(st[1]) - st64[1][r]) / (k * B[r, -1]))
                    worst = min(worst, g)
                assert worst >= 4.0, "planted fault %s at a = %g, n = %d is only %.2f x the gate" % (fault, a, n, worst)
                margins[fault] = min(margins.get(fault, np.inf), worst)
    MEASURED["dcblock_faults"] = margins


def test_dcblock_three_calls_carry_the_bound(port):
    x = am.dc_input(3, 4034, 99)
    st0 = np.array([[0.5, -0.25], [100.0, 3.0], [0.0, 0.0]], f32)
    y64, B, st64, _ = am.dcblock_f64(x, 0.95, (st0[:, 0], st0[:, 1]))
    k = am.KAPPA["dcblock_ff"]
    for r in range(3):
        at, st, ys = 0, tuple(float(v) for v in st0[r]), []
        for n in (33, 1, 4000):
            y, st = am.dcblock_emulate(x[r, at:at + n], 0.95, st); ys.append(y); at += n
        assert am.gate_ratio(np.concatenate(ys), y64[r], B[r], k) <= 0.25
        yo, _ = port.dcblock_ff(x[r], 0.95, tuple(float(v) for v in st0[r]))
        assert am.gate_ratio(yo, y64[r], B[r], k) <= 0.25


# ------------------------------------------------------------------ fastdcblock_ff, fmdemod_atan_cf, amdemod_cf, logpower_cf
def test_fastdcblock_gate(port):
    worst = 0.0
    for s, block, calls in am.FASTDC_CASES:
        nb = sum(calls)
        x = am.dc_input(s, nb * block, 300 + block)
        last = np.array([0.1 * (r % 5) for r in range(s)], f32)
        y64, S, l64 = am.fastdcblock_f64(x, block, last)
        for r in range(s):
            y, lo = port.fastdcblock_ff(x[r], block, float(last[r]))
            worst = max(worst, am.gate_ratio(y, y64[r], S[r]), abs(lo - l64[r]) / S[r, -1])
    MEASURED["fastdcblock_ff"] = (worst, "float32 oracle (sequential block sum)")
    _kappa_holds("fastdcblock_ff", worst)


def test_fmdemod_atan_gate(port):
    worst = 0.0
    for n, _ in am.ATAN_CASES:
        x, last = am.atan_case(n)
        for r in range(3):
            w, S, ph = am.fmdemod_atan_f64(x[r], last[r])
            y, lo = port.fmdemod_atan_cf(x[r], float(last[r]))
            worst = max(worst, am.gate_ratio(y, w, S), abs(lo - ph) / (am.U * np.pi))
    x, last = am.atan_case(700)
    w, _, _ = am.fmdemod_atan_f64(x[0], last[0])
    assert w[11] == pytest.approx(1.0, abs=1e-7) and w[12] == pytest.approx(-1.0, abs=1e-7)          # steps of exactly pi are not unwrapped
    w, _, _ = am.fmdemod_atan_f64(x[1], last[1])
    assert w[11] == pytest.approx(1 - 1e-3 / np.pi, abs=1e-6) and w[12] == pytest.approx(-1 + 1e-3 / np.pi, abs=1e-6)    # just past it: unwrapped
    MEASURED["fmdemod_atan_cf"] = (worst, "float32 oracle")
    _kappa_holds("fmdemod_atan_cf", worst)


def test_amdemod_and_logpower_gates(port):
    x = am.flat_c_input()
    w, S = am.amdemod_f64(x)
    ga = am.gate_ratio(port.amdemod_cf(x), w, S)
    w, S = am.logpower_f64(x, -70.0)
    gl = am.gate_ratio(port.logpower_cf(x, -70.0), w, S)
    MEASURED["amdemod_cf"] = (ga, "float32 oracle"); MEASURED["logpower_cf"] = (gl, "float32 oracle")
    _kappa_holds("amdemod_cf", ga); _kappa_holds("logpower_cf", gl)


# ------------------------------------------------------------------ fmdemod_quadri_cf
def test_fmdemod_quadri_reference_and_ulp_bound(port):
    worst = 0.0
    for s, n, _ in am.FM_CASES:
        x, last, zeros = am.fm_case(s, n)
        for r in range(min(s, 4)):
            ref = am.fmdemod_quadri_ref(x[r], last[r])
            y, _ = port.fmdemod_quadri_cf(x[r], (float(last[r].real), float(last[r].imag)))
            am.assert_bits(ref, y, "fmdemod_quadri_ref %dx%d" % (s, n))
            gate = am.fmdemod_quadri_ulp_bound(x[r], last[r])
            d, n_abs = am.fmdemod_quadri_check(y, x[r], last[r], gate)
            assert d == 0 and n_abs == len(set(zeros) | {k + 1 for k in zeros if k + 1 < n})
            worst = max(worst, gate)
    gate = am.fmdemod_quadri_ulp_bound(am.FM_SWEEP_X, am.FM_SWEEP_LAST)
    if _denormals_live_now():
        y, _ = port.fmdemod_quadri_cf(am.FM_SWEEP_X, (float(am.FM_SWEEP_LAST.real), float(am.FM_SWEEP_LAST.imag)))
        am.assert_bits(am.FM_SWEEP_REF, y, "magnitude sweep")
    # a result that the reciprocal's flush turned into 0 (the defect the device had), one NaN, one value 8 ulp off: each is caught
    x, last, _ = am.fm_case(1, 255)
    ref = am.fmdemod_quadri_ref(x[0], last[0])
    assert all(abs(ref[k]) >= np.finfo(f32).tiny for k in (40, 50, 60))
    for k, v in ((40, 0.0), (50, np.nan), (60, ref[60] + 8 * np.spacing(ref[60]))):
        bad = ref.copy(); bad[k] = v
        with pytest.raises(AssertionError):
            d, _ = am.fmdemod_quadri_check(bad, x[0], last[0], gate)
            assert d <= gate
    MEASURED["fmdemod_quadri_cf"] = (max(worst, gate), "ulps: the emulated fast path's worst distance + 1, over the |x| ~ 0.7 cases and the magnitude sweep")


# ------------------------------------------------------------------ agc_ff and fastagc_ff: the planted defects differ in bits
def test_agc_counters_that_do_not_restart_differ(port):
    hits = 0
    for si, (s, n, block, _) in enumerate(am.AGC_SHAPES):
        for pi, p in enumerate(am.AGC_PARAMS):
            x, g0, _ = am.agc_case(si, pi)
            for r in range(min(s, 2)):
                good, _ = am.port_agc(port, x[r], block, p, g0[r])
                bad, _ = am.port_agc(port, x[r], block, p, g0[r], restart=False)
                hits += am.bit_mismatches(good, bad).size > 0 or not np.any(x[r])
    assert hits == sum(min(s, 2) for s, *_ in am.AGC_SHAPES) * len(am.AGC_PARAMS)


def test_fastagc_model_is_the_oracle_and_next_blocks_gain_differs(port):
    for s, block, calls in am.FASTAGC_CASES:
        nb = sum(calls)
        x = am.fastagc_input(s, block, nb, block * 7 + nb)
        for zero in (True, False):
            st = am.fastagc_state(s, block, zero, block)
            w, ws = am.port_fastagc(port, x[0], block, 1.0, st[0])
            y, ys = am.fastagc_emulate(x[0], block, 1.0, st[0])
            am.assert_bits(y, w, "fastagc_emulate block %d" % block); am.assert_bits(ys[:2 * block + 3], ws[:2 * block + 3], "state")
            # split into the calls: the state carries everything
            at, stc, parts = 0, st[0], []
            for k in calls:
                yk, stc = am.port_fastagc(port, x[0, at * block:(at + k) * block], block, 1.0, stc); parts.append(yk); at += k
            am.assert_bits(np.concatenate(parts), w, "calls %r" % (calls,))
            if nb >= 3:
                bad, _ = am.fastagc_emulate(x[0], block, 1.0, st[0], gain_of_next=True)
                assert am.bit_mismatches(bad, w).size > block // 2


def test_fracdec_oracle_driver_matches_the_one_call_form(port):
    x = np.random.default_rng(8).uniform(-1, 1, 9000).astype(f32)
    for rate, P, T, buf, _ in am.FRACDEC_CASES:
        taps = am.asym_taps(T, 900 + P) if T else None
        y, _ = am.PortFracdec(port, rate, P, taps, buf).call(x)
        am.assert_bits(y, port.fractional_decimator_ff(x, rate, P, taps, buf or None), "rate %g" % rate)


# ------------------------------------------------------------------ the float64 forms behind the compiled reference's gates
def test_fastagc_and_fracdec_float64_gates(port):
    worst = 0.0
    for s, block, calls in am.FASTAGC_CASES:
        nb = sum(calls)
        x = am.fastagc_input(s, block, nb, block * 7 + nb)
        for zero in (True, False):
            st = am.fastagc_state(s, block, zero, block)
            for r in range(min(s, 3)):
                y64, S = am.fastagc_f64(x[r], block, 1.0, st[r])
                worst = max(worst, am.gate_ratio(am.port_fastagc(port, x[r], block, 1.0, st[r])[0], y64, S))
    MEASURED["fastagc_ff"] = (worst, "float32 oracle")
    _kappa_holds("fastagc_ff", worst)
    worst = 0.0
    for rate, P, T, buf, _ in am.FRACDEC_CASES:
        taps, x = _fracdec_input(rate, P, T)
        for n in am.FRACDEC_CALLS:
            o = am.PortFracdec(port, rate, P, taps, buf)
            w0 = o.where
            y, proc = o.call(x[0, :n])
            y64, S, w_after, p64 = am.fracdec_f64(x[0, :n], rate, P, taps, w0, buf)
            assert y.size == y64.size and proc == p64 and w_after == o.where, (rate, P, n)
            worst = max(worst, am.gate_ratio(y, y64, S))
    MEASURED["fractional_decimator_ff"] = (worst, "float32 oracle")
    _kappa_holds("fractional_decimator_ff", worst)


def _fracdec_input(rate, P, T):
    """the GPU file's taps and input of one FRACDEC_CASES entry"""
    taps = am.asym_taps(T, 900 + P) if T else None
    return taps, np.random.default_rng(int(rate * 1000) + P).uniform(-1, 1, (3, 3 * max(am.FRACDEC_CALLS) + 100)).astype(f32)


# ------------------------------------------------------------------ the compiled reference, where it is built (loading it switches the process to flush-to-zero)
def test_models_against_the_compiled_reference(ref, port):
    """Every case list of the GPU file against the unmodified reference.  The reference is built with -ffast-math, so:
      bits   deemphasis_wfm_ff, fmdemod_quadri_cf, gain_ff, and limit_ff except at NaN inputs (its min / max assume there are none and return the limit);
      gate   the blocks the GPU file gates (dcblock_ff, fastdcblock_ff, fmdemod_atan_cf, amdemod_cf, logpower_cf), to the same gate -- dcblock_ff with the bound
             of an evaluation that sums its three terms in any order, audio_model.dcblock_bound_any_order --; and fastagc_ff and
             fractional_decimator_ff, whose gain ramp and Lagrange / FIR sums -ffast-math reassociates: to the gates of their float64 forms, with the counts,
             input_processed and `where` exact;
      agc_ff cannot be held to bits (the gain filter line is reassociated) nor to a derived per-sample gate (the recursion's error multiplier 2 - alpha exceeds 1
             and the branches depend on the perturbed gain): it is held, at every shape and parameter set, to the suite's standing pin of this block to the
             reference (test_oracle_vs_ref.py: 5e-6 relative RMS per stream, 1e-5 on the carried gain)."""
    from oracle import relrms
    # ---- bits
    for tau, fs, _ in am.DEEMPH_TAUS:
        for s, n in am.DEEMPH_SHAPES:
            x = np.random.default_rng(s * 100003 + n).uniform(-1, 1, (s, n)).astype(f32)
            for r in range(s):
                last = float(f32(am.DEEMPH_STATES[r % 3]))
                (y, l), (w, wl) = ref.deemphasis_wfm_ff(x[r], tau, fs, last), port.deemphasis_wfm_ff(x[r], tau, fs, last)
                am.assert_bits(y, w, "deemphasis_wfm_ff %dx%d tau %g" % (s, n, tau)); am.assert_bits([l], [wl], "state")
    for s, n, _ in am.FM_CASES:
        x, last, _ = am.fm_case(s, n)
        for r in range(s):
            am.assert_bits(ref.fmdemod_quadri_cf(x[r], (float(last[r].real), float(last[r].imag)))[0], am.fmdemod_quadri_ref(x[r], last[r]), "fmdemod_quadri_cf %dx%d" % (s, n))
    x = am.flat_f_input()
    am.assert_bits(ref.gain_ff(x, 0.37), port.gain_ff(x, 0.37), "gain_ff")
    y, w = ref.limit_ff(x, 1.0), port.limit_ff(x, 1.0)
    nan = np.isnan(x)
    am.assert_bits(y[~nan], w[~nan], "limit_ff")
    assert nan.sum() == 2 and np.all(y[nan] == 1.0) and np.all(np.isnan(w[nan]))
    # ---- the GPU file's gates
    k = am.KAPPA["dcblock_ff"]
    for ci, (s, n, a) in enumerate(am.DC_CASES):
        x, y64, _, st64 = am.dc_case(ci)
        B = am.dcblock_bound_any_order(x, a, y64)                     # (the reference may sum the three terms in another order)
        for r in range(s):
            y, st = ref.dcblock_ff(x[r], a)
            assert am.gate_ratio(y, y64[r], B[r], k) <= 1.0 and abs(st[1] - st64[1][r]) <= k * B[r, -1] and st[0] == x[r, -1], (ci, r)
    k = am.KAPPA["fastdcblock_ff"]
    for s, block, calls in am.FASTDC_CASES:
        x = am.dc_input(s, sum(calls) * block, 300 + block)
        last = np.array([0.1 * (r % 5) for r in range(s)], f32)
        y64, S, l64 = am.fastdcblock_f64(x, block, last)
        for r in range(s):
            y, lo = ref.fastdcblock_ff(x[r], block, float(last[r]))
            assert am.gate_ratio(y, y64[r], S[r], k) <= 1.0 and abs(lo - l64[r]) <= k * S[r, -1], (block, r)
    k = am.KAPPA["fmdemod_atan_cf"]
    for n, _ in am.ATAN_CASES:
        x, last = am.atan_case(n)
        for r in range(3):
            w, S, ph = am.fmdemod_atan_f64(x[r], last[r])
            y, lo = ref.fmdemod_atan_cf(x[r], float(last[r]))
            assert am.gate_ratio(y, w, S, k) <= 1.0 and abs(lo - ph) <= k * am.U * np.pi, (n, r)
    x = am.flat_c_input()
    w, S = am.amdemod_f64(x)
    assert am.gate_ratio(ref.amdemod_cf(x), w, S, am.KAPPA["amdemod_cf"]) <= 1.0
    w, S = am.logpower_f64(x, -70.0)
    assert am.gate_ratio(ref.logpower_cf(x, -70.0), w, S, am.KAPPA["logpower_cf"]) <= 1.0
    # ---- reassociated by -ffast-math: the gates of the float64 forms
    k = am.KAPPA["fastagc_ff"]
    for s, block, calls in am.FASTAGC_CASES:                           # (the reference's CLI framing starts from the zero state)
        nb = sum(calls)
        x = am.fastagc_input(s, block, nb, block * 7 + nb)
        for r in range(s):
            y64, S = am.fastagc_f64(x[r], block, 1.0, np.zeros(2 * block + 4, f32))
            assert am.gate_ratio(ref.fastagc_ff(x[r], block, 1.0), y64, S, k) <= 1.0, (block, r)
    k = am.KAPPA["fractional_decimator_ff"]
    for rate, P, T, buf, _ in am.FRACDEC_CASES:                        # (a fresh object per call size: the harness of the reference keeps no state)
        taps, x = _fracdec_input(rate, P, T)
        for n in am.FRACDEC_CALLS:
            for r in range(3):
                y = ref.fractional_decimator_ff(x[r, :n], rate, P, taps, buf or None)
                y64, S, _, _ = am.fracdec_f64(x[r, :n], rate, P, taps, float(P // 2 - 1), buf)
                assert y.size == y64.size and am.gate_ratio(y, y64, S, k) <= 1.0, (rate, P, n, r)
    # ---- agc_ff
    for si, (s, n, block, _) in enumerate(am.AGC_SHAPES):
        for pi, p in enumerate(am.AGC_PARAMS):
            x, g0, _ = am.agc_case(si, pi)
            for r in range(s):
                y, g = ref.agc_ff(x[r], block=block, last_gain=float(g0[r]), **p)
                w, wg = am.port_agc(port, x[r], block, p, g0[r])
                assert relrms(w, y) <= 5e-6 and abs(wg - g) <= 1e-5 * max(1, abs(g)), (si, pi, r)


# ------------------------------------------------------------------ the record
CPU_BLOCKS = ("dcblock_ff", "fastdcblock_ff", "fmdemod_atan_cf", "amdemod_cf", "logpower_cf", "fastagc_ff", "fractional_decimator_ff")


def test_gates_record_names_the_constants():
    text = open(GATES_MD).read()
    for b in CPU_BLOCKS:
        row = [l for l in text.splitlines() if l.startswith("| `%s` |" % b)]
        assert row and "| %g |" % am.KAPPA[b] in row[0], "profiles/audio_blocks_gates.md is behind audio_model.KAPPA[%r]: run python tests/test_audio_blocks_cpu.py" % b


def write_record():
    """measure (the tests above, run here in the order they need) and write the CPU part of profiles/audio_blocks_gates.md"""
    sys.path.insert(0, ROOT)
    import oracle
    port = oracle.port()
    test_deemph_repair_inputs_reach_the_repair()
    for t in (test_dcblock_gate_and_planted_faults, test_fastdcblock_gate, test_fmdemod_atan_gate, test_amdemod_and_logpower_gates,
              test_fmdemod_quadri_reference_and_ulp_bound, test_fastagc_and_fracdec_float64_gates):
        t(port)
    lines = ["# Gates of the audio-rate block tests", "",
             "Written by `python tests/test_audio_blocks_cpu.py`.  gate_i = kappa * S_i, S_i the structural bound evaluated along the float64 run (tests/audio_model.py);",
             "kappa is at least 4 x the worst ratio of the float32 oracle (for dcblock_ff also of the three-pass emulation) to S_i over every shape the GPU file runs.",
             "Measured against float64, never against the kernels.", "",
             "| block | worst float32 ratio | kappa | measured on |", "|---|---|---|---|"]
    for b in CPU_BLOCKS:
        lines.append("| `%s` | %.2f | %g | %s |" % (b, MEASURED[b][0], am.KAPPA[b], MEASURED[b][1]))
    lines += ["", "`fmdemod_quadri_cf`: gate %.1f %s." % MEASURED["fmdemod_quadri_cf"], "",
              "`fastdcblock_ff`: S does not grow with the block length, while the error of the oracle's sequential float32 block sum does (of the order of block x u x",
              "mean|x|): the oracle sits at 11 x S and the gate at 47 x S, about 12 times what the kernel's tree mean needs (0.08 of the gate).  It follows the recipe",
              "above; a bound with the sum's own error term would track the kernel more closely.", "",
              "Against the compiled reference (test_models_against_the_compiled_reference, every case list of the GPU file): `deemphasis_wfm_ff`, `fmdemod_quadri_cf`,",
              "`gain_ff` and `limit_ff` (except at NaN inputs) meet it bit for bit.  The reference is built with -ffast-math, which reassociates sums: `dcblock_ff`",
              "(with the bound of a three-term sum taken in any order: |x_i| + |x_i-1| in place of |x_i - x_i-1|, which at DC 100 is 100 u against u),",
              "`fastdcblock_ff`, `fmdemod_atan_cf`, `amdemod_cf` and `logpower_cf` are held to the gates above; `fastagc_ff` and `fractional_decimator_ff` -- bit-held",
              "on the device against the oracle -- to the gates of their float64 forms (rows above; counts, input_processed and `where` exact); `agc_ff`, whose",
              "recursion allows no derived per-sample gate, to the suite's standing pin (5e-6 relative RMS per stream, 1e-5 on the carried gain).", "",
              "Planted `dcblock_ff` defects, smallest excess over the gate (a in {0.5, 0.95}, n in {33, 8193, 20011}, DC 0.25 and 100; at least 4 is required): "
              + ", ".join("%s %.3g x" % (f, m) for f, m in sorted(MEASURED["dcblock_faults"].items())) + ".", "",
              "`deemphasis_wfm_ff` repair inputs, chunks that arrive with a state other than the serial one (model; streams with carried state 0 / 0.37): "
              + ", ".join("%s M=%d: %d / %d" % (kind, M, MEASURED["deemph_repair"][(kind, M, 0)], MEASURED["deemph_repair"][(kind, M, 1)])
                          for kind in ("1e30", "nan", "inf") for M in (1, 2, 8)) + ".", ""]
    old = open(GATES_MD).read() if os.path.exists(GATES_MD) else ""
    tail = old[old.index(GPU_MARK):] if GPU_MARK in old else GPU_MARK + "\n\n(not measured yet)\n"
    with open(GATES_MD, "w") as f:
        f.write("\n".join(lines) + "\n" + tail)


if __name__ == "__main__":
    write_record()
