"""Every tap-consuming kernel with random asymmetric taps against float64 (fir_reference.py): a per-sample error gate on random input and exact
equality on an impulse comb.  Symmetric lowpass designs hide reversed taps, mirrored tap indices and swapped polyphase phases; a whole-stream
relative-RMS gate hides a dropped end tap.  Each fir_decimate_cc / fir_ff shape asserts the template instance it reaches
(csdr_amd_fir_last_instance), so a change in the dispatch fails here instead of silently dropping coverage."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

import fir_reference as fr
import resampler_model as rm
from oracle import relrms
from tests_helpers import wfm_signal_u8, nfm_signal_u8

pytestmark = pytest.mark.gpu
c64, f32 = np.complex64, np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 1e30                  # in the row padding behind input_size: a kernel that lets it reach a non-zero weight produces a huge output

DECIMATE, FIR_FF = fr.DECIMATE, fr.FIR_FF


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _report(*a):
    print("RATIO", *a)


# ------------------------------------------------------------------ raw calls (pitched rows, sentinel padding)
def _call_decimate(ctx, x, pitch, D, taps):
    """x [s, n] complex64 in rows of `pitch` samples (padding = SENTINEL) -> (y [s, n_out], instance)"""
    s, n = x.shape
    rows = np.full((s, pitch), SENTINEL, c64); rows[:, :n] = x
    n_out = (n - taps.size) // D + 1
    opitch = n_out + 3
    di = ctx.upload(rows); dt = ctx.upload(taps); do = ctx.alloc(8 * s * opitch + 64)
    no = ctx.check(ctx.L.csdr_amd_fir_decimate_cc(ctx.h, di.ptr, do.ptr, s, n, pitch, opitch, D, dt.ptr, taps.size), "fir_decimate_cc")
    assert no == n_out
    y = ctx.download(do, c64, s * opitch).reshape(s, opitch)[:, :n_out]
    return y, ctx.L.csdr_amd_fir_last_instance().decode()


def _call_ff(ctx, x, pitch, taps):
    s, n = x.shape
    rows = np.full((s, pitch), SENTINEL, f32); rows[:, :n] = x
    n_out = n - taps.size
    opitch = n_out + 3
    di = ctx.upload(rows); dt = ctx.upload(taps); do = ctx.alloc(4 * s * opitch + 64)
    no = ctx.check(ctx.L.csdr_amd_fir_ff(ctx.h, di.ptr, do.ptr, s, n, pitch, opitch, dt.ptr, taps.size), "fir_ff")
    assert no == n_out
    y = ctx.download(do, f32, s * opitch).reshape(s, opitch)[:, :n_out]
    return y, ctx.L.csdr_amd_fir_ff_last_instance().decode()


# ------------------------------------------------------------------ a) fir_decimate_cc
def check_decimate_shape(ctx, D, L, want, force_generic=False):
    """random input on 3 / 4 / 3 streams (tight rows, rows with a larger pitch, one call shorter than a tile, and an odd input length where
    k_fir_mfma3 must fall back) under the per-sample gate, then the impulse comb for exact equality -> worst gate ratio"""
    taps = fr.decimate_taps(D, L)
    rng = np.random.default_rng(D * 7919 + L)
    tile = fr.tile_outputs(want)
    n_tile = fr.decimate_input_length(D, L, want)
    cases = [(3, n_tile, n_tile), (4, n_tile, n_tile + 6), (3, 4 * D + L + (L & 1), 4 * D + L + (L & 1) + 10)]
    if want.startswith("k_fir_mfma3"):
        cases.append((3, n_tile + 1, n_tile + 1))                  # odd input length: k_fir_mfma
    worst = 0.0
    for s, n, pitch in cases:
        exp = fr.fir_decimate_instance(D, L, n, pitch, force_generic)
        x = fr.crand(rng, (s, n))
        y, inst = _call_decimate(ctx, x, pitch, D, taps)
        assert inst == exp, (D, L, n, pitch, inst, exp)
        for r in range(s):
            y64, cr, ci = fr.fir_decimate_cc(x[r], D, taps)
            g = fr.gate_ratio_cc(y[r], y64, cr, ci, L)
            assert g <= 1.0, "%s D=%d L=%d n=%d pitch=%d stream %d: error %.3g x the gate" % (inst, D, L, n, pitch, r, g)
            worst = max(worst, g)
    n = max(fr.comb_length(L, D), n_tile)
    n += n & 1
    xs, combs = [], []
    for r in range(2):
        x, pos, amps = fr.impulse_comb(n, L, D, tile, seed=r + L)
        xs.append(x); combs.append((pos, amps))
    y, inst = _call_decimate(ctx, np.stack(xs), n + 4, D, taps)
    assert inst == fr.fir_decimate_instance(D, L, n, n + 4, force_generic)
    for r in range(2):
        want_y = fr.comb_response(y.shape[1], D, taps, *combs[r])
        bad = np.nonzero(y[r] != want_y)[0]
        assert bad.size == 0, "%s D=%d L=%d: impulse comb differs at %d outputs, first %d: %r vs %r" % (inst, D, L, bad.size, bad[0], y[r, bad[0]], want_y[bad[0]])
    return worst


@pytest.mark.parametrize("D,Lo,Le,want", DECIMATE, ids=["%s-D%d" % (w, d) for d, _, _, w in DECIMATE])
def test_fir_decimate_cc_asymmetric_taps(ctx, D, Lo, Le, want):
    for L in (Lo, Le):
        assert fr.fir_decimate_instance(D, L, 2, 2) == want
        _report(want, "D=%d L=%d" % (D, L), "%.4f" % check_decimate_shape(ctx, D, L, want))


# ------------------------------------------------------------------ b) fir_ff
def check_ff_shape(ctx, L, want, force_generic=False):
    taps = fr.ff_taps(L)
    rng = np.random.default_rng(L)
    tile = fr.tile_outputs(want)
    n_tile = 2 * tile + 37 + L
    worst = 0.0
    for s, n, pitch in [(3, n_tile, n_tile), (4, n_tile, n_tile + 5), (3, L + 7, L + 9)]:
        x = rng.uniform(-1, 1, (s, n)).astype(f32)
        y, inst = _call_ff(ctx, x, pitch, taps)
        assert inst == fr.fir_ff_instance(L, force_generic), (L, inst)
        for r in range(s):
            y64, c = fr.fir_ff(x[r], taps)
            g = fr.gate_ratio(y[r], y64, c, L)
            assert g <= 1.0, "%s L=%d n=%d stream %d: error %.3g x the gate" % (inst, L, n, r, g)
            worst = max(worst, g)
    n = max(fr.comb_length(L), n_tile)
    x, pos, amps = fr.impulse_comb(n, L, 1, tile, seed=L, complex_=False)
    y, inst = _call_ff(ctx, x[None], n + 3, taps)
    want_y = fr.comb_response(y.shape[1], 1, taps, pos, amps)
    bad = np.nonzero(y[0] != want_y)[0]
    assert bad.size == 0, "%s L=%d: impulse comb differs at %d outputs, first %d" % (inst, L, bad.size, bad[0])
    return worst


@pytest.mark.parametrize("Lo,Le,want", FIR_FF, ids=[w for _, _, w in FIR_FF])
def test_fir_ff_asymmetric_taps(ctx, Lo, Le, want):
    for L in (Lo, Le):
        assert fr.fir_ff_instance(L) == want
        _report("fir_ff", want, "L=%d" % L, "%.4f" % check_ff_shape(ctx, L, want))


def _generic_child():
    """run in a fresh process with CSDR_AMD_FIR_GENERIC=1 (read once per process by fir.hip)"""
    import torch  # noqa: F401
    import csdr_amd
    c = csdr_amd.Context(0)
    for D, Lo, Le, _ in DECIMATE:
        for L in (Lo, Le):
            want = fr.fir_decimate_instance(D, L, 2, 2, True)
            _report("generic-switch", want, "D=%d L=%d" % (D, L), "%.4f" % check_decimate_shape(c, D, L, want, True))
    for Lo, Le, _ in FIR_FF:
        for L in (Lo, Le):
            _report("generic-switch fir_ff k_fir_generic", "L=%d" % L, "%.4f" % check_ff_shape(c, L, "k_fir_generic", True))
    c.close()


def test_fir_generic_switch_asymmetric_taps():
    """the same checks with CSDR_AMD_FIR_GENERIC=1: a child process, because the switch is read once per process"""
    env = dict(os.environ, CSDR_AMD_FIR_GENERIC="1")
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(1, %r); import test_fir_taps_gpu as t; t._generic_child()" % (HERE, os.path.dirname(HERE))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("RATIO") == 2 * (len(DECIMATE) + len(FIR_FF))


# ------------------------------------------------------------------ c) rational_resampler_ff and fir_interpolate_cc
CALLS = [7001, 0, 1, 12000, 1, 0, 20997]


@pytest.mark.parametrize("I,D,T", fr.RR)
@pytest.mark.parametrize("generic", [False, True])
def test_rational_resampler_asymmetric_taps(ctx, I, D, T, generic):
    import csdr_amd
    assert I == 1 or T % I
    taps = fr.rr_taps(I, D, T)
    rng = np.random.default_rng(I * 31 + D)
    n = sum(CALLS)
    x = rng.uniform(-1, 1, (3, n)).astype(f32)
    r = csdr_amd.Resampler(ctx, I, D, taps, 3)
    if generic:
        r.force_generic()
    y = r.process(x, CALLS)
    assert r.kernel_name() == ("k_rr_generic" if generic else "k_rr_poly")
    r.close()
    K = -(-T // I)
    worst = 0.0
    for s in range(3):
        want, _ = rm.rational_resampler_ff(x[s], I, D, taps)
        c, _ = rm.rational_resampler_ff(np.abs(x[s]), I, D, np.abs(taps))
        assert y.shape[1] == want.size
        g = fr.gate_ratio(y[s], want, c, K)
        assert g <= 1.0, "stream %d: error %.3g x the gate" % (s, g)
        worst = max(worst, g)
    _report("k_rr_generic" if generic else "k_rr_poly", "I=%d D=%d T=%d" % (I, D, T), "%.4f" % worst)
    # the comb: impulses T apart, so every output sees at most one; expected a * float32(h * I)
    xc, pos, amps = fr.impulse_comb(n, T, 1, None, seed=T, complex_=False)
    r = csdr_amd.Resampler(ctx, I, D, taps, 1)
    if generic:
        r.force_generic()
    yc = r.process(xc, CALLS)
    r.close()
    want_c = fr.rr_comb_response(yc.size, I, D, taps, pos, amps)
    bad = np.nonzero(yc != want_c)[0]
    assert bad.size == 0, "impulse comb differs at %d outputs, first %d: %r vs %r" % (bad.size, bad[0], yc[bad[0]], want_c[bad[0]])


@pytest.mark.parametrize("I,T", fr.INTERP)
@pytest.mark.parametrize("generic", [False, True])
def test_fir_interpolate_asymmetric_taps(ctx, I, T, generic):
    import csdr_amd
    assert T % I
    taps = fr.interp_taps(I, T)
    rng = np.random.default_rng(I + T)
    n = 20000
    calls = [6999, 0, 1, 5000, 1, 0, 7999]
    x = fr.crand(rng, (2, n))
    p = csdr_amd.Interpolator(ctx, I, taps, 2)
    if generic:
        p.force_generic()
    y = p.process(x, calls)
    assert p.kernel_name() == ("k_interp_generic" if generic else "k_interp_poly")
    p.close()
    K = -(-T // I)
    worst = 0.0
    for s in range(2):
        want = rm.fir_interpolate_cc(x[s], I, taps)
        cr = rm.fir_interpolate_cc(np.abs(x[s].real), I, np.abs(taps)).real
        ci = rm.fir_interpolate_cc(np.abs(x[s].imag), I, np.abs(taps)).real
        assert y.shape[1] == want.size
        g = fr.gate_ratio_cc(y[s], want, cr, ci, K)
        assert g <= 1.0, "stream %d: error %.3g x the gate" % (s, g)
        worst = max(worst, g)
    _report("k_interp_generic" if generic else "k_interp_poly", "I=%d T=%d" % (I, T), "%.4f" % worst)
    xc, pos, amps = fr.impulse_comb(n, T, 1, None, seed=T + I)
    p = csdr_amd.Interpolator(ctx, I, taps, 1)
    if generic:
        p.force_generic()
    yc = p.process(xc, calls)
    p.close()
    want_c = fr.interp_comb_response(yc.size, I, taps, pos, amps)
    bad = np.nonzero(yc != want_c)[0]
    assert bad.size == 0, "impulse comb differs at %d outputs, first %d: %r vs %r" % (bad.size, bad[0], yc[bad[0]], want_c[bad[0]])


# ------------------------------------------------------------------ d) bandpass_fir_fft_cc with random complex taps
# (taps, fft_size, streams, blocks per call, CSDR_AMD_FFTFILT_LDS_MODE or None, CSDR_AMD_FFTFILT_LDS_OFF, the kernel, its window)
FFT_PATHS = [
    (1023, 65536, 2, None, "6", False, "k_fftfilt_wave", 4096),
    (1041, 65536, 2, 2, None, False, "k_fftfilt_team<2>", 8192),
    (4095, 65536, 2, 1, None, False, "k_fftfilt_team<4>", 16384),
    (1024, 65536, 2, 1, None, False, "k_fftfilt_lds<4096>", 4096),           # even taps: odd blocks of 64513 samples, the 256- / 512-thread kernels
    (2046, 65536, 2, 1, None, False, "k_fftfilt_lds<8192>", 8192),
    (4094, 65536, 2, 1, None, False, "k_fftfilt_lds<16384>", 16384),
    (8191, 65536, 1, 1, None, False, "", 0),
    (1023, 65536, 2, 2, None, True, "", 0),
    (255, 1024, 2, 2, None, True, "", 0),
]


@pytest.mark.parametrize("ntaps,fft,s,per,mode,lds_off,kernel,window", FFT_PATHS, ids=["%s-%d-%d" % (p[6] or "full", p[0], p[1]) for p in FFT_PATHS])
def test_bandpass_fir_fft_random_complex_taps(ctx, monkeypatch, ntaps, fft, s, per, mode, lds_off, kernel, window):
    if mode:
        monkeypatch.setenv("CSDR_AMD_FFTFILT_LDS_MODE", mode)
    if lds_off:
        monkeypatch.setenv("CSDR_AMD_FFTFILT_LDS_OFF", "1")
    rng = np.random.default_rng(ntaps + fft)
    taps = fr.crand(rng, ntaps)
    inp = fft - ntaps + 1
    nb = 3
    n = inp * nb
    x = fr.crand(rng, (s, n))
    f = ctx.L.csdr_amd_fftfilt_create(ctx.h, fft, taps.ctypes.data_as(C.c_void_p), ntaps, s, per or nb)
    assert f
    try:
        di = ctx.upload(x); do = ctx.alloc(x.nbytes + 64)
        b = 0
        names = set()
        while b < nb:
            k = min(per or nb, nb - b)
            ctx.check(ctx.L.csdr_amd_fftfilt_process(f, di.at(8 * b * inp), do.at(8 * b * inp), k, n, n), "fftfilt")
            names.add(ctx.L.csdr_amd_fftfilt_kernel_name(f).decode())
            b += k
        assert names == {kernel} and ctx.L.csdr_amd_fftfilt_window(f) == window, (names, ctx.L.csdr_amd_fftfilt_window(f))
        y = ctx.download(do, c64, s * n).reshape(s, n)
    finally:
        ctx.L.csdr_amd_fftfilt_destroy(f)
    worst = 0.0
    for r in range(s):
        y64 = fr.convolve_cc(x[r], taps, n)
        g = fr.fft_gate_ratio(y[r], y64, fr.fft_bound(x[r], taps, n, fft))
        assert g <= 1.0, "stream %d: error %.3g x the gate" % (r, g)
        worst = max(worst, g)
    _report(kernel or "full-size", "taps=%d fft=%d" % (ntaps, fft), "%.4f" % worst)


# ------------------------------------------------------------------ e) chains that take caller taps
@pytest.mark.parametrize("D,L", [(10, 79), (20, 321), (50, 801)])
def test_ddc_u8_asymmetric_taps(ctx, port, D, L):
    rate = 0.11
    taps = fr.random_taps(L, 300 + L)
    n = 1024 * 100 + 500
    base = [nfm_signal_u8(700 + s, n, offset=-rate) for s in range(2)]
    y = ctx.ddc_u8(np.stack([base[s % 2] for s in range(17)]), rate, D, taps)
    for s in (0, 1, 16):
        sh, _ = port.shift_addition_cc(port.convert_u8_f(base[s % 2]).view(c64), rate)
        w = port.fir_decimate_cc(sh, D, taps)
        assert y.shape[1] == w.size and relrms(y[s], w) <= 1e-5, (ctx.ddc_kernels, relrms(y[s], w))


@pytest.mark.parametrize("D,L", [(10, 79), (10, 160), (10, 237)])      # (the chain's history holds D + L + 8 <= 256 samples: wfm.hip refuses 20 / 321 and 50 / 801)
def test_wfm_chain_asymmetric_taps(ctx, port, D, L):
    taps = fr.random_taps(L, 400 + L)
    n = 16384 * 6
    u8 = wfm_signal_u8(800 + D, n)
    s16, af = ctx.wfm_chain(np.stack([u8, u8]), -0.085, D, taps)
    ps, pf = port.wfm_chain(u8, -0.085, D, taps)
    m = min(pf.size, af.shape[1])
    assert m > (n - L) // (5 * D) - 8
    for s in range(2):
        assert relrms(af[s, :m], pf[:m]) < 1e-5, (ctx.last_wfm_kernel, relrms(af[s, :m], pf[:m]))
        assert np.abs(s16[s, :m].astype(np.int32) - ps[:m]).max() <= 1


def test_fractional_decimator_asymmetric_taps(ctx, port):
    rng = np.random.default_rng(12)
    x = rng.uniform(-1, 1, 50000).astype(f32)
    for rate, L in [(2.5, 133), (4.17, 120)]:
        taps = fr.random_taps(L, 600 + L)
        a, b = ctx.fractional_decimator_ff(x, rate, taps=taps), port.fractional_decimator_ff(x, rate, taps=taps)
        assert a.size == b.size and relrms(a, b) < 1e-5
