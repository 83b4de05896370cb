"""The gates of test_fir_taps_gpu.py on the CPU: at every shape the GPU tests run, with the same taps and the same input, an honest float32
sum (sequential and pairwise) passes the per-sample gate, and the float64 result of each bug class fails it: reversed taps, one zeroed tap
(first, middle, last), swapped polyphase phases p and I-1-p, conjugated FFT-filter taps.  Also: the impulse comb's exact responses agree
with the float64 references, and the instance table agrees with the transcription of the dispatch."""
import numpy as np
import pytest

import fir_reference as fr
import resampler_model as rm

f32 = np.float32


def _f32_sums(P):
    """float32 sequential and pairwise sums of the rows of the float32 product matrix P"""
    acc = np.zeros(P.shape[0], f32)
    for t in range(P.shape[1]):
        acc = (acc + P[:, t]).astype(f32)
    Q = P
    while Q.shape[1] > 1:
        if Q.shape[1] & 1:
            Q = np.concatenate([Q, np.zeros((Q.shape[0], 1), f32)], axis=1)
        Q = (Q[:, 0::2] + Q[:, 1::2]).astype(f32)
    return acc, Q[:, 0]


def _assert_gate_separates(honest, mutants, ratio):
    for name, y in honest:
        r = ratio(y)
        assert r <= 0.25, "honest %s uses %.3g of the gate" % (name, r)
    for name, y in mutants:
        r = ratio(y)
        assert r > 1.0, "mutation %s passes the gate (%.3g)" % (name, r)


def _mutations(taps, used=None):
    """(name, taps) of the bug classes: reversed, and one zeroed tap at the first / middle / last of the taps the operation uses"""
    used = np.arange(taps.size) if used is None else np.asarray(sorted(used))
    out = [("reversed", taps[::-1].copy())]
    for where, t in (("first", used[0]), ("middle", used[used.size // 2]), ("last", used[-1])):
        m = taps.copy(); m[t] = 0; out.append(("tap %d (%s) zeroed" % (t, where), m))
    return out


def _swap_phase(taps, I, p=0):
    m = taps.copy()
    a, b = m[p::I].copy(), m[I - 1 - p::I].copy()
    k = min(a.size, b.size)
    m[p::I][:k] = b[:k]; m[I - 1 - p::I][:k] = a[:k]
    return m


@pytest.mark.parametrize("D,Lo,Le,want", fr.DECIMATE, ids=["%s-D%d" % (w, d) for d, _, _, w in fr.DECIMATE])
def test_decimate_gate_self_check(D, Lo, Le, want):
    for L in (Lo, Le):
        assert fr.fir_decimate_instance(D, L, 2, 2) == want
        taps = fr.decimate_taps(D, L)
        n = fr.decimate_input_length(D, L, want)
        x = fr.crand(np.random.default_rng(D * 7919 + L), (3, n))[0]          # the GPU test's first stream
        y64, cr, ci = fr.fir_decimate_cc(x, D, taps)
        Wr = np.lib.stride_tricks.sliding_window_view(x.real, L)[::D][:y64.size]
        Wi = np.lib.stride_tricks.sliding_window_view(x.imag, L)[::D][:y64.size]
        sr, pr = _f32_sums((Wr * taps).astype(f32))
        si, pi = _f32_sums((Wi * taps).astype(f32))
        assert np.array_equal(sr, fr.fir_f32_sequential(x.real, D, taps))
        honest = [("sequential", sr + 1j * si), ("pairwise", pr + 1j * pi)]
        mutants = [(nm, fr.fir_decimate_cc(x, D, m)[0]) for nm, m in _mutations(taps)]
        _assert_gate_separates(honest, mutants, lambda y: fr.gate_ratio_cc(y, y64, cr, ci, L))


@pytest.mark.parametrize("Lo,Le,want", fr.FIR_FF, ids=[w for _, _, w in fr.FIR_FF])
def test_fir_ff_gate_self_check(Lo, Le, want):
    for L in (Lo, Le):
        assert fr.fir_ff_instance(L) == want
        taps = fr.ff_taps(L)
        n = 2 * fr.tile_outputs(want) + 37 + L
        x = np.random.default_rng(L).uniform(-1, 1, (3, n)).astype(f32)[0]
        y64, c = fr.fir_ff(x, taps)
        W = np.lib.stride_tricks.sliding_window_view(x, L)[:y64.size]
        s, p = _f32_sums((W * taps).astype(f32))
        mutants = [(nm, fr.fir_ff(x, m)[0]) for nm, m in _mutations(taps)]
        _assert_gate_separates([("sequential", s), ("pairwise", p)], mutants, lambda y: fr.gate_ratio(y, y64, c, L))


def _rr_products(x, I, D, taps, n_out):
    s, d, k = rm.rr_schedule(n_out, I, D, taps.size)
    K = int(k.max())
    i = np.arange(K)[None, :]
    live = i < k[:, None]
    xi = np.where(live, x[np.minimum(s[:, None] + i, x.size - 1)], 0).astype(f32)
    ti = np.where(live, taps[np.minimum(d[:, None] + i * I, taps.size - 1)], 0).astype(f32)
    used = np.unique((d[:, None] + i * I)[live])
    return (xi * ti).astype(f32), used


@pytest.mark.parametrize("I,D,T", fr.RR)
def test_resampler_gate_self_check(I, D, T):
    taps = fr.rr_taps(I, D, T)
    x = np.random.default_rng(I * 31 + D).uniform(-1, 1, (3, 41000)).astype(f32)[0]
    y64, _ = rm.rational_resampler_ff(x, I, D, taps)
    c, _ = rm.rational_resampler_ff(np.abs(x), I, D, np.abs(taps))
    K = -(-T // I)
    P, used = _rr_products(x, I, D, taps, y64.size)
    s, p = _f32_sums(P)
    honest = [("sequential", (s * f32(I)).astype(f32)), ("pairwise", (p * f32(I)).astype(f32))]
    muts = _mutations(taps, used) + ([("phases 0 and %d swapped" % (I - 1), _swap_phase(taps, I))] if I > 1 else [])
    mutants = [(nm, rm.rational_resampler_ff(x, I, D, m)[0]) for nm, m in muts]
    _assert_gate_separates(honest, mutants, lambda y: fr.gate_ratio(y, y64, c, K))


@pytest.mark.parametrize("I,T", fr.INTERP)
def test_interp_gate_self_check(I, T):
    taps = fr.interp_taps(I, T)
    x = fr.crand(np.random.default_rng(I + T), (2, 20000))[0]
    y64 = rm.fir_interpolate_cc(x, I, taps)
    cr = rm.fir_interpolate_cc(np.abs(x.real), I, np.abs(taps)).real
    ci = rm.fir_interpolate_cc(np.abs(x.imag), I, np.abs(taps)).real
    K = -(-T // I)
    # output (q, ip) = sum_{k: (k+1) I - ip < T} x[q + k] taps[(k + 1) I - ip]
    npos = y64.size // I
    q = np.repeat(np.arange(npos), I); ip = np.tile(np.arange(I), npos)
    k = np.arange(K + 1)[None, :]
    t = (k + 1) * I - ip[:, None]
    live = t < T
    xi = x[np.minimum(q[:, None] + k, x.size - 1)]
    ti = np.where(live, taps[np.minimum(t, T - 1)], 0).astype(f32)
    sr, pr = _f32_sums(np.where(live, xi.real * ti, 0).astype(f32))
    si, pi = _f32_sums(np.where(live, xi.imag * ti, 0).astype(f32))
    used = np.unique(t[live])
    muts = _mutations(taps, used) + [("phases 0 and %d swapped" % (I - 1), _swap_phase(taps, I))]
    mutants = [(nm, rm.fir_interpolate_cc(x, I, m)) for nm, m in muts]
    _assert_gate_separates([("sequential", sr + 1j * si), ("pairwise", pr + 1j * pi)], mutants,
                           lambda y: fr.gate_ratio_cc(y, y64, cr, ci, K))


@pytest.mark.parametrize("ntaps,fft", [(1023, 65536), (1041, 65536), (4095, 65536), (1024, 65536), (2046, 65536), (4094, 65536), (8191, 65536), (255, 1024)])
def test_fft_gate_self_check(port, ntaps, fft):
    """the oracle's float32 overlap-add FFT filter passes the FFT gate; the same filter with conjugated taps fails it"""
    rng = np.random.default_rng(ntaps + fft)
    taps = fr.crand(rng, ntaps)
    inp = fft - ntaps + 1
    x = fr.crand(rng, (2, 3 * inp))[0]
    n = x.size
    y64 = fr.convolve_cc(x, taps, n)
    bound = fr.fft_bound(x, taps, n, fft)
    assert np.allclose(y64[:50], np.convolve(x.astype(np.complex128), taps.astype(np.complex128))[:50], rtol=0, atol=1e-12)
    honest = port.bandpass_fir_fft_cc(x, taps, fft)
    assert honest.size == n
    r = fr.fft_gate_ratio(honest, y64, bound)
    assert r <= 0.25, r
    assert fr.fft_gate_ratio(port.bandpass_fir_fft_cc(x, np.conj(taps), fft), y64, bound) > 1.0


def test_impulse_combs_are_exact_references():
    """the comb responses the GPU tests demand bit for bit equal the float64 references rounded to float32"""
    D, L = 7, 45
    taps = fr.random_taps(L, 1)
    n = fr.comb_length(L, D)
    x, pos, amps = fr.impulse_comb(n, L, D, 16, seed=3)
    assert np.all(np.diff(pos) >= L) and pos[0] == 0 and pos[-1] == n - 1
    assert set(pos % D) == set(range(D))
    assert set(np.abs(amps.real) + np.abs(amps.imag)) <= {2.0 ** k for k in range(-3, 4)}
    y64, _, _ = fr.fir_decimate_cc(x, D, taps)
    want = fr.comb_response(y64.size, D, taps, pos, amps)
    assert np.array_equal(want, y64.astype(np.complex64)) and np.count_nonzero(want) > 0
    assert np.array_equal(fr.fir_f32_sequential(x.real, D, taps), want.real)
    for I, Dr, T in fr.RR:
        taps = fr.rr_taps(I, Dr, T)
        x, pos, amps = fr.impulse_comb(30000, T, 1, None, seed=T, complex_=False)
        y64, _ = rm.rational_resampler_ff(x, I, Dr, taps)
        want = fr.rr_comb_response(y64.size, I, Dr, taps, pos, amps)
        assert np.array_equal(want, y64.astype(f32)) and np.count_nonzero(want) > 0
    for I, T in fr.INTERP:
        taps = fr.interp_taps(I, T)
        x, pos, amps = fr.impulse_comb(20000, T, 1, None, seed=T + I)
        y64 = rm.fir_interpolate_cc(x, I, taps)
        want = fr.interp_comb_response(y64.size, I, taps, pos, amps)
        assert np.array_equal(want, y64.astype(np.complex64)) and np.count_nonzero(want) > 0


def test_instance_table_matches_dispatch():
    """every row's odd and even taps reach the row's instance; mfma3 rows fall back to k_fir_mfma on odd input lengths and odd pitches"""
    for D, Lo, Le, want in fr.DECIMATE:
        for L in (Lo, Le):
            assert fr.fir_decimate_instance(D, L, 20000, 20000) == want
            if want.startswith("k_fir_mfma3"):
                assert fr.fir_decimate_instance(D, L, 20001, 20001).startswith("k_fir_mfma<8,")
                assert fr.fir_decimate_instance(D, L, 20000, 20001).startswith("k_fir_mfma<8,")
    assert {w for *_, w in fr.DECIMATE} >= {"k_fir_poly<R%d,U%d>" % (r, u) for r in (4, 2) for u in (24, 44)} | {"k_fir_generic"}
    assert fr.fir_decimate_instance(10, 8200, 20000, 20000) == "k_fir_generic" and fr.fir_decimate_instance(10, 100000, 2, 2) is None
