"""CPU validation of the matrix-core receiver front end's weight table and index arithmetic (csdr_amd/csrc/ddc_mfma.hip):
one tile evaluated the way k_ddc_mfma does (one phase-independent weight set, K-range split over four waves, snapshot / half-K-step
handling of 1024-chunk boundaries, post factors C_m D^e, prefix-sum offset constants; exact int8 digit arithmetic as
v_mfma_i32_16x16x64_i8 does) must equal the direct double-precision evaluation of
    y[k] = sum_t h[t] * R[n] * u8_to_float(x[n]),   R[n] = C_chunk(n) * D^(n mod 1024)
for every 16-sample position of the tile inside a chunk (all boundary positions in all four waves)."""
import ctypes as C
import numpy as np
import pytest

import ddc_reference
import fir_reference

f32 = np.float32


OLD_SHAPES = [(50, 801, 0.11), (50, 801, -0.4321), (10, 79, -0.085), (20, 321, 0.3)]
# every decimation class of the kernel family (tests/ddc_reference.py: SHAPES) and the edges of ddc_mfma_supported: smallest / largest D, the window limit
# 7 D + L = 1152, the longest history, both sides of the two-team limit D = 80; rates of both rotator classes
NEW_SHAPES = [(2, 63, 0.25), (2, 1025, 0.05), (4, 1025, -0.3), (6, 1025, 0.499), (16, 255, -0.4321), (64, 704, 0.3), (80, 592, -0.2718), (82, 578, 0.25),
              (100, 451, -0.085), (128, 255, 0.05), (160, 31, 0.2), (164, 4, 1e-4)]


def _check(D, Lt, rate, kind, worst, scale, ratio, old_gate):
    """The gate is ddc_reference's kappa(L) u c + Q per output (the tile has random seeds and an ideal d^k: no rotator term).  1e-6 max(sum |h|, 1), the gate of the
    four original shapes, is no bound -- designed lowpass taps at (2, 1025, 0.05) exceed it: their large centre taps make the 23-bit weight step large relative
    to sum |h| --; the original shapes are held to both."""
    old = worst / (1e-6 * max(scale, 1.0))
    print("RATIO tile D=%d L=%d rate=%g %s: %.4f x the gate, %.4f x 1e-6 max(sum |h|, 1)" % (D, Lt, rate, kind, ratio, old))
    assert ratio <= 1.0, ratio
    if old_gate:
        assert old < 1.0, worst


@pytest.mark.parametrize("D,Lt,rate", OLD_SHAPES + [s for s in NEW_SHAPES if s[1] % 2])
def test_ddc_tile_matches_direct_evaluation(port, D, Lt, rate):
    """designed lowpass taps: odd lengths only (the oracle's firdes_lowpass_f, like the reference's, writes one element past an even-length buffer)"""
    worst, scale, ratio = _ddc_tile_worst(port.firdes_lowpass_f(Lt, 0.5 / D), D, rate)
    _check(D, Lt, rate, "lowpass", worst, scale, ratio, (D, Lt, rate) in OLD_SHAPES)


@pytest.mark.parametrize("D,Lt,rate", OLD_SHAPES + NEW_SHAPES)
def test_ddc_tile_asymmetric_taps(D, Lt, rate):
    """The same with random taps without symmetry, which would show reversed or mirrored tap indices in the weight table."""
    worst, scale, ratio = _ddc_tile_worst(fir_reference.random_taps(Lt, D + Lt), D, rate)
    _check(D, Lt, rate, "random", worst, scale, ratio, (D, Lt, rate) in OLD_SHAPES)


def _ddc_tile_worst(taps, D, rate):
    """(worst |tile output - direct double-precision evaluation|, sum |taps|, worst error / gate per component) over every 16-sample tile position inside a chunk"""
    Lt = taps.size
    import csdr_amd
    L = csdr_amd.lib()
    fn = L.csdr_amd_debug_ddc_mfma_tile
    fn.argtypes = [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(11)
    d = ddc_reference.step_phasor(rate)
    Dk = d ** np.arange(1024)
    q = ddc_reference.weight_step(D, Lt, taps, rate)
    out = np.zeros(16, f32)
    worst = ratio = 0.0
    scale = np.abs(taps).sum()
    h = taps.astype(np.float64)
    for pos in range(0, 1024, 16):                               # every position of the tile start inside a chunk
        n0 = 1024 * 7 + pos
        window = rng.integers(0, 256, 2304, dtype=np.uint8)
        ct = np.array([[np.cos(a), np.sin(a)] for a in rng.uniform(-np.pi, np.pi, 3)], f32)   # unrelated seeds: a wrong chunk assignment shows
        assert fn(D, Lt, rate, taps.ctypes.data, n0, window.ctypes.data, ct.ctypes.data, out.ctypes.data) == 0
        xs = window.astype(np.float64) / 127.5 - 1.0
        xc = xs[0::2] + 1j * xs[1::2]
        vs = window.astype(np.float64) - 128.0
        Cc = ct[:, 0].astype(np.float64) + 1j * ct[:, 1].astype(np.float64)
        for o in range(8):
            n = n0 + D * o + np.arange(Lt)
            R = Cc[(n >> 10) - (n0 >> 10)] * Dk[n & 1023]
            xw = xc[D * o:D * o + Lt]
            y = np.sum(h * R * xw)
            got = complex(out[2 * o], out[2 * o + 1])
            worst = max(worst, abs(got - y))
            vw = vs[2 * D * o:2 * (D * o + Lt)]
            bnd = ddc_reference.bound(np.sum(np.abs(h) * (np.abs(xw.real) + np.abs(xw.imag))), np.abs(vw).sum(), np.sqrt((vw ** 2).sum()), Lt, q, 0.0)
            ratio = max(ratio, abs(got.real - y.real) / bnd, abs(got.imag - y.imag) / bnd)
    return worst, scale, ratio


def test_ddc_unsupported_shapes():
    import csdr_amd
    L = csdr_amd.lib()
    fn = L.csdr_amd_debug_ddc_mfma_tile
    fn.argtypes = [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    taps = np.ones(2000, f32); w = np.zeros(2304, np.uint8); ct = np.zeros(6, f32); out = np.zeros(16, f32)
    assert fn(51, 801, 0.1, taps.ctypes.data, 0, w.ctypes.data, ct.ctypes.data, out.ctypes.data) == -1      # odd decimation
    assert fn(50, 1200, 0.1, taps.ctypes.data, 0, w.ctypes.data, ct.ctypes.data, out.ctypes.data) == -1     # window too long
    assert fn(50, 801, 0.1, taps.ctypes.data, 8, w.ctypes.data, ct.ctypes.data, out.ctypes.data) == -1      # tile start not 16-sample aligned
