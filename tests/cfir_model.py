"""The model of the complex-tap FIR (apply_fir_cc, libcsdr.c:2261-2273) in numpy: the library's float32 order (each output part ONE fmaf chain over the 2 T
interleaved tap floats, from 0), float64, the per-output gate of a float32 dot product, other float32 orders, and the reference library through ctypes.

  y[o] = sum_{t < T} x[o + t] h[t]         n - T + 1 outputs of n samples
  y.re[o] = sum_j a_re[j] xf[2 o + j]      a_re[2t] = h[t].re, a_re[2t + 1] = -h[t].im        (xf: the interleaved floats of x)
  y.im[o] = sum_j a_im[j] xf[2 o + j]      a_im[2t] = h[t].im, a_im[2t + 1] =  h[t].re"""
import ctypes as C
import os
import numpy as np

from pulse_model import fma32

f32 = np.float32
c64 = np.complex64
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")
GOLDEN = os.path.join(HERE, "golden", "cfir_ref_vectors.npz")
U = 2.0 ** -24


def tap_floats(h):
    """(a_re, a_im): the 2 T interleaved tap floats of both output parts"""
    h = np.asarray(h, c64)
    a_re = np.empty(2 * h.size, f32); a_im = np.empty(2 * h.size, f32)
    a_re[0::2] = h.real; a_re[1::2] = -h.imag
    a_im[0::2] = h.imag; a_im[1::2] = h.real
    return a_re, a_im


def cfir32(x, h):
    """the library's order: per part, acc = fmaf(a[j], xf[2 o + j], acc) for j = 0 .. 2T-1, from 0; all outputs at once"""
    x = np.ascontiguousarray(x, c64); h = np.asarray(h, c64)
    T, n = h.size, x.size - h.size + 1
    if n <= 0:
        return np.zeros(0, c64)
    xf = x.view(f32)
    a_re, a_im = tap_floats(h)
    re = np.zeros(n, f32); im = np.zeros(n, f32)
    for j in range(2 * T):
        v = xf[j:j + 2 * n:2]
        re = fma32(a_re[j], v, re)
        im = fma32(a_im[j], v, im)
    y = np.empty(n, c64)
    y.real = re; y.imag = im
    return y


def cfir64(x, h):
    """float64"""
    x = np.asarray(x, np.complex128); h = np.asarray(h, np.complex128)
    if x.size < h.size:
        return np.zeros(0, np.complex128)
    return np.correlate(x, np.conj(h), "valid")


def cfir_gate(x, h):
    """(g_re, g_im): per output and part the bound 1.01 gamma_2T c on |y32 - y64| for ANY float32 summation order of the part's 2 T products, with or
    without fma: gamma_n = n U / (1 - n U), U = 2^-24, c_re = sum_t |x.re||h.re| + |x.im||h.im|, c_im = sum_t |x.re||h.im| + |x.im||h.re|"""
    x = np.asarray(x, np.complex128); h = np.asarray(h, np.complex128)
    T = h.size
    if x.size < T:
        return np.zeros(0), np.zeros(0)
    g = 2 * T * U / (1 - 2 * T * U)
    xr, xi, hr, hi = np.abs(x.real), np.abs(x.imag), np.abs(h.real), np.abs(h.imag)
    c_re = np.correlate(xr, hr, "valid") + np.correlate(xi, hi, "valid")
    c_im = np.correlate(xr, hi, "valid") + np.correlate(xi, hr, "valid")
    return 1.01 * g * c_re, 1.01 * g * c_im


def outside(y, y64, gate):
    """the share of outputs with a part outside its gate"""
    y = np.asarray(y, np.complex128)
    return float(np.mean((np.abs(y.real - y64.real) > gate[0]) | (np.abs(y.imag - y64.imag) > gate[1])))


def within(y, y64, gate):
    return y.shape == y64.shape and outside(y, y64, gate) == 0.0


def cfir32_other(x, h, pairwise=False):
    """another float32 order: each part's 2 T rounded products summed sequentially (no fma), or pairwise"""
    x = np.ascontiguousarray(x, c64); h = np.asarray(h, c64)
    T, n = h.size, x.size - h.size + 1
    xf = x.view(f32)
    idx = 2 * np.arange(n)[:, None] + np.arange(2 * T)[None, :]
    W = xf[idx]
    parts = []
    for a in tap_floats(h):
        p = (W * a[None, :]).astype(f32)
        if pairwise:
            while p.shape[1] > 1:
                if p.shape[1] & 1:
                    p = np.concatenate([p, np.zeros((n, 1), f32)], axis=1)
                p = (p[:, 0::2] + p[:, 1::2]).astype(f32)
            parts.append(p[:, 0])
        else:
            parts.append(np.cumsum(p, axis=1, dtype=f32)[:, -1])
    y = np.empty(n, c64)
    y.real, y.imag = parts
    return y


def signal(n, seed, scale=1.0):
    """complex normal samples in float32 (no subnormals: the reference library flushes them)"""
    rng = np.random.default_rng(seed)
    x = (scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(c64)
    xf = x.view(f32)
    xf[np.abs(xf) < 1e-30] = f32(1e-3)
    return x


def random_taps(T, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(T) + 1j * rng.standard_normal(T)) / np.sqrt(2 * T)).astype(c64)


# ---------------------------------------------------------------- the reference library through ctypes
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ref_lib():
    if not os.path.exists(REF_LIB):
        return None
    L = C.CDLL(REF_LIB)
    L.apply_fir_cc.restype = C.c_int
    L.apply_fir_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.firdes_add_peak_c.restype = None
    L.firdes_add_peak_c.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int]
    return L


def ref_apply(L, x, h):
    x = np.ascontiguousarray(x, c64); h = np.ascontiguousarray(h, c64)
    y = np.zeros(max(x.size, 1), c64)
    k = L.apply_fir_cc(_p(x), _p(y), x.size, _p(h), h.size)
    return y[:max(k, 0)].copy()


def ref_peaks(L, length, rates, window=2):
    """csdr.c:2997-3002"""
    t = np.zeros(length, c64)
    for k, r in enumerate(rates):
        L.firdes_add_peak_c(_p(t), length, f32(r), window, 1, int(k == len(rates) - 1))
    return t
