"""Strict float32 models of the transmit-side modulators (libcsdr.c:1174-1208, csdr.c:2084-2127), their seeded input cases, and the expected output of the
transmit bank as the composition of these models with the existing yardsticks (oracle.port, resampler_model).

fmmod_fc: PI is the float (float)3.14159265358979323846 (libcsdr.h:65), so the phase chain is float32 throughout:  p = fl(p + fl(x PI)), then
`while (p > PI) p -= 2 PI; while (p <= -PI) p += 2 PI`, every step rounded.  The outputs are float32(cos(float64(p))), float32(sin(float64(p)))."""
import ctypes as C
import functools
import numpy as np

import resampler_model as rm

R = np.float32
PI = R(3.14159265358979323846)
TWO_PI = R(2) * PI
N_FM = 8192


# ------------------------------------------------------------------ fmmod_fc
def fm_phases(x, p0=0.0):
    """the phase after every sample, float32 step by step"""
    x = np.asarray(x, R)
    d = x * PI                                   # float32 products, one rounding each
    out = np.empty(x.size, R)
    p = R(p0)
    for k in range(x.size):
        p = R(p + d[k])
        while p > PI:
            p = R(p - TWO_PI)
        while p <= -PI:
            p = R(p + TWO_PI)
        out[k] = p
    return out


def fm_outputs(phases):
    p = np.asarray(phases, R).astype(np.float64)
    return (np.cos(p).astype(R) + 1j * np.sin(p).astype(R)).astype(np.complex64)


def model_fmmod(x, p0=0.0):
    """-> (outputs complex64, phases float32, last_phase float32)"""
    ph = fm_phases(x, p0)
    return fm_outputs(ph), ph, (ph[-1] if ph.size else R(p0))


FM_CASES = ["tone_noise_dev0.1", "uniform_1", "const_0.3", "const_+1", "const_-1", "uniform_3"]


@functools.lru_cache(maxsize=None)
def _fm_input(case):
    rng = np.random.default_rng(7100 + case)
    n = np.arange(N_FM)
    if case == 0:
        x = 0.1 * (0.8 * np.sin(2 * np.pi * 0.013 * n) + 0.2 * rng.standard_normal(N_FM))
    elif case == 1:
        x = rng.uniform(-1, 1, N_FM)
    elif case == 2:
        x = np.full(N_FM, 0.3)
    elif case == 3:
        x = np.full(N_FM, 1.0)                   # steps of exactly +PI: the `> PI` edge every other sample
    elif case == 4:
        x = np.full(N_FM, -1.0)                  # steps of exactly -PI: the `<= -PI` edge
    else:
        x = rng.uniform(-3, 3, N_FM)             # more than one turn per wrap
    x = x.astype(R)
    x.setflags(write=False)
    return x


def fm_input(case):
    return _fm_input(case)


@functools.lru_cache(maxsize=None)
def _fm_model(case):
    out, ph, last = model_fmmod(_fm_input(case))
    out.setflags(write=False); ph.setflags(write=False)
    return out, ph, last


def fm_model(case):
    """the model over the whole case, computed once: (outputs, phases, last_phase).  The phase after n samples is phases[n - 1]."""
    return _fm_model(case)


# ------------------------------------------------------------------ the elementwise operators
def dsb(x, q=0.0):
    x = np.asarray(x, R)
    return (x + 1j * np.full(x.size, R(q), R)).astype(np.complex64)


def add_dcoffset(z):
    z = np.asarray(z, np.complex64)
    i = (0.5 + (z.real / R(2)).astype(np.float64)).astype(R)      # 0.5 is a double in the reference
    return (i + 1j * (z.imag / R(2))).astype(np.complex64)


def fixed_amplitude(z, amp):
    z = np.asarray(z, np.complex64)
    i, q = z.real.astype(R), z.imag.astype(R)
    now = np.sqrt(i * i + q * q)                                   # float32 products, sum and root
    with np.errstate(divide="ignore", invalid="ignore"):
        gain = np.where(now > 0, R(amp) / now, R(0)).astype(R)
    return ((i * gain) + 1j * (q * gain)).astype(np.complex64)


def samplerf(x, wait):
    """16 bytes per sample: the float as a double, wait_for_this_sample, 0 -> uint8 [16 n]"""
    x = np.asarray(x, R)
    rec = np.zeros(x.size, np.dtype([("v", "<f8"), ("w", "<u4"), ("z", "<u4")]))
    rec["v"] = x.astype(np.float64); rec["w"] = np.uint32(wait)
    return rec.view(np.uint8)


def elementwise_input(n, seed=0, zeros=False):
    rng = np.random.default_rng(7300 + seed)
    z = (0.5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)      # Gaussian, sigma 0.5 per component
    if zeros and n:
        z[:: max(1, n // 7)] = 0
    return z


# ------------------------------------------------------------------ the reference library
def bind(L):
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    L.fmmod_fc.restype = f; L.fmmod_fc.argtypes = [vp, vp, i, f]
    L.add_dcoffset_cc.restype = None; L.add_dcoffset_cc.argtypes = [vp, vp, i]
    L.fixed_amplitude_cc.restype = None; L.fixed_amplitude_cc.argtypes = [vp, vp, i, f]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def lib_fmmod(L, x, p0=0.0, calls=None):
    """fmmod_fc of a library with the reference's signature (the reference itself, or the drop-in), in calls of `calls` samples"""
    x = np.ascontiguousarray(x, R); y = np.zeros(x.size, np.complex64)
    p, at = R(p0), 0
    for k in ([x.size] if calls is None else calls):
        p = R(L.fmmod_fc(_p(x[at:]), _p(y[at:]), int(k), float(p))); at += k
    return y, p


def lib_add_dcoffset(L, z):
    z = np.ascontiguousarray(z, np.complex64); y = np.zeros_like(z)
    L.add_dcoffset_cc(_p(z), _p(y), z.size); return y


def lib_fixed_amplitude(L, z, amp):
    z = np.ascontiguousarray(z, np.complex64); y = np.zeros_like(z)
    L.fixed_amplitude_cc(_p(z), _p(y), z.size, float(amp)); return y


def maxdev(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return float(np.abs(a - b).max(initial=0.0))


def words_differing(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)))


# ------------------------------------------------------------------ the bank
TX_MODES = ("fm", "am", "dsb")


def bank_n_out(n_in_total, I, T):
    """outputs of fir_interpolate_cc over n samples: I per input index i with i I + (I - 1) + T <= n I  (libcsdr.c:583-586)"""
    i = 0
    while i * I + (I - 1) + T <= n_in_total * I:
        i += 1
    return i * I


def bank_audio(n_streams, n, seed=0):
    """spread s16 audio: a tone per stream plus noise, about a third of full scale"""
    rng = np.random.default_rng(7500 + seed)
    k = np.arange(n)
    x = np.empty((n_streams, n), np.int16)
    for s in range(n_streams):
        v = 0.25 * np.sin(2 * np.pi * (0.011 + 0.003 * s) * k + s) + 0.08 * rng.standard_normal(n)
        x[s] = np.clip(np.round(v * 32767), -32767, 32767).astype(np.int16)
    return x


def bank_baseband(port, x_s16, mode, gain, q_value):
    """convert_s16_f | gain_ff | modulator, one stream -> complex64"""
    a = port.gain_ff(port.convert_s16_f(x_s16), gain)
    if mode == "fm":
        return model_fmmod(a)[0]
    z = dsb(a, q_value)
    return add_dcoffset(z) if mode == "am" else z


def bank_expected(port, x_s16, mode, gain, q_value, I, taps, segments, out_format="cf32"):
    """one stream.  segments: [(outputs, rate), ...]; the rotator runs per segment with a fresh 1024-chunk grid and the phase carried; the last segment may give
    None for `everything left` -> complex64 [n_out], or uint8 [n_out, 2]"""
    bb = bank_baseband(port, x_s16, mode, gain, q_value)
    y = rm.fir_interpolate_cc(bb, I, np.asarray(taps, R)).astype(np.complex64)
    out, at, ph = [], 0, 0.0
    for count, rate in segments:
        seg = y[at:] if count is None else y[at:at + count]
        z, ph = port.shift_addition_cc(seg, rate, 1024, ph)
        out.append(z); at += seg.size
    z = np.concatenate(out) if out else np.zeros(0, np.complex64)
    assert at == y.size or segments[-1][0] is not None
    z = z[:y.size]
    if out_format == "u8":
        return port.convert_f_u8(np.ascontiguousarray(z).view(R)).reshape(-1, 2)
    return z
