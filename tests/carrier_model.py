"""Float32 model of carrier recovery (libcsdr.c: bpsk_costas_loop_cc 2108-2142, pll_cc 1874-1915, their init functions 1856-1871 and 2094-2106), the test
signals, and one ctypes driver for the reference library and the drop-in library.

The model keeps C's order of float32 operations.  Each +, - and * is done on Python floats (doubles) and rounded to float32 at once, which gives the float32
operation's own result (a double holds the exact sum or product of two float32 values far inside its precision, so rounding twice is rounding once); it is
ten times faster than arithmetic on numpy scalars and bit for bit the same.  cos, sin and atan2 are the C library's double functions rounded to float32, as
the reference takes them on float operands."""
import ctypes as C
import math
import struct
import numpy as np

f32 = np.float32
_pack, _unpack = struct.Struct("f").pack, struct.Struct("f").unpack


def R(v):
    """round a Python float to float32"""
    return _unpack(_pack(v))[0]


PI = R(math.pi)                     # libcsdr.h:65: a float
TWO_PI = 2 * PI                     # exact in float32
HALF_PI = PI / 2

COSTAS, COSTAS_DD, PLL_P, PLL_PI = 0, 1, 2, 3
N = 8192                            # samples per test signal

# (bandwidth, damping, decision_directed, carrier offset in cycles per sample, SNR dB)
COSTAS_CASES = [(0.05, .707, 0, .001, 30), (0.05, .707, 1, .001, 30), (0.1, .707, 1, .002, 20), (0.05, .707, 0, .002, 10), (0.01, .707, 0, .0005, 20),
                (0.05, .707, 1, .002, 6)]
# (type, alpha (P) or bandwidth (PI), tone in cycles per sample, SNR dB); PI: ko 10, kd 0.1, damping 0.707
PLL_CASES = [("P", 0.01, 0.0005, 30), ("P", 0.01, 0.005, 10), ("P", 0.1, 0.02, 3), ("P", 0.1, 0.002, 20),
             ("PI", 0.01, 0.0005, 30), ("PI", 0.01, 0.005, 10), ("PI", 0.05, 0.02, 3), ("PI", 0.05, 0.002, 20)]
PLL_KO, PLL_KD, PLL_DAMPING = 10.0, 0.1, 0.707


# ------------------------------------------------------------------ coefficients
def costas_coefficients(bandwidth, damping):
    """init_bpsk_costas_loop_cc -> (alpha, beta, dphase_max): all float32, PI the float constant.  The denominator follows the order of the reference's
    -ffast-math build, (bw bw + 1) + 2 (damping bw); the factors 2 and 4 elsewhere are exact in any order"""
    bandwidth, damping = R(bandwidth), R(damping)
    bw = R(TWO_PI * bandwidth)
    den = R(R(R(bw * bw) + 1) + 2 * R(damping * bw))
    return R(R(R(4 * damping) * bw) / den), R(R(R(4 * bw) * bw) / den), bw


def pll_pi_coefficients(bandwidth, ko=PLL_KO, kd=PLL_KD, damping=PLL_DAMPING):
    """pll_cc_init_pi_controller -> (alpha, beta): 2 * M_PI * bandwidth in double, stored to float32"""
    bandwidth, ko, kd, damping = R(bandwidth), R(ko), R(kd), R(damping)
    bw = R(2 * math.pi * bandwidth)
    return R(R(R(damping * 2) * bw) / R(ko * kd)), R(R(bw * bw) / R(R(1 * ko) * kd))


# ------------------------------------------------------------------ the loops
def costas(x, alpha, beta, dphase_max, dd=False, reset_to_zero=False, state=(0.0, 0.0, 0.0)):
    """bpsk_costas_loop_cc over x (complex64) -> (dict out / error / dphase / nco, state (phase, dphase, freq))"""
    x = np.asarray(x, np.complex64)
    xi, xq = x.real.astype(np.float64).tolist(), x.imag.astype(np.float64).tolist()
    alpha, beta, dmax = R(alpha), R(beta), R(dphase_max)
    phase, d, freq = (R(v) for v in state)
    n = x.size
    out = np.empty((n, 2), f32); nco = np.empty((n, 2), f32); err = np.empty(n, f32); dph = np.empty(n, f32)
    cos, sin, atan2 = math.cos, math.sin, math.atan2
    for k in range(n):
        a, b = xi[k], xq[k]
        ni, nq = R(cos(phase)), R(sin(phase))
        oi = R(R(a * ni) - R(b * nq)); oq = R(R(a * nq) + R(ni * b))
        if dd:
            ph = R(atan2(oq, oi))
            if abs(ph) < HALF_PI:
                e = -ph
            else:
                e = R(PI - ph)
                while e > PI:
                    e = R(e - TWO_PI)
        else:
            e = R(R(PI * oi) * oq)
        freq = R(freq + R(e * beta))
        d = R(R(e * alpha) + freq)
        if d > dmax:
            d = 0.0 if reset_to_zero else dmax
        if d < -dmax:
            d = 0.0 if reset_to_zero else -dmax
        phase = R(phase + d)
        while phase > TWO_PI:
            phase = R(phase - TWO_PI)
        while phase <= 0:
            phase = R(phase + TWO_PI)
        out[k, 0] = oi; out[k, 1] = oq; nco[k, 0] = ni; nco[k, 1] = nq; err[k] = e; dph[k] = d
    return dict(out=out.view(np.complex64)[:, 0], error=err, dphase=dph, nco=nco.view(np.complex64)[:, 0]), (phase, d, freq)


def _wrap(v):
    while v > PI:
        v = R(v - TWO_PI)
    while v < -PI:
        v = R(v + TWO_PI)
    return v


def pll(x, pi_controller, alpha, beta=0.0, state=(0.0, 0.0, 0.0)):
    """pll_cc over x -> (dict dphase (= -dphase, the reference's output) / nco (sin, cos), state (output_phase, dphase, iir_temp))"""
    x = np.asarray(x, np.complex64)
    xi, xq = x.real.astype(np.float64).tolist(), x.imag.astype(np.float64).tolist()
    alpha, beta = R(alpha), R(beta)
    phase, d, tmp = (R(v) for v in state)
    n = x.size
    nco = np.empty((n, 2), f32); dph = np.empty(n, f32)
    cos, sin, atan2 = math.cos, math.sin, math.atan2
    for k in range(n):
        phase = _wrap(R(phase + d))
        nco[k, 0] = R(sin(phase)); nco[k, 1] = R(cos(phase))
        nd = _wrap(R(R(atan2(xi[k], xq[k])) - phase))             # atan2(i, q): the reference's operand order
        if pi_controller:
            d = R(R(nd * alpha) + tmp)
            tmp = R(tmp + R(nd * beta))
            d = _wrap(d)
        else:
            d = R(nd * alpha)
        dph[k] = -d
    return dict(dphase=dph, nco=nco.view(np.complex64)[:, 0]), (phase, d, tmp)


def run_case(params_mode, x, alpha, beta=0.0, dphase_max=0.0, state=(0.0, 0.0, 0.0)):
    """the model by library mode number"""
    if params_mode <= COSTAS_DD:
        return costas(x, alpha, beta, dphase_max, params_mode == COSTAS_DD, False, state)
    return pll(x, params_mode == PLL_PI, alpha, beta, state)


# ------------------------------------------------------------------ signals
def bpsk_signal(n, sps, offset, snr_db, seed, phase=None, amplitude=0.5):
    """BPSK at sps samples per symbol with raised-cosine smoothed transitions, a carrier offset (cycles per sample) and start phase, AWGN"""
    rng = np.random.default_rng(seed)
    phase = rng.uniform(0, 2 * np.pi) if phase is None else phase
    sym = rng.integers(0, 2, n // sps + 2) * 2.0 - 1.0
    base = np.repeat(sym, sps)
    w = np.hanning(sps // 2 + 2)[1:-1]; w /= w.sum()
    base = np.convolve(base, w, mode="same")[:n]
    k = np.arange(n)
    x = amplitude * base * np.exp(1j * (2 * np.pi * offset * k + phase))
    sigma = math.sqrt(amplitude ** 2 / 10 ** (snr_db / 10) / 2)
    x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def tone_signal(n, freq, snr_db, seed, phase=None, amplitude=0.5):
    rng = np.random.default_rng(seed)
    phase = rng.uniform(0, 2 * np.pi) if phase is None else phase
    k = np.arange(n)
    x = amplitude * np.exp(1j * (2 * np.pi * freq * k + phase))
    sigma = math.sqrt(amplitude ** 2 / 10 ** (snr_db / 10) / 2)
    x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def costas_input(case_index, n=N, channel=0):
    """the committed input of COSTAS_CASES[case_index]; `channel` varies seed, phase and offset so that swapped channels show"""
    bw, damping, dd, offset, snr = COSTAS_CASES[case_index]
    return bpsk_signal(n, 16 if (case_index + channel) % 2 == 0 else 32, offset * (1 + 0.03 * channel), snr, 3000 + 17 * case_index + 101 * channel)


def pll_input(case_index, n=N, channel=0):
    kind, coef, freq, snr = PLL_CASES[case_index]
    return tone_signal(n, freq * (1 + 0.03 * channel), snr, 2000 + 17 * case_index + 101 * channel)


def costas_mode_coefficients(case_index):
    """-> (mode, alpha, beta, dphase_max) of COSTAS_CASES[case_index]"""
    bw, damping, dd, offset, snr = COSTAS_CASES[case_index]
    return (COSTAS_DD if dd else COSTAS,) + costas_coefficients(bw, damping)


def pll_mode_coefficients(case_index):
    """-> (mode, alpha, beta, 0) of PLL_CASES[case_index]"""
    kind, coef, freq, snr = PLL_CASES[case_index]
    if kind == "P":
        return PLL_P, R(coef), 0.0, 0.0
    return (PLL_PI,) + pll_pi_coefficients(coef) + (0.0,)


_cache = {}


def model_costas(case_index):
    """the model's outputs on the committed input, computed once per session (read-only arrays)"""
    key = ("c", case_index)
    if key not in _cache:
        mode, a, b, dm = costas_mode_coefficients(case_index)
        r, st = costas(costas_input(case_index), a, b, dm, mode == COSTAS_DD)
        for v in r.values():
            v.flags.writeable = False
        _cache[key] = (r, st)
    return _cache[key]


def model_pll(case_index):
    key = ("p", case_index)
    if key not in _cache:
        mode, a, b, _ = pll_mode_coefficients(case_index)
        r, st = pll(pll_input(case_index), mode == PLL_PI, a, b)
        for v in r.values():
            v.flags.writeable = False
        _cache[key] = (r, st)
    return _cache[key]


# ------------------------------------------------------------------ one ctypes driver for the reference library and the drop-in library
class CostasState(C.Structure):             # bpsk_costas_loop_state_t (libcsdr.h:364-374)
    _fields_ = [("alpha", C.c_float), ("beta", C.c_float), ("decision_directed", C.c_int), ("current_freq", C.c_float), ("dphase", C.c_float),
                ("nco_phase", C.c_float), ("dphase_max", C.c_float), ("dphase_max_reset_to_zero", C.c_int)]


class PllState(C.Structure):                # pll_t (libcsdr.h:298-308)
    _fields_ = [("pll_type", C.c_int), ("output_phase", C.c_float), ("dphase", C.c_float), ("frequency", C.c_float), ("alpha", C.c_float),
                ("beta", C.c_float), ("iir_temp", C.c_float)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def bind(L):
    """prototypes of the five functions on a library that exports the reference's names"""
    L.init_bpsk_costas_loop_cc.restype = None; L.init_bpsk_costas_loop_cc.argtypes = [C.POINTER(CostasState), C.c_int, C.c_float, C.c_float]
    L.bpsk_costas_loop_cc.restype = None
    L.bpsk_costas_loop_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CostasState)]
    L.pll_cc_init_pi_controller.restype = None; L.pll_cc_init_pi_controller.argtypes = [C.POINTER(PllState), C.c_float, C.c_float, C.c_float, C.c_float]
    L.pll_cc_init_p_controller.restype = None; L.pll_cc_init_p_controller.argtypes = [C.POINTER(PllState), C.c_float]
    L.pll_cc.restype = None; L.pll_cc.argtypes = [C.POINTER(PllState), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return L


def costas_init(L, bandwidth, damping, dd):
    st = CostasState()
    st.decision_directed = int(dd)                  # the init function never stores it (libcsdr.c:2094-2106)
    with _quiet_stderr():
        L.init_bpsk_costas_loop_cc(C.byref(st), int(dd), damping, bandwidth)
    return st


def drive_costas(L, x, bandwidth, damping, dd, block=None, st=None):
    """bpsk_costas_loop_cc block by block (default: one block) from a fresh state (or st) -> (dict of the four outputs, final CostasState)"""
    x = np.ascontiguousarray(x, np.complex64)
    st = st if st is not None else costas_init(L, bandwidth, damping, dd)
    n = x.size; block = block or max(n, 1)
    out = np.zeros(n, np.complex64); nco = np.zeros(n, np.complex64); err = np.zeros(n, f32); dph = np.zeros(n, f32)
    for a in range(0, n, block):
        m = min(block, n - a)
        L.bpsk_costas_loop_cc(_p(x[a:]), _p(out[a:]), m, _p(err[a:]), _p(dph[a:]), _p(nco[a:]), C.byref(st))
    return dict(out=out, error=err, dphase=dph, nco=nco), st


def pll_init(L, kind, coef):
    st = PllState()
    if kind == "P":
        st.pll_type = 1
        L.pll_cc_init_p_controller(C.byref(st), coef)
    else:
        st.pll_type = 2
        L.pll_cc_init_pi_controller(C.byref(st), coef, PLL_KO, PLL_KD, PLL_DAMPING)
    return st


def drive_pll(L, x, kind, coef, block=None, st=None):
    x = np.ascontiguousarray(x, np.complex64)
    st = st if st is not None else pll_init(L, kind, coef)
    n = x.size; block = block or max(n, 1)
    nco = np.zeros(n, np.complex64); dph = np.zeros(n, f32)
    for a in range(0, n, block):
        m = min(block, n - a)
        L.pll_cc(C.byref(st), _p(x[a:]), _p(dph[a:]), _p(nco[a:]), m)
    return dict(dphase=dph, nco=nco), st


class _quiet_stderr:
    """the reference's init function prints its coefficients to stderr: keep the test log clean"""

    def __enter__(self):
        import os
        import sys
        sys.stderr.flush()
        self.keep = os.dup(2); self.null = os.open(os.devnull, os.O_WRONLY); os.dup2(self.null, 2)

    def __exit__(self, *a):
        import os
        os.dup2(self.keep, 2); os.close(self.keep); os.close(self.null)


def maxdev(a, b):
    """largest absolute deviation between two arrays (complex: over both components)"""
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    if np.iscomplexobj(a):
        a = a.view(f32); b = b.view(f32)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if a.size else 0.0


def words_differing(a, b):
    """number of differing 32-bit words"""
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)))
