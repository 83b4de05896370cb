"""What tests/test_wfm_deemph_cpu.py and tests/test_wfm_deemph_gpu.py share: the (tau, audio_rate) pairs, the GPU cases' inputs, the de-emphasis rule restated in
Python, and a CPU model of the chain kernels' fixed warm-up.

The chain kernels cut a call's audio into segments; every segment but the call's first starts its de-emphasis from zero state W samples early.  The segment
geometry of the GPU cases' shape (D 10, 79 taps, F 5, 1024 * 60 samples per stream = 1224 audio samples, 3 streams), read from the code:
  shared rate   wfm_mfma_launch: 306 tiles of 4 samples, one 16-stream group, n_seg = min(CUs, 306 / 24) = 12 wanted -> tiles_per_seg = ceil(ceil(306 / 12) / 6) * 6 = 30:
                segments of 120 samples (11 of them; any GPU with >= 12 CUs), W = 2 steps of 4 * SEQ_TPG = 24 samples = 48
  per stream    a column = lcm(4 D F, 1024) = 25600 input samples = 128 tiles: columns of 512 samples (3 of them), W = 48
  fallback      k_wfm_back: a seam every BK_SEG = 16 samples, W = WARM = 48
  ring          a seam at every block start: 4096 input samples = 81.92 audio samples apart, W = 48
The library reports the three W (csdr_amd_wfm_deemph_warm_samples); the CPU test holds them to the figures above."""
import numpy as np

f32 = np.float32
D, L, F = 10, 79, 5
N = 1024 * 60
S = 3
SHIFT = -0.085
WRATES3 = [-0.085, 0.11, 0.25]                       # = WRATES[:3] of tests/test_rates_gpu.py
# (tau, audio_rate): the default, the US time constant, CD rate, a short tau, and the pairs at which 48 samples of warm-up leave 1e-4 .. 0.37 of the state
TR = [(50e-6, 48000), (75e-6, 48000), (50e-6, 44100), (5e-6, 48000), (50e-6, 96000), (75e-6, 96000), (75e-6, 192000), (1e-3, 48000)]
TR_FALLBACK = [(50e-6, 48000), (75e-6, 48000), (75e-6, 96000), (1e-3, 48000)]
W_CHAIN, W_FALLBACK, W_RING = 48, 48, 48             # what the code warms up over (the CPU test compares them with the library's)
SEG_SHARED, SEG_PS, SEG_FALLBACK = 120, 512, 16      # audio samples between two seams at the shape above
BOUND = 2.0 ** -20


def alpha_b(tau, audio_rate):
    """alpha and b = 1 - alpha in float32, the division 1 / audio_rate in float64 (libcsdr.c:1090-1091)"""
    dt = f32(1.0 / audio_rate)
    alpha = f32(dt / (f32(tau) + dt))
    return alpha, f32(f32(1) - alpha)


def left_over(tau, audio_rate, warm):
    """b^warm in float64: what a seam leaves of the true state"""
    return float(alpha_b(tau, audio_rate)[1]) ** warm


def rule(tau, audio_rate, warm):
    return 1 if left_over(tau, audio_rate, warm) > BOUND else 0


def shared_inputs():
    from tests_helpers import wfm_signal_u8
    return np.stack([wfm_signal_u8(7 + s, N, offset=-SHIFT) for s in range(S)])


def ps_inputs():
    from tests_helpers import wfm_signal_u8
    return np.stack([wfm_signal_u8(2000 + s, N, offset=-WRATES3[s]) for s in range(S)])


_pre = {}


def pre_audio(port, which):
    """the oracle's audio in front of the de-emphasis for the three streams of the shared-rate ('shared') or the per-stream ('ps') cases: computed once"""
    if which not in _pre:
        taps = port.firdes_lowpass_f(L, 0.05)
        u8 = shared_inputs() if which == "shared" else ps_inputs()
        rows = []
        for s in range(S):
            r = SHIFT if which == "shared" else WRATES3[s]
            sh, _ = port.shift_addition_cc(port.convert_u8_f(u8[s]).view(np.complex64), r)
            dem, _ = port.fmdemod_quadri_cf(port.fir_decimate_cc(sh, D, taps))
            rows.append(port.fractional_decimator_ff(dem, float(F)))
        _pre[which] = rows
    return _pre[which]


_want = {}


def oracle_audio(port, which, tau, audio_rate, last=0.0):
    """(s16, float) of the oracle's whole chain per stream, computed once per (inputs, tau, audio_rate, start state) and handed out read-only"""
    key = (which, tau, audio_rate, repr(last))
    if key not in _want:
        out = []
        for a in pre_audio(port, which):
            de, _ = port.deemphasis_wfm_ff(a, tau, audio_rate, last=last)
            s16 = port.convert_f_s16(de)
            de.setflags(write=False); s16.setflags(write=False)
            out.append((s16, de))
        _want[key] = out
    return _want[key]


def recurrence(x, alpha, b, y):
    out = np.empty(x.size, f32)
    for k in range(x.size):
        y = f32(f32(alpha * x[k]) + f32(b * y))
        out[k] = y
    return out


def fixed_warmup(x, tau, audio_rate, seg, warm):
    """the de-emphasis as the chain kernels run it: segment 0 from state 0 (a stream's start), every later segment of `seg` samples from zero state `warm` samples early"""
    alpha, b = alpha_b(tau, audio_rate)
    x = np.asarray(x, f32)
    out = np.empty(x.size, f32)
    for a in range(0, x.size, seg):
        lo = max(0, a - warm) if a else 0
        out[a:a + seg] = recurrence(x[lo:a + seg], alpha, b, f32(0))[a - lo:]
    return out


def to_s16(e):
    """convert_f_s16: truncation of e * 32767 (libcsdr.c:2397)"""
    return np.trunc(np.asarray(e, f32) * f32(32767)).astype(np.int64)


def model_worst_lsb(port, which, tau, audio_rate, seg, warm):
    """worst s16 deviation of the modelled fixed warm-up from the oracle over the three streams"""
    worst = 0
    for a, (s16, _) in zip(pre_audio(port, which), oracle_audio(port, which, tau, audio_rate)):
        d = np.abs(to_s16(fixed_warmup(a, tau, audio_rate, seg, warm)) - s16.astype(np.int64))
        worst = max(worst, int(d.max()))
    return worst
