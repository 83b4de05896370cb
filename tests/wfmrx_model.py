"""What the WFM receive bank's tests share (csdr_amd_wfmrx, csdr_amd/csrc/wfmrx.hip): the inputs, the expected values, the framing rule and the gates.

Inputs are complex baseband at the decimator's input rate, one kind per channel (KINDS, channel k gets KINDS[k % 4]):
  fm       constant-envelope FM: amplitude 0.7, two tones, peak deviation 0.08 cycles per sample, additive complex noise of sigma 0.002.  |demodulated| stays
           below 0.21 (Kf * 2 pi * 0.08 = 0.171 plus the noise), so convert_f_s16 never overflows
  zeros    the same with two runs of exact (0, 0) samples, ZERO_RUNS: the demodulator's `den == 0` branch.  The first run crosses sample 341 (the first cut of
           the tests' ragged calls), the second sample 1024 (the end of the first window, and of a first call of exactly one window)
  allzero  every sample (0, 0)
  weak     the fm signal, noise included, scaled to amplitude 1e-3
There is no pure-noise channel: the quadrature demodulator is ill-conditioned where I^2 + Q^2 -> 0.

Expected values: the oracle's stages in turn, port.fmdemod_quadri_cf, fractional_decimator_ff(rate, P, taps, bufsize=W), deemphasis_wfm_ff(tau, audio_rate),
convert_f_s16.  Gates: float audio relrms <= 1e-5 (the project's standing gate for float paths); no s16 sample more than 1 LSB from the oracle's and fewer than
1 % of them 1 LSB apart."""
import ctypes as C
import functools

import numpy as np

c64 = np.complex64
f32 = np.float32

KINDS = ("fm", "zeros", "allzero", "weak")
ZERO_RUNS = ((300, 400), (1000, 1100))
W = 1024
TAU, AUDIO_RATE = 50e-6, 48000
TOL = 1e-5
S16_FRACTION = 0.01
KF = f32(0.340447550238101026565118445432744920253753662109375)


def fm_baseband(rng, n, dev=0.08):
    t = np.arange(n)
    msg = 0.6 * np.sin(2 * np.pi * 0.004 * t) + 0.4 * np.sin(2 * np.pi * 0.0171 * t + 1.0)      # |msg| <= 1: the peak deviation is dev
    ph = 2 * np.pi * np.cumsum(dev * msg)
    return 0.7 * np.exp(1j * ph) + 0.002 * (rng.normal(size=n) + 1j * rng.normal(size=n))


def channel(kind, seed, n):
    """one channel of `kind`, n samples, complex64"""
    rng = np.random.default_rng(seed)
    x = fm_baseband(rng, n)
    if kind == "zeros":
        for a, b in ZERO_RUNS:
            x[a:b] = 0
    if kind == "allzero":
        x[:] = 0
    if kind == "weak":
        x *= 1e-3 / 0.7
    return x.astype(c64)


def make_input(n_channels, n, seed=0):
    """[n_channels, n] complex64, channel k of kind KINDS[k % 4]"""
    return np.stack([channel(KINDS[k % len(KINDS)], 9000 + 131 * seed + k, n) for k in range(n_channels)])


def prefilter_taps(rate, transition_bw=0.03):
    """the taps `csdr fractional_decimator_ff <rate> <P> --prefilter` designs (csdr.c:1506-1509), by the library's host functions (no GPU)"""
    import csdr_amd
    L = csdr_amd.lib()
    L.csdr_amd_firdes_filter_len.argtypes = [C.c_float]
    L.csdr_amd_firdes_lowpass_f.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int]
    n = L.csdr_amd_firdes_filter_len(transition_bw)
    taps = np.zeros(n, f32)
    L.csdr_amd_firdes_lowpass_f(taps.ctypes.data, n, float(f32(0.5) / (f32(rate) - f32(transition_bw))), 2)      # CSDR_WINDOW_HAMMING
    return taps


@functools.lru_cache(maxsize=None)
def window_call(rate, P, taps_length, window, where):
    """one call of fractional_decimator_ff on a window (libcsdr.c:763, 790-791), positions only -> (outputs, where afterwards, input_processed)"""
    rate, where = f32(rate), f32(where)
    n_out = 0
    while True:
        hi = int(np.ceil(where))
        if not hi + P + taps_length < window:
            break
        n_out += 1
        where = f32(where + rate)
    processed = hi - 1 + (-(P // 2) + 1)
    return n_out, float(f32(where - f32(processed))), processed


def plan(rate, P, taps_length, window, where, held, n_in):
    """csdr_amd_wfmrx_plan restated: the reference's position bookkeeping over the windows of csdr.c:1513-1524: a window is run once `window` samples from the
    first unprocessed one are there -> (samples written per channel, where afterwards, samples held afterwards)"""
    where = float(f32(where))
    if not n_in:
        return 0, where, held                                            # (a call without input does nothing)
    total, base, n_out = held + n_in, 0, 0
    while base + window <= total:
        k, where, processed = window_call(float(f32(rate)), P, taps_length, window, where)
        n_out += k
        if processed <= 0:
            break
        base += processed
    return n_out, where, total - base


def fresh_where(P):
    return float(P // 2 - 1)


def demod_rcp_model(x):
    """the kernels' demodulator on the host in float32 steps: Kf * num times a reciprocal of den that is correctly rounded (the Newton-refined v_rcp_f32 is within
    an ulp of it), where the oracle divides in double and rounds once"""
    x = np.ascontiguousarray(x, c64)
    p = np.concatenate([np.zeros(1, c64), x[:-1]])
    xi, xq, pi, pq = (a.astype(f32) for a in (x.real, x.imag, p.real, p.imag))
    num = (xi * (xq - pq)).astype(f32) - (xq * (xi - pi)).astype(f32)
    den = (xi * xi).astype(f32) + (xq * xq).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        rd = (f32(1) / den).astype(f32)
        v = ((KF * num).astype(f32) * rd).astype(f32)
    return np.where(den != 0, v, f32(0)).astype(f32)


def tail(port, dem, rate, P=12, taps=None, window=W, tau=TAU, audio_rate=AUDIO_RATE):
    """the oracle's decimator, de-emphasis and conversion behind demodulated samples -> (s16, float audio)"""
    a = port.fractional_decimator_ff(dem, rate, P, taps, bufsize=window)
    e, _ = port.deemphasis_wfm_ff(a, tau, audio_rate)
    return port.convert_f_s16(e), e


def expected(port, x, rate, P=12, taps=None, window=W, tau=TAU, audio_rate=AUDIO_RATE):
    """the oracle's chain on one channel -> (s16, float audio)"""
    dem, _ = port.fmdemod_quadri_cf(x)
    return tail(port, dem, rate, P, taps, window, tau, audio_rate)


def gate_figures(s16, af, want_s16, want_af):
    """(relrms of the float audio, largest s16 difference, fraction of s16 samples that differ); the lengths are asserted here"""
    from oracle import relrms
    assert af.shape == want_af.shape and s16.shape == want_s16.shape, (af.shape, want_af.shape)
    assert want_af.size > 0
    d = np.abs(s16.astype(np.int32) - want_s16.astype(np.int32))
    return relrms(af, want_af), int(d.max()), float((d > 0).mean())


def assert_gates(s16, af, want_s16, want_af, what=""):
    r, dmax, frac = gate_figures(s16, af, want_s16, want_af)
    print("%s: relrms %.3g, s16 max diff %d, differing %.4f %%" % (what, r, dmax, 100 * frac))
    assert r <= TOL, (what, r)
    assert dmax <= 1 and frac < S16_FRACTION, (what, dmax, frac)


def bank_composition(ctx, x, tbw, decimation, rates, per, frac_rate, retunes=None, resets=None):
    """ctx.fastddc_bank -> WfmRx with `per` blocks per call; retunes {call: [(channel, rate), ...]} and resets {call: [channel, ...]} are applied in front of that
    call -> (the s16 audio of every call, [n_channels, count] each; the bank's rows; the channelizer's per-call counts)"""
    import csdr_amd
    y = ctx.fastddc_bank(x, tbw, decimation, rates, blocks_per_call=per, retunes=retunes)
    assert all(np.all(c == c[0]) for c in ctx.ddc_call_counts)           # the channelizer's counts do not depend on the rate
    counts = [int(c[0]) for c in ctx.ddc_call_counts]
    out, at = [], 0
    with csdr_amd.WfmRx(ctx, len(rates), rate=frac_rate, max_samples_per_call=max(counts)) as o:
        for call, k in enumerate(counts):
            for ch in (resets or {}).get(call, []):
                o.reset_channel(ch)
            out.append(o.process(np.stack([row[at:at + k] for row in y]))[0])
            at += k
    return out, y, counts


if __name__ == "__main__":
    # python wfmrx_model.py <in.npz> <out.npz>: bank_composition in a process of its own.  The channelizer's small geometries transform with hipFFT, and a process
    # that has imported torch resolves hipFFT to the copy torch ships, whose last bits differ from those of the system's copy the `csdr` binary links: a
    # composition that is to equal the command byte for byte runs with CSDR_AMD_NO_TORCH_PRELOAD=1, on the same library.
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import csdr_amd
    a = np.load(sys.argv[1])
    c = csdr_amd.Context(0)
    args = (c, a["x"], float(a["tbw"]), int(a["decimation"]), [float(r) for r in a["rates"]], int(a["per"]), float(a["frac_rate"]))
    lines, _, _ = bank_composition(*args, retunes={1: [(int(a["retune_channel"]), float(a["retune_rate"]))]}, resets={1: [int(a["reset_channel"])]})
    plain, _, _ = bank_composition(*args)
    np.savez(sys.argv[2], first=lines[0], second=lines[1], plain=np.concatenate(plain, axis=1), torch_loaded="torch" in sys.modules)
    c.close()
