"""Float64 reference of the fused u8 front end convert_u8_f | shift_addition_cc | fir_decimate_cc (csdr_amd_ddc_*, csdr_amd/csrc/ddc_mfma.hip), its
per-sample error gate, and a transcription of the host dispatch (ddc_process_fused), the way fir_reference.py does it for fir.hip.

Reference.   y64[k] = sum_t h[t] R[D k + t] x[D k + t],   n_out = (n - L) // D + 1
    x   the oracle's convert_u8_f widened to float64 (the kernel's exact (2 v - 255) / 255 differs by at most u |x| per term: inside the kappa term),
    R   the oracle's own float32 phasor sequence, shift_addition_cc applied to ones in the stream model's 1024-sample chunks ((1 + 0j) R is exact in
        float32, test_ddc_reference_cpu.py asserts it), widened to float64; a retune changes the rate at a sample and keeps the phase,
    sum in float64, in chunks (fir_reference._corr).

Gate, per output and per component, with the condition sum c_k = sum_t |h[t]| (|Re x| + |Im x|) of both components (|R| = 1):

    |y - y64| <= kappa(L) u c_k + rho(rate) c_k + Q_k

kappa(L) u c_k is fir_reference's bound of a float32 sum of L products in any order.

Q_k, weight quantisation.  ddc_build_table rounds the weights a h[t] d^ts (a = 2/255, two real weights per tap and row) to multiples of
    q = 2^-22 a max|h| 1.0001 max(1, |d|^(7 D + L))
and multiplies them with the exact integers v - 128; the +0.5 of u8 -> float goes through unquantised prefix sums.  lrint errs by at most q/2 per weight, so
a row's error is at most q/2 S1_k, S1_k = sum |v - 128| over the 2 L bytes of the window; the roundings are independent, so its standard deviation is
q / sqrt(12) S2_k, S2_k = sqrt(sum (v - 128)^2).  (The post factor of modulus 1 turns the (Re, Im) row pair: the variance is unchanged.)
    Q_k = min(q/2 S1_k, 6 q / sqrt(12) S2_k)
For fir_reference.random_taps (|h| >= max|h| / 4) the first form is at most 8 u c_k; the second is what counts for designed lowpass taps and constant rows,
where a few large centre taps set q and the hard bound is loose.

rho(rate), the rotator.  The kernel does not replay the reference's float32 recurrence: it models R[n] = C_m d^(n mod 1024) (C_m: the float (cos, sin) of
chunk m's starting phase, d: the float (cos, sin) of the phase step as a complex double) and, for rates whose recurrence drifts (RMS deviation over a
chunk > 2e-6, ddc_rotator_model_rms), corrects the model with a table of one value per 32-sample granule: k_ddc_direct looks every tap's granule up, the
shared-rate k_ddc_mfma one granule per output and K-range part (the centre of the output's taps there; the rest of that stretch is inside the kappa term), the
per-stream k_ddc_mfma one per K-range part, which is why it only runs drifting streams from 100 taps on.  rho is measured on the reference's own R:
    chunk_peak   = max_n |R[n] - R[1024 floor(n / 1024)] d^(n mod 1024)|
    granule_peak = the same about each granule's centre 32 j + 16
    rho = chunk_peak if chunk_peak <= 4e-6 else granule_peak + 2 u
A rate that the library corrects although rho assumed the chunk model only makes the kernel more accurate than the gate allows for.

Every output is gated, none is excluded; where c_k = 0 the result must be exact (no byte converts to 0, so this never happens on u8 input)."""
import math
import numpy as np

import fir_reference as fr

f32, c64 = np.float32, np.complex64
U = fr.U
PI_F = f32(3.14159265358979323846)
RHO_SWITCH = 4e-6
# the rates the gate has been measured for: each sits clear of the library's switch (2e-6 RMS over a chunk) on one side or the other
RATES_CHUNK = (0.11, -0.4321, -0.085, 0.3, -0.2718, 0.499)       # chunk model: chunk peak <= 4e-6
RATES_DRIFT = (0.05, 0.2, 0.25, 1e-4)                            # corrected per granule: chunk peak 7e-6 .. 3e-5

# the shapes the GPU tests run (test_ddc_shapes_gpu.py) and the self-check covers: (D, L of random taps, odd L of designed lowpass taps or None, rate)
SHAPES = [
    (2, 1025, 1025, 0.05),      # smallest D, longest history; drifting rate on a two-team shape
    (16, 255, None, -0.4321),   # idle K-range waves, 8-tile period
    (50, 801, None, 0.11),      # anchor: the shape every other test runs
    (64, 704, None, 0.3),       # window limit 1152, 2-tile period
    (80, 592, None, -0.2718),   # last two-team D
    (82, 578, 577, 0.25),       # first one-team D; drifting rate on a one-team shape
    (100, 451, 451, -0.085),    # one team, typical
    (128, 255, None, 0.499),    # one team, 1-tile period
    (164, 4, None, 0.2),        # largest D
]
# a rate per stream: 3 streams, one negative and one drifting rate each
RATE_SHAPES = [
    (16, 255, (0.11, -0.4321, 0.05)),
    (50, 801, (-0.085, 0.25, 0.3)),
    (64, 704, (0.499, -0.2718, 0.2)),
    (100, 451, (0.05, -0.4321, 0.11)),
    (128, 255, (-0.085, 1e-4, 0.3)),
]


def step_phasor(rate):
    """d: shift_addition_init's float (cos, sin) of the phase step (libcsdr_gpl.c:81-89) as a complex double"""
    inc = f32(f32(f32(rate) * f32(2)) * PI_F)
    return complex(float(f32(np.cos(np.float64(inc)))), float(f32(np.sin(np.float64(inc)))))


def phasor_sequence(port, n, plan):
    """R[0..n): the oracle's float32 phasor; plan = [(first sample, rate), ...] (first samples multiples of 1024, the phase carries over)"""
    parts, ph = [], 0.0
    for i, (pos, r) in enumerate(plan):
        end = plan[i + 1][0] if i + 1 < len(plan) else n
        y, ph = port.shift_addition_cc(np.ones(end - pos, c64), r, phase=ph)
        parts.append(y)
    return np.concatenate(parts)


def rotator_rho(R, rate):
    """(rho, chunk peak, granule peak) of one rate measured on a stretch R of the reference's phasor that starts at a chunk boundary"""
    R = np.asarray(R).astype(np.complex128)
    d = step_phasor(rate)
    k = np.arange(R.size)
    chunk = np.abs(R - R[(k >> 10) << 10] * d ** (k & 1023)).max()
    g = np.minimum((k >> 5 << 5) + 16, R.size - 1)
    gran = np.abs(R - R[g] * d ** (k - g).astype(np.float64)).max()
    return (chunk if chunk <= RHO_SWITCH else gran + 2 * U), chunk, gran


def plan_rho(R, plan):
    """the largest rho over the stretches of a plan"""
    n = np.asarray(R).size
    return max(rotator_rho(R[pos:(plan[i + 1][0] if i + 1 < len(plan) else n)], r)[0] for i, (pos, r) in enumerate(plan))


def weight_step(D, L, taps, rate):
    """q of ddc_build_table for one rate"""
    return 2.0 ** -22 * (2.0 / 255.0) * float(np.abs(np.asarray(taps, f32)).max()) * 1.0001 * max(1.0, abs(step_phasor(rate)) ** (7 * D + L))


def reference(port, u8, R, D, taps):
    """(y64 complex128, c, S1, S2) for one stream of u8 IQ bytes and its phasor sequence R"""
    u8 = np.ascontiguousarray(u8, np.uint8)
    h = np.asarray(taps, f32).astype(np.float64)
    x = port.convert_u8_f(u8).astype(np.float64)
    xc = x[0::2] + 1j * x[1::2]
    n = xc.size
    n_out = (n - h.size) // D + 1 if n >= h.size else 0
    z = np.asarray(R).astype(np.complex128)[:n] * xc
    y64 = fr._corr(z.real, h, D, n_out) + 1j * fr._corr(z.imag, h, D, n_out)
    c = fr._corr(np.abs(xc.real) + np.abs(xc.imag), np.abs(h), D, n_out)
    v = u8.astype(np.float64) - 128.0
    one = np.ones(h.size)
    s1 = fr._corr(np.abs(v[0::2]) + np.abs(v[1::2]), one, D, n_out)
    s2 = np.sqrt(fr._corr(v[0::2] ** 2 + v[1::2] ** 2, one, D, n_out))
    return y64, c, s1, s2


def bound(c, s1, s2, L, q, rho):
    """the per-sample gate kappa(L) u c + rho c + Q"""
    return (fr.kappa(L) * U + rho) * c + np.minimum(0.5 * q * s1, 6.0 * q / math.sqrt(12.0) * s2)


def gate_ratio(y, y64, bnd):
    """worst |y - y64| / bound over the outputs and both components: <= 1 passes; an output whose bound is 0 must be exact"""
    y = np.asarray(y).astype(np.complex128)
    err = np.maximum(np.abs(y.real - y64.real), np.abs(y.imag - y64.imag))
    if err.size == 0:
        return 0.0
    if np.any((bnd == 0) & (err != 0)):
        return np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bnd > 0, err / bnd, 0.0).max())


# ------------------------------------------------------------------ test inputs
def fm_clipped_u8(seed, n, offset, amplitude=1.6):
    """a narrow-band FM signal driven into the converter's rails: most bytes are 0 or 255"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    msg = np.sin(2 * np.pi * 1e3 / 2.4e6 * t) + 0.3 * np.convolve(rng.uniform(-1, 1, n + 199), np.ones(200) / 200, "valid")
    sig = amplitude * np.exp(1j * (2 * np.pi * np.cumsum(5e3 / 2.4e6 * msg) + 2 * np.pi * offset * t))
    iq = np.empty(2 * n, f32); iq[0::2] = sig.real; iq[1::2] = sig.imag
    return np.clip(np.round(127.5 * (iq + 1)), 0, 255).astype(np.uint8)


def byte_rows(n, rate, seed):
    """the 19 streams of the shared-rate tests: rows 0-2 uniform random bytes, 3 all 0 (int8 -128 on the matrix cores), 4 all 255, 5 I = 0 / Q = 255,
    6 an FM signal clipped to the rails, 15-18 copies of rows 0-3 (the second, ragged group of 16); the rest random"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 256, (19, 2 * n), dtype=np.uint8)
    rows[3] = 0
    rows[4] = 255
    rows[5, 0::2] = 0; rows[5, 1::2] = 255
    rows[6] = fm_clipped_u8(seed + 1, n, -rate)
    rows[15:19] = rows[0:4]
    return rows


def schedule(D, L):
    """(call sizes, n): calls that are multiples of 1024 samples -- the first with at least 33 tiles, i.e. two segments and a ragged last one, and a partial
    first and last tile --, one call of exactly 1024 samples (k_ddc_direct takes it whole), one more whole call, and a ragged last call; n <= 1024 * 96"""
    first = max(-(-(33 * 8 * D + L) // 1024) * 1024, 2048)
    for _ in range(16):                                    # a last tile that is partial, a last segment shorter than the others and a third call whose first tile is
        tiles = (first - L) // D // 8 + 1                  # partial, where the shape has such a size ((2, 1025) has none: its calls are whole tiles)
        per_seg = -(-tiles // max(min(128, tiles // 16), 1))
        if (first - L) // D % 8 != 7 and tiles % per_seg and ((first + 1024 - L) // D + 1) % 8:
            break
        first += 1024
    else:
        first -= 16 * 1024
    tail = 48 * D + 2 * L + 1024 + 346                     # four whole tiles inside the ragged call, behind the outputs that reach back into the call before
    third = max(2048, -(-(5 * 8 * D + L) // 2048) * 2048)
    if max(first, third) < tail:                           # (the wrapper cuts what follows the listed calls into calls of the largest listed size)
        third = -(-tail // 2048) * 2048
    return [first, 1024, third], first + 1024 + third + tail


# ------------------------------------------------------------------ ddc_process_fused's dispatch, transcribed
def ddc_supported(D, L):
    return 2 <= D <= 224 and D % 2 == 0 and 2 * (7 * D + L) <= 2304 and L - 1 <= 1024


def ddc_instance(D, L, ps, fuse, T, aligned=True, teams=2, B=0, retuned=False, drifting=False):
    """csdr_amd_ddc_last_instance of a call of T samples that starts at stream position B (a multiple of 1024): "k_ddc_mfma<13,NT,FUSE,PS> whole|tiles",
    " + k_ddc_direct" when the plain kernel runs beside it, "k_ddc_direct" alone, "" when the call completes no output.  aligned: input pointer and pitch are
    multiples of 128 bytes; teams: CSDR_AMD_DDC_TEAMS; retuned: a stream of a per-stream object was retuned in front of this call; drifting: one of a per-stream
    object's rates is corrected for drift (with fewer than 100 taps such an object runs on k_ddc_direct: DDC_PS_DRIFT_MIN_TAPS)."""
    k_first = (B - L) // D + 1 if B >= L else 0             # the calls before delivered every k with D k + L <= B
    k_hi = (B + T - L) // D if B + T >= L else -1
    n_out = max(k_hi - k_first + 1, 0)
    if n_out == 0:
        return ""
    ta, tb, whole = 0, -1, False
    ts = 16 * D
    if ddc_supported(D, L) and aligned:
        if T % 512 == 0 and T >= 2048:
            ta, tb, whole = k_first // 8, k_hi // 8, True
            if tb - ta + 1 < 4 or ta * ts - 2 * B < -3072:
                ta, tb, whole = 0, -1, False
        else:
            ta, tb = (k_first + 7) // 8, (k_hi + 1) // 8 - 1
            while ta <= tb and ta * ts - 2 * B < 0:
                ta += 1
            while tb >= ta and ((tb * ts - 2 * B + 2304 + 1023) & ~1023) > 2 * T:
                tb -= 1
            if tb - ta + 1 < 4:
                ta, tb = 0, -1
    if ps and (not whole or (drifting and L < 100)):
        ta, tb, whole = 0, -1, False
    n_fix = min(max(-(-B // D) - k_first, 0), n_out) if (ps and retuned) else 0
    name = ""
    if tb >= ta:
        nt = 2 if (teams == 2 and 3 * 16 * D <= 3842) else 1
        name = "k_ddc_mfma<13,%d,%s,%s> %s" % (nt, "true" if fuse else "false", "true" if ps else "false", "whole" if whole else "tiles")
        n_direct = 0 if whole else (8 * ta - k_first) + (k_hi - 8 * (tb + 1) + 1)
    else:
        n_direct = n_out
    if n_direct > 0 or n_fix > 0:
        name += " + k_ddc_direct" if name else "k_ddc_direct"
    return name


def ddc_instances(D, L, ps, fuse, sizes, n, teams=2, retunes=None, drifting=False):
    """the set of reports of Context.ddc_u8 / nfm_chain over call sizes `sizes` followed by the rest of the n samples in calls of max(sizes)"""
    out, pos, call = set(), 0, 0
    while pos < n:
        T = min(sizes[call] if call < len(sizes) else max(sizes), n - pos)
        out.add(ddc_instance(D, L, ps, fuse, T, True, teams, pos, bool((retunes or {}).get(call)), drifting))
        pos += T; call += 1
    return out
