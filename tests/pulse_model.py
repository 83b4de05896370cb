"""The model of the pulse-shaped symbol modem, in numpy: the transmit stream psk_modulator_u8_c | plain_interpolate_cc I | apply_real_fir_cc in
float32 (the library's order: the nonzero products in ascending tap index, each step one fused multiply-add) and in float64, the per-output gate of a
float32 dot product, the two pulse designs, the slicer in float32 and the bit packers.  A restatement of what libcsdr.c:1731-1765, 1810-1827,
2276-2291 and 2473-2506 compute, not a copy of them."""
import numpy as np

f32 = np.float32
c64 = np.complex64
PI_F = f32(3.14159265358979323846)          # the reference's PI is a float
EPS = 2.0 ** -24                            # half an ulp of 1: the relative error of one float32 rounding


# ------------------------------------------------------------------ float32 fused multiply-add
def fma32(a, b, c):
    """float32(a * b + c) with one rounding, elementwise.  The product of two float32 is exact in float64; its sum with c is rounded to odd in float64
    (the exact sum's error comes from the error-free two-sum), and a value rounded to odd at 53 bits rounds to float32 as the exact value does."""
    a = np.asarray(a, f32).astype(np.float64); b = np.asarray(b, f32).astype(np.float64); c = np.asarray(c, f32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (e != 0) & even
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(f32)


# ------------------------------------------------------------------ symbols
def symbols(n_psk):
    """the 256 symbols of psk_modulator_u8_c: the library's one table (csdr_amd_psk31tx_tables)"""
    import csdr_amd
    return csdr_amd.psk31tx_tables(n_psk, 1)[0]


def stuffed(c, interpolation):
    """plain_interpolate_cc: c[m] at index m * interpolation, zeros between"""
    c = np.atleast_2d(np.asarray(c))
    x = np.zeros((c.shape[0], c.shape[1] * interpolation), c.dtype)
    x[:, ::interpolation] = c
    return x


def n_outputs(n_symbols, interpolation, n_taps):
    return max(0, n_symbols * interpolation - n_taps + 1)


# ------------------------------------------------------------------ the transmit stream
def shape32(c, interpolation, taps):
    """[channels, n] (or [n]) complex symbols -> the stream's outputs 0 .. n I - T in float32.  Output i adds its products c[ceil(i / I) + k] *
    taps[ph + k I], ph = (-i) mod I, in ascending k by fma32, from 0; a phase without a tap gives 0 + 0i."""
    c = np.asarray(c, c64); squeeze = c.ndim == 1
    c = np.atleast_2d(c)
    taps = np.asarray(taps, f32)
    I, T = int(interpolation), taps.size
    n = n_outputs(c.shape[1], I, T)
    i = np.arange(n)
    ph = (-i) % I
    m0 = (i + ph) // I
    K = (T + I - 1) // I
    re = np.zeros((c.shape[0], n), f32); im = np.zeros((c.shape[0], n), f32)
    cr = np.ascontiguousarray(c.real); ci = np.ascontiguousarray(c.imag)
    for k in range(K):
        t = ph + k * I
        on = t < T
        if not on.any():
            break
        w = taps[np.where(on, t, 0)]
        m = np.where(on, m0 + k, 0)
        re = np.where(on, fma32(cr[:, m], w, re), re)
        im = np.where(on, fma32(ci[:, m], w, im), im)
    y = np.empty(re.shape, c64)
    y.real = re; y.imag = im
    return y[0] if squeeze else y


def shape64(c, interpolation, taps):
    """the same stream in float64, and the sum of the magnitudes of every output's products per component: (y, mag_re, mag_im)"""
    c = np.asarray(c, np.complex128); squeeze = c.ndim == 1
    x = stuffed(c, interpolation)
    t = np.asarray(taps, np.float64)
    n = n_outputs(c.shape[-1], interpolation, t.size)
    y = np.zeros((x.shape[0], n), np.complex128); mr = np.zeros((x.shape[0], n)); mi = np.zeros((x.shape[0], n))
    if n:
        for r in range(x.shape[0]):
            y[r] = np.correlate(x[r], t, "valid")
            mr[r] = np.correlate(np.abs(x[r].real), np.abs(t), "valid")
            mi[r] = np.correlate(np.abs(x[r].imag), np.abs(t), "valid")
    return (y[0], mr[0], mi[0]) if squeeze else (y, mr, mi)


def dot_gate(n_terms, mag):
    """the bound of a float32 dot product of n_terms products whose magnitudes add up to mag, against the exact sum: n 2^-24 1.01 mag"""
    return n_terms * EPS * 1.01 * mag


def within(y, want, gate_re, gate_im):
    y = np.asarray(y); want = np.asarray(want)
    return y.shape == want.shape and bool(np.all(np.abs(y.real.astype(np.float64) - want.real) <= gate_re) and
                                          np.all(np.abs(y.imag.astype(np.float64) - want.imag) <= gate_im))


# ------------------------------------------------------------------ designs
def normalize(t):
    """normalize_fir_f: a float32 running sum, a float32 quotient"""
    t = np.asarray(t, f32)
    s = f32(0)
    for v in t:
        s = f32(s + v)
    return (t / s).astype(f32)


def rrc_special_index(sps, beta):
    """the i at which the design takes its closed-form branch: i == sps / (4 beta) compared in float32 (None: no such i)"""
    q = f32(sps) / f32(f32(4) * f32(beta))
    return int(q) if q == np.floor(q) and q >= 1 else None


def firdes_rrc(n_taps, sps, beta):
    """root raised cosine, n_taps odd: float32 where the operands are float32, float64 through sin / cos / sqrt, every tap rounded to float32, normalised"""
    beta = f32(beta); s = f32(sps)
    t = np.zeros(n_taps, f32)
    mid = n_taps // 2
    t[mid] = (f32(1) / s) * (f32(1) + beta * (f32(4) / PI_F - f32(1)))
    for i in range(1, 1 + n_taps // 2):
        if f32(i) == s / (f32(4) * beta):
            a = f32(1) + f32(2) / PI_F; b = f32(1) - f32(2) / PI_F; arg = np.float64(PI_F / (f32(4) * beta))
            v = (np.float64(beta) / (sps * np.sqrt(2.0))) * (np.float64(a) * np.sin(arg) + np.float64(b) * np.cos(arg))
        else:
            r = f32(i) / s
            num = np.sin(np.float64(PI_F * r * (f32(1) - beta))) + np.float64(f32(4) * beta * r) * np.cos(np.float64(PI_F * r * (f32(1) + beta)))
            q = f32(4) * beta * r
            den = PI_F * r * (f32(1) - f32(q * q))
            v = np.float64(f32(1) / s) * num / np.float64(den)
        if mid + i < n_taps:
            t[mid + i] = f32(v)
        t[mid - i] = f32(v)
    return normalize(t)


def firdes_cosine(sps):
    """raised cosine pulse of 2 sps + 1 taps; the two end taps are 0"""
    n = 2 * sps + 1
    t = np.zeros(n, f32)
    mid = n // 2
    for i in range(sps):
        t[mid + i] = t[mid - i] = f32((1 + np.cos(np.float64(PI_F * f32(i) / f32(sps)))) / 2)
    return normalize(t)


# ------------------------------------------------------------------ slicer and packers
def slicer_limits(n_symbols):
    """(lower limits of symbols 1 .. n - 1, upper limits of symbols 0 .. n - 2) in float32: centre -1 + j d, d = float32(2.0 / (n - 1)), limits -/+ d / 2"""
    d = f32(2.0 / (n_symbols - 1))
    j = np.arange(n_symbols).astype(f32)
    center = (f32(-1) + (j * d).astype(f32)).astype(f32)
    half = f32(d / f32(2))
    return (center - half).astype(f32)[1:], (center + half).astype(f32)[:-1]


def _order_key(x):
    """float32 -> int64 with the order of the values (-0 and +0 equal).  Comparing keys does not depend on the processor's treatment of subnormals, which a
    library built with -ffast-math switches to flush-to-zero for the whole process when it is loaded."""
    b = np.asarray(x, f32).view(np.int32).astype(np.int64)
    mag = b & 0x7FFFFFFF
    return np.where(b < 0, -mag, mag)


def slicer(x, n_symbols):
    """the first symbol j whose test holds: j = 0: x < hi[0]; j = n - 1: x >= lo[n - 1]; between: lo[j] <= x < hi[j]; none (NaN, a gap): 0"""
    x = np.asarray(x, f32)
    lo, hi = slicer_limits(n_symbols)
    kx, klo, khi = _order_key(x), _order_key(lo), _order_key(hi)
    nan = (x.view(np.int32) & 0x7FFFFFFF) > 0x7F800000
    out = np.zeros(x.shape, np.uint8); done = nan.copy()
    for j in range(n_symbols):
        if j == 0:
            hit = kx < khi[0]
        elif j == n_symbols - 1:
            hit = kx >= klo[j - 1]
        else:
            hit = (kx >= klo[j - 1]) & (kx < khi[j])
        hit &= ~done
        out[hit] = j; done |= hit
    return out


def pack_1to8(x):
    x = np.asarray(x, np.uint8)
    return ((x[..., None] >> np.arange(8, dtype=np.uint8)) & 1).astype(np.uint8).reshape(x.shape[:-1] + (8 * x.shape[-1],))


def pack_8to1(x):
    x = np.asarray(x, np.uint8)
    g = (x.reshape(x.shape[:-1] + (x.shape[-1] // 8, 8)) != 0).astype(np.uint16)
    return (g << np.arange(7, -1, -1, dtype=np.uint16)).sum(-1).astype(np.uint8)
