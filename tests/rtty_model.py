"""Float32 model of the RTTY receive chain (bfsk_demod_cf | serial_line_decoder_f_u8 | rtty_baudot2ascii_u8_u8, and the bit-per-sample
binary_slicer_f_u8 | rtty_line_decoder_u8_u8), a float64 discriminator with its per-sample error gate, and a generator of continuous-phase 2-FSK RTTY.

Cites are to the reference (libcsdr.c / csdr.c).  The serial decoder follows libcsdr.c:1662-1728 literally: data-bit bounds in double, stop-bit bounds
int + float in float then + double, the fit test and samples_used_up_now in float, bit sums sequential in float32."""
import ctypes as C
import math
import os
import numpy as np

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")
U = 2.0 ** -24

# libcsdr.c:1577-1604, indexed by code
LTR = [0, 84, 13, 79, 32, 72, 78, 77, 10, 76, 82, 71, 73, 80, 67, 86, 69, 90, 68, 66, 83, 89, 70, 88, 65, 87, 74, 0, 85, 81, 75, 0]
FIG = [0, 53, 13, 57, 32, 36, 44, 46, 10, 41, 52, 42, 56, 48, 58, 61, 51, 43, 35, 63, 39, 54, 64, 47, 45, 50, 7, 0, 55, 49, 40, 0]
FIGS, LTRS = 0b11011, 0b11111


# ---------------------------------------------------------------- taps and the discriminator
def window_hamming(r):
    x = float(f32(0.5 + float(f32(r)) / 2))
    return float(f32(0.54 - 0.46 * math.cos(float(f32(2 * f32(math.pi) * f32(x))))))


def firdes_peak_c(length, rate):
    """firdes_add_peak_c(taps, length, rate, HAMMING, 0, 1), libcsdr.c:2219-2257, in its float / double arithmetic"""
    middle = length // 2
    phase = f32(0)
    add = f32(-float(f32(rate)) * math.pi * 2)
    t = np.zeros(length, np.complex64)
    for i in range(length):
        w = f32(window_hamming(float(f32(abs(float(f32(f32(middle - i) / f32(middle))))))))
        t[i] = complex(f32(f32(math.cos(float(phase))) * w), f32(f32(math.sin(float(phase))) * w))
        phase = f32(phase + add)
        while float(phase) > 2 * math.pi:
            phase = f32(float(phase) - 2 * math.pi)
        while float(phase) < 0:
            phase = f32(float(phase) + 2 * math.pi)
    s = f32(0)
    for v in t:
        s = f32(float(s) + math.sqrt(float(f32(f32(v.real) * f32(v.real) + f32(v.imag) * f32(v.imag)))))
    return (t.real.astype(f32) / s + 1j * (t.imag.astype(f32) / s)).astype(np.complex64)


def bfsk_taps(spacing, length):
    """csdr.c:3286-3287: (mark at +spacing/2, space at -spacing/2)"""
    return firdes_peak_c(length, f32(spacing) / 2), firdes_peak_c(length, -f32(spacing) / 2)


def corr64(x, h):
    """the valid correlation sum_t x[i + t] h[t] in float64"""
    return np.correlate(np.asarray(x, np.complex128), np.conj(np.asarray(h, np.complex128)), "valid")


def bfsk64(x, mark, space):
    a, b = corr64(x, mark), corr64(x, space)
    return np.abs(a) ** 2 - np.abs(b) ** 2


def bfsk_gate(x, mark, space):
    """per-sample bound on |y - y64| for ANY float32 summation order of the two correlations' 2L products per part (sequential, pairwise or blocked, with or
    without fma), then the power difference in float32.  e_f = gamma_2L * c_f bounds each part's error, c_f = sum_t |x| (|h.re| + |h.im|); a part a, its
    computed square and the sum of two squares add 2 |a| e + e^2 and 2 u of the result; the final difference u |y|."""
    L = len(mark)
    g = 2 * L * U / (1 - 2 * L * U)
    ax = np.abs(np.asarray(x, np.complex128))
    out = 0.0
    for h in (mark, space):
        c = np.correlate(ax, np.abs(h.real).astype(np.float64) + np.abs(h.imag).astype(np.float64), "valid")
        a = np.abs(corr64(x, h))
        e = g * c
        hat = a + math.sqrt(2) * e
        out = out + 2 * math.sqrt(2) * a * e + 2 * e * e + 3 * U * hat * hat
    y = np.abs(bfsk64(x, mark, space))
    return 1.01 * (out + U * (y + out))


def bfsk32_seq(x, mark, space, pairwise=False):
    """the discriminator with float32 sums: each part's 2L products summed sequentially (or pairwise), then the reference's epilogue"""
    x = np.asarray(x, np.complex64)
    L = len(mark)
    n = len(x) - L + 1
    if n <= 0:
        return np.zeros(0, f32)
    idx = np.arange(n)[:, None] + np.arange(L)[None, :]
    W = x[idx]
    xr, xi = W.real.astype(f32), W.imag.astype(f32)
    parts = []
    for h, sgn in ((mark, 0), (mark, 1), (space, 0), (space, 1)):
        hr, hi = h.real.astype(f32), h.imag.astype(f32)
        if sgn == 0:
            p = np.stack([xr * hr, xi * (-hi)], axis=2).reshape(n, 2 * L)
        else:
            p = np.stack([xr * hi, xi * hr], axis=2).reshape(n, 2 * L)
        if pairwise:
            while p.shape[1] > 1:
                if p.shape[1] & 1:
                    p = np.concatenate([p, np.zeros((n, 1), f32)], axis=1)
                p = (p[:, 0::2] + p[:, 1::2]).astype(f32)
            parts.append(p[:, 0])
        else:
            parts.append(np.cumsum(p, axis=1, dtype=f32)[:, -1])
    mr, mi, sr, si = parts
    return (-(sr * sr + si * si) + (mr * mr + mi * mi)).astype(f32)


# ---------------------------------------------------------------- the serial decoder (libcsdr.c:1662-1728)
def serial_window(x, spb, databits=8, stopbits=1.0, ratio=0.4):
    """one library call on the window x -> (list of shr, input_used)"""
    spb, stopbits, ratio = f32(spb), f32(stopbits), f32(ratio)
    all_bits = f32(f32(1 + databits) + stopbits)
    x = np.asarray(x, f32)
    n = len(x)
    off, used, out = 0, 0, []
    lo, hi = 0.5 * float(f32(1 - ratio)), 0.5 * float(f32(1 + ratio))
    slo, shi = float(stopbits) * 0.5 * float(f32(1 - ratio)), float(stopbits) * 0.5 * float(f32(1 + ratio))
    while True:
        w = x[off:off + n]
        e = np.nonzero((w[1:] < 0) & (w[:-1] > 0))[0]
        if e.size == 0:
            return out, used + max(n, 1)
        ss = int(e[0]) + 1
        if f32(f32(ss) + f32(spb * all_bits)) >= f32(n):
            return out, used + max(0, ss - 2)
        shr = 0
        for di in range(databits):
            a = int(ss + (float(1 + di) + lo) * float(spb))
            b = int(ss + (float(1 + di) + hi) * float(spb))
            acc = np.cumsum(w[a:b], dtype=f32)[-1] if b > a else f32(0)
            shr = (shr << 1) | int(acc > 0)
        sb = f32(f32(ss) + f32(f32(1 + databits) * spb))
        a = int(float(sb) + slo * float(spb))
        b = int(float(sb) + shi * float(spb))
        acc = np.cumsum(w[a:b], dtype=f32)[-1] if b > a else f32(0)
        if acc < 0:
            return out, used + min(ss + 1, n)
        out.append(shr)
        u = f32(f32(ss) + f32(all_bits * spb))
        now = int(f32(n) if u > f32(n) else u)
        used += now
        off += now
        n -= now
        if n == 0:
            return out, used


def serial_stream(x, spb, databits=8, stopbits=1.0, B=16384, ratio=0.4):
    """the CLI's bigbufs loop (csdr.c:2511-2524) over whole windows of B samples; no stale window at the end"""
    x = np.asarray(x, f32)
    pos, out = 0, []
    while len(x) - pos >= B:
        o, used = serial_window(x[pos:pos + B], spb, databits, stopbits, ratio)
        assert used > 0
        out += o
        pos += used
    return out


def baudot(codes, fig=0):
    """rtty_baudot2ascii_u8_u8 (csdr.c:2461-2473): NULs left out"""
    out = []
    for c in codes:
        c &= 255
        if c == FIGS:
            fig = 1
        elif c == LTRS:
            fig = 0
        elif c < 32:
            ch = (FIG if fig else LTR)[c]
            if ch:
                out.append(ch)
    return bytes(out)


def line_decoder(bits):
    """rtty_line_decoder_u8_u8 (csdr.c:2446-2458 / libcsdr.c:1615-1655) from a fresh decoder"""
    state, rec, shr, cnt, fig, out = 0, 0, 0, 0, 0, []
    for b in bits:
        b = 1 if b else 0
        if state == 0:
            if b == 1:
                state = 1
                if rec:
                    c = shr & 31
                    if c == FIGS:
                        fig = 1
                    elif c == LTRS:
                        fig = 0
                    else:
                        ch = (FIG if fig else LTR)[c]
                        if ch:
                            out.append(ch)
            else:
                rec = 0
        elif state == 1:
            rec = 0
            if b == 0:
                state, shr, cnt = 2, 0, 0
        else:
            shr = ((shr << 1) | b) & 0xFFFF
            cnt += 1
            if cnt == 5:
                state, rec = 0, 1
    return bytes(out)


def chain(x, spacing=0.02125, L=101, spb=176.0176, databits=5, stopbits=1.5, B=16384):
    """bfsk (float32, sequential sums) | serial | Baudot"""
    m, s = bfsk_taps(spacing, L)
    return baudot(serial_stream(bfsk32_seq(x, m, s), spb, databits, stopbits, B))


# ---------------------------------------------------------------- the generator
def encode(text):
    """ASCII -> Baudot codes with LTRS / FIGS shifts (letters first)"""
    codes, fig = [LTRS], 0
    for ch in text.upper():
        o = ord(ch)
        if o in (10, 13, 32):
            codes.append(LTR.index(o))
        elif o in LTR:
            if fig:
                codes.append(LTRS)
                fig = 0
            codes.append(LTR.index(o))
        elif o in FIG:
            if not fig:
                codes.append(FIGS)
                fig = 1
            codes.append(FIG.index(o))
    return codes


def rtty_signal(text, spb=176.0176, spacing=0.02125, stopbits=1.5, amplitude=0.5, carrier=0.0, bit_phase=0.0, snr_db=None, lead=2000, tail=0, seed=0, gap=1.0):
    """continuous-phase 2-FSK: idle mark, then per character 1 start bit (space), 5 data bits MSB first (the decoder's shift order), stopbits of mark
    and `gap` bits of idle mark (the reference consumes a character up to the end of its stop bits, so back-to-back characters lose every other start edge);
    mark = +spacing/2, space = -spacing/2 (plus carrier), in cycles per sample.  snr_db: complex Gaussian noise against the carrier power."""
    bits = []
    for c in encode(text):
        bits.append((0, 1.0))
        bits += [((c >> (4 - k)) & 1, 1.0) for k in range(5)]
        bits.append((1, stopbits + gap))
    t0 = lead + bit_phase * spb
    edges, level, pos = [0.0], [1], t0
    edges.append(t0)
    for b, length in bits:
        level.append(b)
        pos += length * spb
        edges.append(pos)
    level.append(1)
    n = int(math.ceil(pos)) + tail
    edges.append(float(n))
    freq = np.empty(n)
    bnd = [int(round(e)) for e in edges]
    for k, lv in enumerate(level):
        freq[bnd[k]:bnd[k + 1]] = carrier + (spacing / 2 if lv else -spacing / 2)
    ph = 2 * np.pi * np.concatenate([[0.0], np.cumsum(freq[:-1])])
    x = amplitude * np.exp(1j * ph)
    if snr_db is not None:
        rng = np.random.default_rng(seed)
        sd = amplitude / math.sqrt(2) * 10 ** (-snr_db / 20)
        x = x + sd * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


# ---------------------------------------------------------------- the reference library through ctypes
class SerialLine(C.Structure):              # serial_line_t (libcsdr.h:276-284)
    _fields_ = [("samples_per_bits", C.c_float), ("databits", C.c_int), ("stopbits", C.c_float), ("output_size", C.c_int), ("input_used", C.c_int),
                ("bit_sampling_width_ratio", C.c_float)]


class BaudotDecoder(C.Structure):           # rtty_baudot_decoder_t (libcsdr.h:252-259)
    _fields_ = [("fig_mode", C.c_ubyte), ("character_received", C.c_ubyte), ("shr", C.c_ushort), ("bit_cntr", C.c_ubyte), ("state", C.c_int)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ref_lib():
    if not os.path.exists(REF_LIB):
        return None
    L = C.CDLL(REF_LIB)
    L.bfsk_demod_cf.restype = C.c_int
    L.bfsk_demod_cf.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.firdes_add_peak_c.restype = None
    L.firdes_add_peak_c.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int]
    L.serial_line_decoder_f_u8.restype = None
    L.serial_line_decoder_f_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.binary_slicer_f_u8.restype = None
    L.binary_slicer_f_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.rtty_baudot_decoder_lookup.restype = C.c_char
    L.rtty_baudot_decoder_lookup.argtypes = [C.c_void_p, C.c_ubyte]
    L.rtty_baudot_decoder_push.restype = C.c_char
    L.rtty_baudot_decoder_push.argtypes = [C.c_void_p, C.c_ubyte]
    return L


def ref_peak(L, length, rate):
    t = np.zeros(length, np.complex64)
    L.firdes_add_peak_c(_p(t), length, f32(rate), 2, 0, 1)
    return t


def ref_bfsk(L, x, mark, space):
    x = np.ascontiguousarray(x, np.complex64)
    n = len(x) - len(mark) + 1
    y = np.zeros(max(n, 1), f32)
    k = L.bfsk_demod_cf(_p(x), _p(y), len(x), _p(np.ascontiguousarray(mark)), _p(np.ascontiguousarray(space)), len(mark))
    return y[:max(k, 0)]


def ref_serial_window(L, x, spb, databits=8, stopbits=1.0, ratio=0.4):
    x = np.ascontiguousarray(x, f32)
    s = SerialLine(f32(spb), databits, f32(stopbits), 0, 0, f32(ratio))
    out = np.zeros(len(x) + 16, np.uint32 if databits > 16 else (np.uint16 if databits > 8 else np.uint8))
    L.serial_line_decoder_f_u8(C.byref(s), _p(x), _p(out), len(x))
    return [int(v) for v in out[:s.output_size]], s.input_used


def ref_serial_stream(L, x, spb, databits=8, stopbits=1.0, B=16384):
    x = np.asarray(x, f32)
    pos, out = 0, []
    while len(x) - pos >= B:
        o, used = ref_serial_window(L, x[pos:pos + B], spb, databits, stopbits)
        assert used > 0
        out += o
        pos += used
    return out


def ref_chain(L, x, spacing=0.02125, length=101, spb=176.0176, databits=5, stopbits=1.5, B=16384):
    m, s = ref_peak(L, length, f32(spacing) / 2), ref_peak(L, length, -f32(spacing) / 2)
    codes = ref_serial_stream(L, ref_bfsk(L, x, m, s), spb, databits, stopbits, B)
    fig = C.c_ubyte(0)
    out = []
    for c in codes:
        r = L.rtty_baudot_decoder_lookup(C.byref(fig), c)[0]
        if r:
            out.append(r)
    return bytes(out)
