"""Float32 model of the BPSK31 receive chain (libcsdr.c: simple_agc_cc 2201-2217, timing_recovery_cc 1977-2075, dbpsk_decoder_c_u8 2319-2333,
psk31_varicode_decoder_push 1536-1549) and a PSK31 signal generator for the tests.

The model keeps C's order of float32 operations with IEEE sqrt and division.  Where the reference's -ffast-math build reordered harmlessly, it follows
the compiled order: correction_offset = (int)((error * loop_gain) * (float)(D/2 * sign)).  atan2 is taken in double and rounded to float, as the
reference does on float inputs."""
import math
import numpy as np

f32 = np.float32
PI = f32(math.pi)
GARDNER, EARLYLATE = 0, 1

# The PSK31 varicode (G3PLX) for characters 0..127, as bit strings
VARICODE = [
    "1010101011", "1011011011", "1011101101", "1101110111", "1011101011", "1101011111", "1011101111", "1011111101",
    "1011111111", "11101111", "11101", "1101101111", "1011011101", "11111", "1101110101", "1110101011",
    "1011110111", "1011110101", "1110101101", "1110101111", "1101011011", "1101101011", "1101101101", "1101010111",
    "1101111011", "1101111101", "1110110111", "1101010101", "1101011101", "1110111011", "1011111011", "1101111111",
    "1", "111111111", "101011111", "111110101", "111011011", "1011010101", "1010111011", "101111111",
    "11111011", "11110111", "101101111", "111011111", "1110101", "110101", "1010111", "110101111",
    "10110111", "10111101", "11101101", "11111111", "101110111", "101011011", "101101011", "110101101",
    "110101011", "110110111", "11110101", "110111101", "111101101", "1010101", "111010111", "1010101111",
    "1010111101", "1111101", "11101011", "10101101", "10110101", "1110111", "11011011", "11111101",
    "101010101", "1111111", "111111101", "101111101", "11010111", "10111011", "11011101", "10101011",
    "11010101", "111011101", "10101111", "1101111", "1101101", "101010111", "110110101", "101011101",
    "101110101", "101111011", "1010101101", "111110111", "111101111", "111111011", "1010111111", "101101101",
    "1011011111", "1011", "1011111", "101111", "101101", "11", "111101", "1011011",
    "101011", "1101", "111101011", "10111111", "11011", "111011", "1111", "111",
    "111111", "110111111", "10101", "10111", "101", "110111", "1111011", "1101011",
    "11011111", "1011101", "111010101", "1010110111", "110111011", "1010110101", "1011010111", "1110110101",
]


# ------------------------------------------------------------------ receive chain
def agc(x, rate, reference=1.0, max_gain=65535.0, gain=1.0):
    """simple_agc_cc: x complex64 -> (output complex64, gain after the last sample)"""
    x = np.asarray(x, np.complex64)
    i = x.real.astype(f32); q = x.imag.astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        amp = np.sqrt(i * i + q * q)
        ideal = f32(reference) / amp
    ideal = np.where(ideal > f32(max_gain), f32(max_gain), ideal).astype(f32)
    ideal = np.where(ideal <= 0, f32(0), ideal).astype(f32)
    rate = f32(rate); r1 = f32(1) - rate
    g = f32(gain)
    gs = np.empty(x.size, f32)
    for k, d in enumerate(ideal.tolist()):
        g = (f32(d) - g) * rate + g * r1
        gs[k] = g
    out = np.empty(x.size, np.complex64)
    out.real = gs * i; out.imag = gs * q
    return out, g


def timing(x, algorithm, decimation, loop_gain=0.5, max_error=2.0, use_q=False, correction_offset=0):
    """one timing_recovery_cc call over the whole of x -> (symbols, errors (unclamped), indexes, input_processed, last_correction_offset)"""
    x = np.asarray(x, np.complex64)
    xi = x.real.astype(f32).tolist(); xq = x.imag.astype(f32).tolist()
    n = x.size
    D = decimation; hb = D // 2; qb = D // 4; wing = int(f32(D) * f32(0.25))
    sign = -1 if algorithm == GARDNER else 1
    hbs = f32(hb * sign); lg = f32(loop_gain); me = f32(max_error)
    cbi, corr = 0, int(correction_offset)
    syms, errs, idxs = [], [], []
    while cbi + hb * 3 < n:
        if corr <= -qb * 0.9 or corr >= 0.9 * qb:
            corr = 0
        if algorithm == EARLYLATE:
            pr, pl, pm = cbi + wing * 3, cbi + wing - corr, cbi + hb
            po = pm
        else:
            pr, pl, pm = cbi + hb * 3, cbi + hb, cbi + hb * 2
            po = pl
        syms.append(complex(xi[po], xq[po])); idxs.append(po)
        e = (f32(xi[pr]) - f32(xi[pl])) * f32(xi[pm])
        if use_q:
            e = e + (f32(xq[pr]) - f32(xq[pl])) * f32(xq[pm])
            e = e / f32(2)
        errs.append(e)
        if e > me:
            e = me
        if e < -me:
            e = -me
        corr = int((e * lg) * hbs)
        cbi += D + corr
    return np.array(syms, np.complex64), np.array(errs, f32), np.array(idxs, np.int64), cbi, corr


def dbpsk(symbols, last=0j):
    """dbpsk_decoder_c_u8 from last_input `last` -> bits uint8"""
    s = np.asarray(symbols, np.complex64)
    ph = [f32(math.atan2(float(v.imag), float(v.real))) for v in s]
    lp = f32(math.atan2(float(f32(np.imag(last))), float(f32(np.real(last)))))
    out = np.empty(len(ph), np.uint8)
    for k, p in enumerate(ph):
        d = p - lp
        while d < -PI:
            d = d + f32(2) * PI
        while d >= PI:
            d = d - f32(2) * PI
        out[k] = 0 if (d > PI / f32(2) or d < -PI / f32(2)) else 1
        lp = p
    return out


_MASK64 = (1 << 64) - 1
_TABLE = [(int(c, 2), len(c), a) for a, c in enumerate(VARICODE)]


def varicode_push(shr, bit):
    """psk31_varicode_decoder_push, the reference's table scan -> (shr, character or 0)"""
    shr = ((shr << 1) | (1 if bit else 0)) & _MASK64
    for code, bc, a in _TABLE:
        if (code << 2) == shr & ((1 << ((bc + 4) & 63)) - 1):
            return shr, a
    return shr, 0


def varicode_decode(bits, shr=0):
    """psk31_varicode_decoder_u8_u8 -> (bytes of the decoded characters, NUL left out, shr)"""
    out = bytearray()
    for b in np.asarray(bits).tolist():
        shr, c = varicode_push(shr, b)
        if c:
            out.append(c)
    return bytes(out), shr


def chain(x, rate=0.001, reference=0.5, max_gain=65535.0, algorithm=GARDNER, decimation=256, loop_gain=0.5, max_error=2.0, use_q=True):
    """the whole chain, one call per stage over the whole stream -> dict of every stage's output"""
    a, _ = agc(x, rate, reference, max_gain)
    s, e, i, _, _ = timing(a, algorithm, decimation, loop_gain, max_error, use_q)
    b = dbpsk(s)
    t, _ = varicode_decode(b)
    return dict(agc=a, symbols=s, errors=e, indexes=i, bits=b, text=t)


# ------------------------------------------------------------------ generator
def varicode_encode(text):
    """psk31_varicode_encoder_u8_u8: each character's code, MSB first, then 00"""
    bits = []
    for ch in text:
        c = VARICODE[ch if isinstance(ch, int) else ord(ch)]
        bits += [int(b) for b in c] + [0, 0]
    return np.array(bits, np.uint8)


def differential_encode(bits, state=0):
    """differential_codec(encode=1): a 0 bit toggles the state"""
    out = np.empty(len(bits), np.uint8)
    for k, b in enumerate(np.asarray(bits).tolist()):
        if not b:
            state = 1 - state
        out[k] = state
    return out


def interpolate_sine(symbols, interpolation, last=0j):
    """psk31_interpolate_sine_cc: raised-cosine transitions from the last symbol to the next, `interpolation` samples each"""
    s = np.asarray(symbols, np.complex64)
    j = np.arange(interpolation)
    rate = np.array([(1 + math.sin(-(math.pi / 2) + math.pi * (f32(k + 1) / f32(interpolation)))) / 2 for k in j], np.float64).astype(f32)
    prev = np.concatenate([[np.complex64(last)], s[:-1]]).astype(np.complex64)
    out_i = s.real[:, None].astype(f32) * rate[None] + prev.real[:, None].astype(f32) * (f32(1) - rate)[None]
    out_q = s.imag[:, None].astype(f32) * rate[None] + prev.imag[:, None].astype(f32) * (f32(1) - rate)[None]
    out = np.empty(out_i.size, np.complex64)
    out.real = out_i.reshape(-1); out.imag = out_q.reshape(-1)
    return out


def psk31_signal(text, decimation=256, amplitude=0.3, carrier=0.0, phase=0.0, timing_offset=0, snr_db=None, preamble=32, postamble=32, seed=0):
    """a baseband PSK31 burst: idle reversals (preamble zeros), the text's varicode, idle again; differential BPSK, cosine-shaped reversals.
    carrier: offset in cycles per sample; timing_offset: samples of silence-free lead-in; snr_db: AWGN against the signal power."""
    rng = np.random.default_rng(seed)
    bits = np.concatenate([np.zeros(preamble, np.uint8), varicode_encode(text), np.zeros(postamble, np.uint8)])
    st = differential_encode(bits)
    sym = np.where(st == 1, -1.0, 1.0).astype(np.complex64)          # psk_modulator_u8_c 2: state 1 -> phase pi
    x = interpolate_sine(sym, decimation).astype(np.complex128) * amplitude
    if timing_offset:
        x = np.concatenate([np.full(timing_offset, x[0]), x])
    n = np.arange(x.size)
    x = x * np.exp(1j * (2 * np.pi * carrier * n + phase))
    if snr_db is not None:
        p = np.mean(np.abs(x) ** 2)
        sigma = math.sqrt(p / (10 ** (snr_db / 10)) / 2)
        x = x + sigma * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    return x.astype(np.complex64)
