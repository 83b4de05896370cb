"""Float32 model of the BPSK31 transmit chain (libcsdr.c: psk31_varicode_encoder_u8_u8 1551-1575, differential_codec 1828-1843, psk_modulator_u8_c
1772-1782, psk31_interpolate_sine_cc 1793-1808) and of duplicate_samples_ntimes_u8_u8 (1784-1791).

The model keeps C's arithmetic: the modulator's phase is the float product float(2 pi / n_psk) * byte, its cos and sin are taken in double and rounded
to float (so n_psk = 2 gives 1 + 0j and -1 - 8.742278e-8j, not -1 + 0j); the shaper's rate is a float quotient, the rest in double, rounded to float,
and its output is two float products and one float sum per component."""
import math
import numpy as np

from psk31_model import VARICODE

f32 = np.float32
STAGES = ["varicode", "diff", "mod", "shape"]


def varicode_encode(text):
    """bytes -> bits (uint8): each table character's code MSB first, then 00; bytes 128..255 give nothing"""
    bits = []
    for ch in bytes(text):
        if ch < 128:
            bits += [int(b) for b in VARICODE[ch]] + [0, 0]
    return np.array(bits, np.uint8)


def differential_encode(bits, state=0):
    """differential_codec(encode = 1) -> (states uint8, state after the last byte)"""
    out = np.empty(len(bits), np.uint8)
    for k, b in enumerate(np.asarray(bits, np.uint8).tolist()):
        if not b:
            state = 0 if state else 1
        out[k] = state
    return out, state


def differential_decode(x, state=0):
    """differential_codec(encode = 0) -> (output uint8, state after the last byte)"""
    x = np.asarray(x, np.uint8)
    prev = np.concatenate([[np.uint8(state)], x[:-1]]).astype(np.uint8) if x.size else x
    return (x == prev).astype(np.uint8), (int(x[-1]) if x.size else int(state))


def symbol_table(n_psk):
    """the 256 symbols of psk_modulator_u8_c n_psk, complex64"""
    inc = f32((2 * math.pi) / n_psk)
    t = np.empty(256, np.complex64)
    for v in range(256):
        ph = float(inc * f32(v))
        t[v] = complex(f32(math.cos(ph)), f32(math.sin(ph)))
    return t


def modulate(idx, n_psk=2):
    return symbol_table(n_psk)[np.asarray(idx, np.uint8)]


def rate_table(interpolation):
    """psk31_interpolate_sine_cc's factors, float32"""
    return np.array([(1 + math.sin(-(math.pi / 2) + math.pi * float(f32(j + 1) / f32(interpolation)))) / 2 for j in range(interpolation)],
                    np.float64).astype(f32)


def shape(symbols, interpolation, last=0j):
    """psk31_interpolate_sine_cc from last_input `last` -> (samples complex64, the last symbol)"""
    s = np.asarray(symbols, np.complex64)
    last = np.complex64(last)
    if not s.size:
        return np.zeros(0, np.complex64), last
    rate = rate_table(interpolation)
    r1 = f32(1) - rate
    prev = np.concatenate([[last], s[:-1]]).astype(np.complex64)
    out = np.empty((s.size, interpolation), np.complex64)
    out.real = s.real[:, None] * rate[None] + prev.real[:, None] * r1[None]
    out.imag = s.imag[:, None] * rate[None] + prev.imag[:, None] * r1[None]
    return out.reshape(-1), s[-1]


def duplicate_samples(x, sample_size, ntimes):
    x = np.asarray(x, np.uint8)
    m = x.size // sample_size
    return np.repeat(x[:m * sample_size].reshape(m, sample_size), ntimes, axis=0).reshape(-1)


def run(x, first="varicode", last="shape", n_psk=2, interpolation=256, state=(0, 0j)):
    """stages first..last over one stream from the channel state (diff_state, last symbol) -> (output, state after it)"""
    f, l = STAGES.index(first), STAGES.index(last)
    ds, ls = state
    y = np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x
    if f <= 0 <= l:
        y = varicode_encode(y)
    if f <= 1 <= l:
        y, ds = differential_encode(y, ds)
    if f <= 2 <= l:
        y = modulate(y, n_psk)
    if f <= 3 <= l:
        y, ls = shape(y, interpolation, ls)
    return y, (ds, ls)


def chain(text, n_psk=2, interpolation=256):
    """the whole chain from a fresh channel -> dict of every stage's output"""
    bits = varicode_encode(text)
    st, _ = differential_encode(bits)
    sym = modulate(st, n_psk)
    x, _ = shape(sym, interpolation)
    return dict(varicode=bits, diff=st, mod=sym, shape=x)
