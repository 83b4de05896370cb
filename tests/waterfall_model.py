"""float64 model of the waterfall path `[convert_u8_f |] fft_cc N E window | logaveragepower_cf A N AVG | fft_exchange_sides_ff N` (csdr.c:1569-1714), shared by
tests/test_waterfall_cpu.py, tests/test_waterfall_gpu.py and bench_waterfall.py --verify.

Frames follow fft_cc's schedule: frame k covers stream samples [k E + off, k E + off + N), off = min(0, E - N), positions before 0 being the zeros of the fresh
sliding buffer.  The window is the library's float table (oracle.port().precalculate_window), the transform np.fft.fft in float64, the power is summed over
the row's frames, add_db' = float32(add_db - 10 log10(avg)) as csdr.c:1678 forms it, and the halves are exchanged."""
import numpy as np


def samples(x, in_format):
    """stream samples as complex128: cf32 as given, u8 IQ pairs through convert_u8_f's float32 arithmetic (libcsdr.c:2365)"""
    if in_format == "u8":
        u = np.asarray(x, np.uint8).astype(np.float64)
        f = (u / 127.5 - 1.0).astype(np.float32).astype(np.float64)
        return f[0::2] + 1j * f[1::2]
    return np.asarray(x, np.complex64).astype(np.complex128)


def add_db_eff(add_db, avg):
    return np.float32(np.float64(np.float32(add_db)) - 10.0 * np.log10(avg))


def rows(x, in_format, fft, every, window_table, avg, add_db=0.0):
    """-> (power, db): [rows, fft] float64 each, halves exchanged; only complete rows"""
    s = samples(x, in_format)
    off = every - fft if every < fft else 0
    n_frames = 0 if s.size < off + fft else (s.size - off - fft) // every + 1
    n_rows = n_frames // avg
    w = np.asarray(window_table, np.float32).astype(np.float64)
    power = np.zeros((n_rows, fft))
    pad = np.concatenate([np.zeros(-off, np.complex128), s])
    for r in range(n_rows):
        for k in range(r * avg, (r + 1) * avg):
            a = k * every                                     # index in pad of stream position k E + off
            X = np.fft.fft(pad[a:a + fft] * w)
            power[r] += X.real ** 2 + X.imag ** 2
    power = np.roll(power, fft // 2, axis=1)
    db = 10 * np.log10(np.maximum(power, 1e-300)) + float(add_db_eff(add_db, avg))
    return power, db


def relrms(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2) / np.mean(b ** 2)))


def db_gate(db_got, db_want, span=60.0):
    """max |dB error| over the bins within `span` dB of each row's peak"""
    db_got = np.atleast_2d(db_got); db_want = np.atleast_2d(db_want)
    m = db_want >= db_want.max(axis=1, keepdims=True) - span
    return float(np.abs(db_got - db_want)[m].max())
