"""float64 model of the real-input spectrum path `[convert_s16_f |] fft_fc M E window | logaveragepower_cf A M AVG` (csdr.c:3414-3498, 1663-1695), shared by
tests/test_realfft_cpu.py, tests/test_realfft_gpu.py and bench_realfft.py --verify.

M is the number of output bins, a frame is N = 2M real samples.  Frame schedule in real samples, fft_fc's: E <= N: frame k covers [k E + E - N, k E + E),
positions before 0 being the zeros of the fresh sliding buffer; E > N: the reference's skip loop reads complexf-sized items from its float stream
(csdr.c:3466-3469), so it drops 2 (E - N) floats and frame k covers [k P, k P + N) with P = 2 E - N.  The window is the library's float table of N entries
(oracle.port().precalculate_window), the transform np.fft.rfft of float64 data (numpy 2 transforms float32 input in float32: cast first), bins 0 .. M-1 are
kept, the power is summed over the row's frames, add_db' = float32(add_db - 10 log10(avg)) as csdr.c:1678 forms it, and the halves are not exchanged: a
one-sided row is in display order."""
import numpy as np

from waterfall_model import add_db_eff, db_gate, relrms  # noqa: F401  (re-exported: the gates are the waterfall's)


def samples(x, in_format):
    """stream samples as float64: f32 as given, s16 through convert_s16_f's float32 arithmetic (a product with the rounded reciprocal of SHRT_MAX)"""
    if in_format == "s16":
        return (np.asarray(x, np.int16).astype(np.float32) * (np.float32(1.0) / np.float32(32767.0))).astype(np.float32).astype(np.float64)
    return np.asarray(x, np.float32).astype(np.float64)


def schedule(m, every):
    """-> (frame length N, period P, offset of frame 0): frame k covers [k P + off, k P + off + N)"""
    n = 2 * m
    return (n, every, every - n) if every <= n else (n, 2 * every - n, 0)


def n_frames(n_samples, m, every):
    n, p, off = schedule(m, every)
    return 0 if n_samples < off + n else (n_samples - off - n) // p + 1


def n_for_rows(m, every, avg, rows):
    """real samples that complete `rows` rows"""
    n, p, off = schedule(m, every)
    return (rows * avg - 1) * p + off + n


def row_width(m, out_format):
    """elements per row: M floats, or (M + 10) / 2 ADPCM bytes"""
    return m if out_format == "db" else (m + 10) // 2


def spectra(x, in_format, m, every, window_table):
    """fft_fc: -> [frames, M] complex128, only complete frames (the reference's repeated last frame at end of stream is not modelled)"""
    s = samples(x, in_format)
    n, p, off = schedule(m, every)
    k = n_frames(s.size, m, every)
    w = np.asarray(window_table, np.float32).astype(np.float64)
    assert w.size == n
    pad = np.concatenate([np.zeros(-off), s])
    out = np.zeros((k, m), np.complex128)
    for f in range(k):
        out[f] = np.fft.rfft(pad[f * p:f * p + n] * w)[:m]     # index in pad of stream position f P + off
    return out


def rows(x, in_format, m, every, window_table, avg, add_db=0.0):
    """-> (power, db): [rows, M] float64 each, DC first; only complete rows"""
    X = spectra(x, in_format, m, every, window_table)
    n_rows = X.shape[0] // avg
    power = (X.real ** 2 + X.imag ** 2)[:n_rows * avg].reshape(n_rows, avg, m).sum(axis=1)
    db = 10 * np.log10(np.maximum(power, 1e-300)) + float(add_db_eff(add_db, avg))
    return power, db
