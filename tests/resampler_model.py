"""Float64 model of rational_resampler_ff (libcsdr.c:607-640) and fir_interpolate_cc (libcsdr.c:579-605), and of the CLI loops that drive them
(csdr.c:1409-1460, 1179-1232).  Index bookkeeping is the reference's integer arithmetic; the sums are float64 (dtype=np.float32 rounds the inputs only)."""
import numpy as np


def rr_schedule(n, I, D, T, last_taps_delay=0):
    """(startingi, delayi, taps used) of outputs 0..n-1 by the reference's formulas"""
    oi = np.arange(n, dtype=np.int64)
    s = (oi * D + I - 1 - last_taps_delay) // I
    d = (last_taps_delay + s * I - oi * D) % I
    k = np.where(T - d > 0, (T - d) // I, 0)
    return s, d, k


def _rr_values(x, I, taps, s, d):
    x = np.asarray(x, np.float64); taps = np.asarray(taps, np.float64)
    T = taps.size
    out = np.zeros(s.size)
    for dv in np.unique(d):
        sel = np.nonzero(d == dv)[0]
        K = (T - dv) // I if T - dv > 0 else 0
        if K <= 0:
            continue
        idx = s[sel, None] + np.arange(K)[None, :]
        out[sel] = x[idx] @ taps[dv + np.arange(K) * I]
    return out * I


def rational_resampler_ff(x, I, D, taps, last_taps_delay=0):
    """one call of the reference function -> (outputs, (input_processed, output_size, last_taps_delay))"""
    n, T = len(x), len(taps)
    cap = n * I // D
    s, d, _ = rr_schedule(cap + 1, I, D, T, last_taps_delay)
    fits = s[:cap] + T // I + 1 <= n
    brk = int(np.argmin(fits)) if not fits.all() else cap
    if brk < cap:
        state = (int(s[brk]), brk, int(d[brk]))
    elif cap > 0:
        state = (int(s[cap - 1]), cap, int(d[cap - 1]))
    else:
        state = (0, 0, last_taps_delay)
    return _rr_values(x, I, taps, s[:brk], d[:brk]), state


def rational_resampler_cli(x, I, D, taps, bufsize):
    """the `csdr rational_resampler_ff` stream (csdr.c:1441-1459), complete windows only"""
    out, a, L = [], 0, 0
    while a + bufsize <= len(x):
        y, (p, _, L) = rational_resampler_ff(x[a:a + bufsize], I, D, taps, L)
        out.append(y)
        a += p if p else bufsize
    return np.concatenate(out) if out else np.zeros(0)


def fir_interpolate_cc(x, I, taps):
    """one call of the reference function (complex x)"""
    x = np.asarray(x, np.complex128); taps = np.asarray(taps, np.float64)
    n, T = len(x), len(taps)
    npos = 0
    while npos * I + I - 1 + T <= n * I:
        npos += 1
    if npos == 0:
        return np.zeros(0, np.complex128)
    out = np.zeros((npos, I), np.complex128)
    for ip in range(I):
        ks = np.arange(0, max(0, T))
        ks = ks[(ks + 1) * I - ip < T]
        if ks.size:
            out[:, ip] = x[np.arange(npos)[:, None] + ks[None, :]] @ taps[(ks + 1) * I - ip]
    return out.ravel()


def fir_interpolate_cli(x, I, taps, bufsize):
    """the `csdr fir_interpolate_cc` stream (csdr.c:1215-1231): its first pass runs over bufsize zeros"""
    return fir_interpolate_cc(np.concatenate([np.zeros(bufsize, np.complex128), np.asarray(x, np.complex128)]), I, taps)


def interp_bufsize(T, fixed_big=16384):
    """csdr.c:1198 + unitround: the big buffer doubled until it holds two filters"""
    b = fixed_big
    while b < 2 * T:
        b *= 2
    return ((b - 1) & ~3) + 4


def relrms(a, b):
    a = np.asarray(a); b = np.asarray(b)
    den = np.sqrt(np.mean(np.abs(b) ** 2)) if b.size else 0.0
    return float(np.sqrt(np.mean(np.abs(a - b) ** 2)) / den) if den else float(np.abs(a - b).max(initial=0.0))
