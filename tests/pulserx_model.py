"""The model of the pulse-shaped receive stream, in numpy: matched filter (apply_real_fir_cc's convention, no zeros in front) evaluated only where
timing_recovery_cc reads it, the timing loop in float32, gain and slicer.  The order of a filtered sample's T products is the library's definition:
16 partial sums over t = r (mod 16), each in ascending t by one fused multiply-add per product from 0, then p[r] += p[r + s] for r < s, s = 8, 4, 2, 1.
All channels of a batch walk in step (each with its own positions), so a batch costs about what one channel does.  A restatement of what
libcsdr.c:1977-2072, 2276-2291, 1139-1142 and 1731-1765 compute, not a copy of them; also the signals and the float64 figures of the tests."""
import numpy as np

import pulse_model as pm

f32 = np.float32
c64 = np.complex64
GARDNER, EARLYLATE = 0, 1
FILTER, TIMING, SLICE = 0, 1, 2


def fold16(p):
    """[..., 16] float32 -> [...]: p[r] += p[r + s] for r < s, s = 8, 4, 2, 1, every sum rounded to float32"""
    p = np.asarray(p, f32)
    for s in (8, 4, 2, 1):
        p = (p[..., :s] + p[..., s:2 * s]).astype(f32)
    return p[..., 0]


def dot32(x, pos, taps):
    """x: [channels, n] complex64, pos: [channels, P] start indexes -> the filtered samples f[pos] as (re, im) float32 [channels, P], in the defined order"""
    taps = np.asarray(taps, f32)
    T = taps.size
    nch, P = pos.shape
    xr = np.ascontiguousarray(x.real); xi = np.ascontiguousarray(x.imag)
    acc = np.zeros((2, nch, P, 16), f32)
    r = np.arange(16)
    rows = np.arange(nch)[:, None, None]
    for t0 in range(0, T, 16):
        t = t0 + r
        on = t < T
        tt = np.where(on, t, 0)
        at = pos[:, :, None] + tt[None, None, :]
        w = np.broadcast_to(taps[tt], at.shape)
        v = np.stack([xr[rows, at], xi[rows, at]])
        acc = np.where(on, pm.fma32(v, w[None], acc), acc)
    return fold16(acc[0]), fold16(acc[1])


def _trunc_int(v):
    return np.trunc(v.astype(np.float64)).astype(np.int64)


def receive(x, taps=None, decimation=8, algorithm=GARDNER, use_q=True, loop_gain=0.5, max_error=2.0, first=FILTER, last=SLICE, gain=1.0, n_symbols=2,
            slice_q=False):
    """x: [channels, n] complex64, the whole stream of every channel -> a list of per-channel dicts: sym (complex64), err (float32, unclamped), idx
    (uint32), corr (the correction each symbol produced), bytes (from SLICE), out (what the object writes at `last`) and state (tail_len,
    correction_offset, base) behind the stream"""
    x = np.atleast_2d(np.asarray(x, c64))
    nch, n = x.shape
    D = int(decimation); hb, qb = D // 2, D // 4
    wing = int(f32(D) * f32(0.25))
    T = np.asarray(taps).size if first == FILTER else 1
    Tm1 = T - 1
    lg, me = f32(loop_gain), f32(max_error)
    hb_sign = f32(hb * (-1 if algorithm == GARDNER else 1))
    cbi = np.zeros(nch, np.int64); corr = np.zeros(nch, np.int64)
    held_at = np.full(nch, -1, np.int64)
    sym = [[] for _ in range(nch)]; errs = [[] for _ in range(nch)]; idxs = [[] for _ in range(nch)]; corrs = [[] for _ in range(nch)]
    while True:
        act = cbi + 3 * hb + Tm1 < n
        if not act.any():
            break
        corr = np.where(act & ((corr <= -qb * 0.9) | (corr >= 0.9 * qb)), 0, corr)
        if algorithm == EARLYLATE:
            pr = cbi + 3 * wing; pl = cbi + wing - corr; pmid = cbi + hb
        else:
            pr = cbi + 3 * hb; pl = cbi + hb; pmid = cbi + 2 * hb
        pos = np.where(act[:, None], np.stack([pl, pmid, pr], 1), 0)
        if first == FILTER:
            re, im = dot32(x, pos, taps)
        else:
            v = x[np.arange(nch)[:, None], pos]
            re, im = np.ascontiguousarray(v.real), np.ascontiguousarray(v.imag)
        with np.errstate(over="ignore", invalid="ignore"):
            e = ((re[:, 2] - re[:, 0]).astype(f32) * re[:, 1]).astype(f32)
            if use_q:
                e = (e + ((im[:, 2] - im[:, 0]).astype(f32) * im[:, 1]).astype(f32)).astype(f32)
                e = (e / f32(2)).astype(f32)
            ec = np.where(np.isnan(e), f32(0), e).astype(f32)      # a NaN error corrects by 0 (psk31_correction)
            ec = np.where(ec > me, me, ec).astype(f32)
            ec = np.where(ec < -me, -me, ec).astype(f32)
            new_corr = _trunc_int(((ec * lg).astype(f32) * hb_sign).astype(f32))
        o = 1 if algorithm == EARLYLATE else 0
        po = pmid if algorithm == EARLYLATE else pl
        for ch in np.nonzero(act)[0]:
            sym[ch].append(complex(re[ch, o], im[ch, o])); errs[ch].append(e[ch]); idxs[ch].append(po[ch]); corrs[ch].append(new_corr[ch])
        corr = np.where(act, new_corr, corr)
        cbi = np.where(act, cbi + D + corr, cbi)
    res = []
    for ch in range(nch):
        s = np.array(sym[ch], c64)
        # (complex() above went through float64: exact for float32 values, so the bits are kept)
        d = {"sym": s, "err": np.array(errs[ch], f32), "idx": (np.array(idxs[ch], np.int64) & 0xFFFFFFFF).astype(np.uint32),
             "corr": np.array(corrs[ch], np.int64), "state": (int(n - cbi[ch]), int(corr[ch]), int(cbi[ch]) & 0xFFFFFFFF)}
        if last == SLICE:
            g = f32(gain)
            if slice_q:
                soft = (g * s.view(f32)).astype(f32)
            else:
                soft = (g * np.ascontiguousarray(s.real)).astype(f32)
            d["soft"] = soft
            d["bytes"] = pm.slicer(soft, n_symbols)
            d["out"] = d["bytes"]
        else:
            d["out"] = s
        res.append(d)
    return res


# ------------------------------------------------------------------ signals
def signal(n_psk, sps, taps, n_symbols=300, n_channels=1, rms=1.0, snr_db=20.0, seed=1):
    """[n_channels, n] complex64: random n_psk symbols through pulse_model.shape64 (the transmit stream in float64), channel ch delayed by ch % sps
    samples, white noise at snr_db below the signal, scaled so that the stream behind the matched filter `taps` has about the RMS `rms`"""
    rng = np.random.default_rng(seed + 7919 * n_psk + 31 * sps + np.asarray(taps).size)
    table = pm.symbols(n_psk).astype(np.complex128)
    idx = rng.integers(0, n_psk, (n_channels, n_symbols))
    y, _, _ = pm.shape64(table[idx], sps, taps)
    y = np.atleast_2d(y)
    n = y.shape[1] + sps
    x = np.zeros((n_channels, n), np.complex128)
    for ch in range(n_channels):
        d = ch % sps
        x[ch, d:d + y.shape[1]] = y[ch]
    p = np.mean(np.abs(y) ** 2)
    sigma = np.sqrt(p / 10 ** (snr_db / 10) / 2)
    x += sigma * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))
    t = np.asarray(taps, np.float64)
    filt = np.correlate(x[0], t, "valid")
    x *= rms / np.sqrt(np.mean(np.abs(filt) ** 2))
    return x.astype(c64), idx.astype(np.uint8)


def filter64(x, taps):
    """one channel's whole filtered stream in float64 and the sums of the magnitudes of every sample's products: (f, mag_re, mag_im)"""
    x = np.asarray(x, np.complex128); t = np.asarray(taps, np.float64)
    return (np.correlate(x, t, "valid"), np.correlate(np.abs(x.real), np.abs(t), "valid"), np.correlate(np.abs(x.imag), np.abs(t), "valid"))
