"""Float64 references for the tap-consuming kernels, a per-sample error gate, an exact impulse comb, and a transcription of
fir_decimate_cc's / fir_ff's instance dispatch (csdr_amd/csrc/fir.hip).

References.  Every reference takes the exact float32 inputs and taps and sums in float64:
    fir_decimate_cc   y[i] = sum_t h[t] x[D i + t],  n_out = (n - L) // D + 1        (libcsdr.c:528-549: correlation, not convolution)
    fir_ff            y[i] = sum_t h[t] x[i + t],    n_out = n - L                   (libcsdr.c:1121)
    bandpass_fir_fft  y = (x * h)[:n], the linear convolution that overlap-add computes, complex taps
    resamplers        resampler_model.py, evaluated once on (x, h) and once on (|x|, |h|) for the condition sums

The per-sample gate of a direct-form (or polyphase, or matrix-core) float32 sum.  Output i is a sum of L products p_t = h_t x_{Di+t}.
Whatever order a kernel adds them in, each product is rounded once (or not at all under an FMA) and each partial sum once, every rounding
contributes at most u = 2^-24 times a partial sum, and every partial sum is bounded by c_i = sum_t |h_t| |x_{Di+t}|, output i's own
condition sum.  So the error is at most about L u c_i in the worst case (Higham, Accuracy and Stability of Numerical Algorithms, 4.2), and
when the rounding errors have random signs, as they do on random data, it grows like sqrt(L) u c_i.  The gate is
    |y_i - y64_i| <= kappa(L) u c_i,   kappa(L) = 4 ceil(sqrt(L)) + 4,
about L^1.5 times tighter than the contribution of a single average tap (|h_t x| ~ c_i / L): 16 times at 4096 taps.  Complex data is gated
per component (real and imaginary parts are separate real sums with their own c_i).  The resamplers scale their sums by I: one more rounding,
covered by the +4.  test_fir_reference_cpu.py shows that a float32 sequential and a float32 pairwise sum pass the gate with a wide margin
at every shape the GPU tests run, and that reversed taps and a single zeroed tap (first, middle, last) fail it.

The FFT filter's error is not a property of one output's taps: every output of a transform of size N carries rounding from the whole
window, about u log2(N) ||h||_2 times the RMS of the window's input.  Its gate is
    |y_i - y64_i| <= KAPPA_FFT u log2(N) ||h||_2 ||x_{i-L+1..i}||_2,
with ||x_{i-L+1..i}||_2 >= sqrt(L) RMS(x) on stationary input, which leaves room for the window's own variation.  KAPPA_FFT = 4: the oracle's
float32 FFT filter uses a few percent of it, conjugated taps exceed it by orders of magnitude (test_fir_reference_cpu.py).

The impulse comb.  Impulses of amplitude +-2^k, on the real part of some and the imaginary part of others, at least L samples apart: every
output window sees at most one impulse, every product is a power of two times a tap (exact), and every other term is an exact zero.  So a
direct-form kernel's response is exactly a h[k - D i] at the outputs whose window covers the impulse at k and exactly zero elsewhere."""
import math
import numpy as np

f32 = np.float32
U = 2.0 ** -24
KAPPA_FFT = 4.0


def kappa(L):
    return 4 * math.ceil(math.sqrt(L)) + 4


def random_taps(L, seed):
    """float32 taps with no symmetry (the generator of every asymmetric-tap test): random signs, magnitudes uniform in [1/4, 1), so that no
    tap is so small that zeroing it hides under the gate"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], L) * rng.uniform(0.25, 1.0, L)).astype(f32)


def crand(rng, shape):
    return (rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)).astype(np.complex64)


# ------------------------------------------------------------------ float64 references
def _windows(x, D, L, n_out):
    return np.lib.stride_tricks.sliding_window_view(x, L)[:(n_out - 1) * D + 1:D]


def _corr(x, h, D, n_out, chunk=512):
    out = np.zeros(n_out, np.float64)
    for a in range(0, n_out, chunk):
        b = min(n_out, a + chunk)
        out[a:b] = _windows(x[a * D:(b - 1) * D + h.size], D, h.size, b - a) @ h
    return out


def fir_real(x, D, taps):
    """y64, c: y64[i] = sum_t h[t] x[D i + t] in float64 and c[i] = sum_t |h[t]| |x[D i + t]| for real x"""
    x = np.asarray(x, np.float64); h = np.asarray(taps, f32).astype(np.float64)
    n_out = (x.size - h.size) // D + 1 if x.size >= h.size else 0
    return _corr(x, h, D, n_out), _corr(np.abs(x), np.abs(h), D, n_out)


def fir_decimate_cc(x, D, taps):
    """(y64 complex128, c_re, c_im) of fir_decimate_cc (n_out = (n - L) // D + 1)"""
    x = np.asarray(x, np.complex64)
    yr, cr = fir_real(x.real, D, taps)
    yi, ci = fir_real(x.imag, D, taps)
    return yr + 1j * yi, cr, ci


def fir_ff(x, taps):
    """(y64, c) of fir_ff: n_out = n - L (libcsdr.c:1121 stops one output short of the full correlation)"""
    y, c = fir_real(np.asarray(x, f32), 1, taps)
    n_out = max(np.asarray(x).size - np.asarray(taps).size, 0)
    return y[:n_out], c[:n_out]


def convolve_cc(x, taps, n):
    """the first n samples of the linear convolution of complex x with complex taps (bandpass_fir_fft_cc's overlap-add result), by a float64
    FFT of the whole stream: its rounding (~1e-16 relative) is far below any float32 gate, and np.convolve's direct sum would take minutes at
    8191 taps x 200000 samples"""
    x = np.asarray(x, np.complex64).astype(np.complex128); h = np.asarray(taps, np.complex64).astype(np.complex128)
    m = 1 << int(math.ceil(math.log2(x.size + h.size - 1)))
    return np.fft.ifft(np.fft.fft(x, m) * np.fft.fft(h, m))[:n]


def fft_bound(x, taps, n, fft_size):
    """per-sample bound of the FFT filter: KAPPA_FFT u log2(N) ||h||_2 ||x_{i-L+1..i}||_2 for i < n"""
    x = np.asarray(x, np.complex64).astype(np.complex128); h = np.asarray(taps, np.complex64).astype(np.complex128)
    e = np.concatenate([np.zeros(h.size), np.abs(x[:n]) ** 2])
    cs = np.cumsum(e)
    win = cs[h.size:h.size + n] - cs[:n]
    return KAPPA_FFT * U * math.log2(fft_size) * np.linalg.norm(h) * np.sqrt(np.maximum(win, 0.0))


# ------------------------------------------------------------------ the gate
def gate_ratio(y, y64, c, L):
    """worst |y - y64| / (kappa(L) u c) over the outputs: <= 1 passes.  Outputs whose condition sum is 0 must be exact."""
    err = np.abs(np.asarray(y, np.float64) - np.asarray(y64, np.float64))
    bound = kappa(L) * U * np.asarray(c, np.float64)
    if err.size == 0:
        return 0.0
    if np.any((bound == 0) & (err != 0)):
        return np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, 0.0)
    return float(r.max())


def gate_ratio_cc(y, y64, c_re, c_im, L):
    y = np.asarray(y)
    return max(gate_ratio(y.real, y64.real, c_re, L), gate_ratio(y.imag, y64.imag, c_im, L))


def fft_gate_ratio(y, y64, bound):
    err = np.abs(np.asarray(y, np.complex128) - y64)
    if err.size == 0:
        return 0.0
    if np.any((bound == 0) & (err != 0)):
        return np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, 0.0).max())


# ------------------------------------------------------------------ the shapes the GPU tests run (test_fir_taps_gpu.py) and the self-check covers
# fir_decimate_cc: (D, odd taps, even taps, instance), every k_fir_* instance the dispatch reaches (fir_decimate_instance below)
DECIMATE = [
    (4, 63, 64, "k_fir_poly<R4,U24>"),
    (10, 159, 160, "k_fir_poly<R4,U44>"),
    (10, 161, 162, "k_fir_poly<R2,U24>"),
    (14, 951, 952, "k_fir_poly<R2,U44>"),
    (20, 161, 162, "k_fir_mfma3<8>"),
    (14, 953, 954, "k_fir_mfma3<10>"),
    (11, 1365, 1366, "k_fir_mfma3<12>"),
    (10, 1481, 1482, "k_fir_mfma3<13>"),
    (9, 1621, 1622, "k_fir_mfma3<14>"),
    (10, 1801, 1802, "k_fir_mfma<8,16>"),
    (22, 4043, 4042, "k_fir_mfma<8,32>"),
    (22, 4045, 4044, "k_fir_mfma<4,32>"),
    (98, 1031, 1032, "k_fir_mfma<2,16>"),
    (39, 4099, 4100, "k_fir_mfma<2,32>"),
    (131, 2109, 2110, "k_fir_mfma<1,16>"),
    (67, 4073, 4072, "k_fir_mfma<1,32>"),
    (2, 8201, 8200, "k_fir_generic"),
]
# fir_ff: (odd taps, even taps, instance)
FIR_FF = [(999, 1000, "k_fir_poly<R4,U24>"), (1999, 2000, "k_fir_poly<R4,U44>"), (2553, 2554, "k_fir_poly<R2,U44>"), (3001, 3000, "k_fir_generic")]
# rational_resampler_ff (I, D, T) and fir_interpolate_cc (I, T): T no multiple of I (but for I = 1)
RR = [(1, 4, 81), (1, 6, 81), (3, 2, 82), (2, 3, 81), (5, 7, 81), (4, 1, 81), (147, 160, 4001)]
INTERP = [(2, 81), (4, 83), (5, 81), (3, 80), (16, 161), (7, 4001), (147, 4001)]


def decimate_taps(D, L):
    return random_taps(L, 1000 * D + L)


def decimate_input_length(D, L, instance):
    """an even input length whose output count, 2 tiles + 37, is no multiple of the instance's tile"""
    n = (2 * tile_outputs(instance) + 36) * D + L
    return n + (n & 1)


def ff_taps(L):
    return random_taps(L, 5000 + L)


def rr_taps(I, D, T):
    return random_taps(T, 9000 + T + I)


def interp_taps(I, T):
    return random_taps(T, 7000 + T + I)


# ------------------------------------------------------------------ an honest float32 sum (the self-check)
def fir_f32_sequential(x, D, taps):
    """float32 sum in t = 0 .. L-1 order, one rounding per product and per addition (the reference's loop)"""
    x = np.asarray(x, f32); h = np.asarray(taps, f32)
    n_out = (x.size - h.size) // D + 1
    W = _windows(x, D, h.size, n_out)
    acc = np.zeros(n_out, f32)
    for t in range(h.size):
        acc = (acc + W[:, t] * h[t]).astype(f32)
    return acc


# ------------------------------------------------------------------ impulse comb
def comb_length(L, D=1):
    """an input length at which impulse_comb reaches every residue mod D (D + 8 impulses with gaps < L + D)"""
    return (D + 8) * (L + D) + L


def impulse_comb(n, L, D=1, tile=None, seed=0, complex_=True):
    """(x, positions, amplitudes): impulses of +-2^k (k in -3..3), real on even-numbered and imaginary on odd-numbered impulses (complex_),
    at least L apart.  First placed: the first and the last sample, and both sides of the first two and the last `tile`-output edge (the last
    input of the tile before, the first and the last input of the tile's first output); then, walking forward, impulses on residues
    0, 1, 2, ... mod D in turn, so that every residue is reached when n >= comb_length(L, D)."""
    rng = np.random.default_rng(seed)
    first = [0, n - 1]
    if tile:
        edges = list(range(tile * D, n - L, tile * D))
        for e in edges[:2] + edges[-1:]:
            first += [e - 1, e, e + L - 1]
    pos = []
    for p in first:
        if 0 <= p < n and all(abs(p - q) >= L for q in pos):
            pos.append(p)
    cur, r = 0, 0
    while cur < n:
        p = cur + (r - cur) % D
        clash = [q for q in pos if abs(p - q) < L]
        if clash:
            cur = max(clash) + L
            continue
        if p < n:
            pos.append(p)
        cur, r = p + L, (r + 1) % D
    pos.sort()
    amps = []
    x = np.zeros(n, np.complex64 if complex_ else f32)
    for j, p in enumerate(pos):
        a = float(rng.choice([-1.0, 1.0])) * 2.0 ** int(rng.integers(-3, 4))
        if complex_ and j % 2:
            x[p] = 1j * a; amps.append(1j * a)
        else:
            x[p] = a; amps.append(a)
    return x, np.array(pos, np.int64), np.array(amps, np.complex128 if complex_ else np.float64)


def comb_response(n_out, D, taps, pos, amps, scale=1.0):
    """the exact response of the decimating correlation y[i] = scale sum_t h[t] x[D i + t] to the comb: a scale h[k - D i] (float32)"""
    h = np.asarray(taps, f32)
    cplx = np.iscomplexobj(amps)
    y = np.zeros(n_out, np.complex64 if cplx else f32)
    for k, a in zip(pos, amps):
        i0 = max(0, -(-(k - h.size + 1) // D)); i1 = min(n_out - 1, k // D)
        for i in range(i0, i1 + 1):
            v = h[k - D * i] * f32(scale)
            y[i] = (a.real * v + 1j * (a.imag * v)) if cplx else f32(a) * v
    return y


def rr_comb_response(n_out, I, D, taps, pos, amps):
    """rational_resampler_ff's exact response to a real comb (impulses >= T apart): output o = I sum_{i < K_o} x[s_o + i] taps[d_o + i I]
    (resampler_model.rr_schedule) -> a float32(taps[t] I) where one impulse falls inside the output's K_o inputs"""
    import resampler_model as rm
    h = np.asarray(taps, f32)
    s, d, k = rm.rr_schedule(n_out, I, D, h.size)
    y = np.zeros(n_out, f32)
    for p, a in zip(pos, amps):
        j = p - s
        hit = np.nonzero((j >= 0) & (j < k))[0]
        y[hit] = f32(a) * (h[d[hit] + j[hit] * I] * f32(I))
    return y


def interp_comb_response(n_out, I, taps, pos, amps):
    """fir_interpolate_cc's exact response to a comb: output (q, ip) = sum_k x[q + k] taps[(k + 1) I - ip], so the impulse at p reaches it
    through tap (p - q + 1) I - ip when p >= q and that tap exists"""
    h = np.asarray(taps, f32)
    o = np.arange(n_out); q, ip = o // I, o % I
    y = np.zeros(n_out, np.complex64)
    for p, a in zip(pos, amps):
        t = (p - q + 1) * I - ip
        hit = np.nonzero((p >= q) & (t < h.size))[0]
        v = h[t[hit]]
        y[hit] = (a.real * v) + 1j * (a.imag * v)
    return y


# ------------------------------------------------------------------ fir.hip's instance dispatch, transcribed
def _poly_cfg(D, L, elem):
    for R in (4, 2):
        NA = ((L + D - 1) // D + 2 * R - 1) // (2 * R) * (2 * R)
        Q = (64 * R + NA + R + 1) & ~1
        if Q % 4 == 0:
            Q += 2
        if D * Q * elem + D * NA * 4 + 32 > 48 * 1024:
            continue
        for Uu in (24, 44):
            if D * Q <= 64 * Uu:
                return R, Uu
    return None


def fir_decimate_instance(D, L, input_size, in_pitch, force_generic=False):
    """the k_fir_* instance csdr_amd_fir_decimate_cc launches (16-byte aligned input rows assumed); None: no kernel (the call fails)"""
    pc = None if force_generic else _poly_cfg(D, L, 8)
    if pc:
        return "k_fir_poly<R%d,U%d>" % pc
    for nt in (8, 4, 2, 1):
        W = (16 * nt - 1) * D + L; steps = (15 * D + L + 3) // 4
        if 4 * (2 * (W + 8) + 32 + 15 * D + 4 * steps + 4 + 1024) > 76 * 1024:
            continue
        ns = -(-(W + 8) // 256)
        if ns > 32:
            continue
        nblk = (steps + 3) // 4
        win = 16 * D * 7 + 16 * nblk + 8
        lds3 = ((8 * win + 1023) & ~1023) + 4 * (15 * D + 16 * nblk + 16 + 2048)
        if nt == 8 and (nblk + 7) // 8 + 1 <= 15 and win <= 8192 and in_pitch % 2 == 0 and input_size % 2 == 0 and lds3 <= 80 * 1024:
            need = (nblk + 7) // 8
            return "k_fir_mfma3<%d>" % (8 if need <= 8 else 10 if need <= 10 else 12 if need <= 12 else 13 if need <= 13 else 14)
        return "k_fir_mfma<%d,%d>" % (nt, 8 if ns <= 8 else 16 if ns <= 16 else 32)
    to = 1024
    while to > 1 and ((to - 1) * D + L) * 8 > 64 * 1024:
        to //= 2
    return "k_fir_generic" if ((to - 1) * D + L) * 8 <= 160 * 1024 - 256 else None


def fir_ff_instance(L, force_generic=False):
    pc = None if force_generic else _poly_cfg(1, L, 4)
    return "k_fir_poly<R%d,U%d>" % pc if pc else "k_fir_generic"


def tile_outputs(instance):
    """outputs per tile of an instance"""
    if instance.startswith("k_fir_poly"):
        return 64 * int(instance[len("k_fir_poly<R")])
    if instance.startswith("k_fir_mfma3"):
        return 128
    if instance.startswith("k_fir_mfma<"):
        return 16 * int(instance[len("k_fir_mfma<")])
    return 1024
