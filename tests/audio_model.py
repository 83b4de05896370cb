"""Models of the demodulator and audio-rate blocks (csdr_amd/csrc/audio.hip, f2blocks.hip) in plain numpy: the host-side dispatch rules, an emulation of the
speculative de-emphasis run-in, a float32 emulation of dcblock_ff's three passes, float64 references with per-sample error bounds, input generators and a bit
compare.  Shared by tests/test_audio_blocks_cpu.py (which pins the models to the oracle and establishes the gates) and tests/test_audio_blocks_gpu.py.

Gates.  Every gate is  kappa * S_i  with S_i a structural bound evaluated along the float64 run (u = 2^-24 times the magnitudes that get rounded).  kappa is
4 x the worst ratio |float32 oracle - float64| / S_i over every shape the GPU file runs (for dcblock_ff also of the three-pass emulation): the factor 4 is the
allowance for a different but legitimate summation order (tree mean, segment carries).  test_audio_blocks_cpu.py re-measures the ratios, asserts the constants
below against them and writes both to profiles/audio_blocks_gates.md."""
import ctypes as C
import functools
import numpy as np

f32, f64, u32, c64 = np.float32, np.float64, np.uint32, np.complex64
U = 2.0 ** -24
SENTINEL = 1e30                       # in every input row's padding
PATTERN = f32(-7.25e22)               # every output buffer is filled with it before a call

# kappa per block (see the module docstring; measured ratios are in profiles/audio_blocks_gates.md)
KAPPA = {"dcblock_ff": 3.8, "fastdcblock_ff": 47.0, "fmdemod_atan_cf": 3.0, "amdemod_cf": 3.9, "logpower_cf": 3.6,
         "fastagc_ff": 2.5, "fractional_decimator_ff": 0.85}      # (the last two: gates of the compiled reference only, see fastagc_f64)


# ================================================================== bit compare
def bit_mismatches(got, want):
    """indices where got and want differ: NaN positions must coincide (payloads are not compared), everything else as uint32 (so +0 != -0)"""
    got = np.ascontiguousarray(got, f32).ravel(); want = np.ascontiguousarray(want, f32).ravel()
    assert got.size == want.size, (got.size, want.size)
    gn, wn = np.isnan(got), np.isnan(want)
    return np.nonzero((gn != wn) | (~gn & ~wn & (got.view(u32) != want.view(u32))))[0]


def assert_bits(got, want, what):
    bad = bit_mismatches(got, want)
    if bad.size:
        g, w = np.asarray(got, f32).ravel(), np.asarray(want, f32).ravel()
        raise AssertionError("%s: %d of %d values differ in bits, first at %d: %r vs %r" % (what, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]]))


# ================================================================== dispatch rules (csdr_amd_deemphasis_wfm_ff, csdr_amd_agc_ff, csdr_amd_fractional_decimator_ff)
DW_L = 256


def deemph_alpha(tau, sample_rate):
    dt = f32(1.0 / sample_rate)                                  # float after a double division
    return f32(dt / f32(f32(tau) + dt))


def deemph_run_in(tau, sample_rate, n_streams, n, in_place=False):
    """M of k_deemph_wfm_spec<M>, or 0 for the tiled serial kernel"""
    b = 1.0 - float(deemph_alpha(tau, sample_rate))
    if n_streams < 32 and n >= 8 * DW_L and 0.0 < b < 1.0 and not in_place:
        for m in (1, 2, 4, 8):
            if 256.0 * m * np.log2(b) < -40.0:
                return m
    return 0


def deemph_path(tau, sample_rate, n_streams, n, in_place=False):
    m = deemph_run_in(tau, sample_rate, n_streams, n, in_place)
    return "k_deemph_wfm_spec<%d>" % m if m else "k_deemph_wfm"


def agc_path(n_streams, n):
    return "k_agc_coop" if n_streams < 64 and n >= 256 else "k_agc"


def _lsb_exp(v):
    """exponent of the lowest set bit of a float32 (127 for 0)"""
    v = f32(v)
    if v == 0:
        return 127
    bits = int(np.array(v).view(u32))
    ef = (bits >> 23) & 255
    m = (bits & 0x7fffff) | (0x800000 if ef else 0)
    return (ef if ef else 1) - 127 - 23 + ((m & -m).bit_length() - 1)


def fracdec_exact(where, rate, input_size, num_poly_points, taps_length, cli_bufsize=0):
    """True when the plan is built on the device (every where <- where + rate is exact in float), False for the host walk"""
    P = num_poly_points & ~1
    q = min(_lsb_exp(where), _lsb_exp(rate), 0)
    win = cli_bufsize if cli_bufsize > 0 and input_size >= cli_bufsize else input_size
    return bool(q > -40 and 2.0 ** (q + 24) > float(win) + abs(float(f32(rate))) + P + taps_length + 4 and f32(where) >= 0)


class FracdecPath:
    """the plan cache of one csdr_amd_fracdec object: path(where, n) is what csdr_amd_audio_last_path() reports for a call that starts at `where`"""

    def __init__(self, rate, num_poly_points, taps_length, cli_bufsize=0):
        self.rate, self.P, self.T, self.buf, self.plan = rate, num_poly_points, taps_length, cli_bufsize, None

    def path(self, where, n):
        key = (float(f32(where)), n)
        if self.plan == key:
            return "fracdec:cached"
        self.plan = key
        return "fracdec:exact" if fracdec_exact(where, self.rate, n, self.P, self.T, self.buf) else "fracdec:walked"


# ================================================================== deemphasis_wfm_ff
def deemph_serial(x, alpha, last):
    """the reference's recurrence in float32, operation for operation (NaN state reset) -> (y, state in front of every 256-sample chunk)"""
    x = np.asarray(x, f32); alpha = f32(alpha); om = f32(f32(1) - alpha)
    y = f32(0) if np.isnan(last) else f32(last)
    out = np.empty(x.size, f32); starts = []
    with np.errstate(all="ignore"):
        for k in range(x.size):
            if k % DW_L == 0:
                starts.append(y)
            y = f32(f32(alpha * x[k]) + f32(om * y))
            out[k] = y
    return out, np.array(starts, f32)


def deemph_spec_mismatches(x, alpha, M, last):
    """Emulates k_deemph_wfm_spec<M>'s run-in: chunk c > M starts from zero M chunks earlier, chunks c <= M from the carried state.  Returns the number of
    chunks whose arrival state differs, bit for bit, from the serial recurrence's (a NaN on both sides counts as equal): the chunks the repair has to redo."""
    x = np.asarray(x, f32); alpha = f32(alpha); om = f32(f32(1) - alpha)
    nc = -(-x.size // DW_L)
    xp = np.zeros((nc + M) * DW_L, f32); xp[M * DW_L:M * DW_L + x.size] = x        # M chunks of padding in front, zeros behind n
    rows = xp.reshape(nc + M, DW_L)
    c = np.arange(nc)
    y = np.zeros(nc, f32)
    y[c <= M] = f32(0) if np.isnan(last) else f32(last)
    with np.errstate(all="ignore"):
        for m in range(M):
            live = c + m >= M                                                     # chunk c - M + m exists
            blk = rows[c + m]
            for k in range(DW_L):
                yn = alpha * blk[:, k] + om * y
                y = np.where(live, yn, y)
    _, starts = deemph_serial(x, alpha, last)
    return int(bit_mismatches(y, starts).size)


# ================================================================== dcblock_ff
SEG = 32


def _a_of(a):
    return f32(0.999) if a == 0 else f32(a)


def dcblock_emulate(x, a, state, fault=None):
    """float32 emulation of k_dc_local / k_dc_carry / k_dc_apply for one stream -> (y, (last_input, last_output)).
    fault: None, or one of the planted defects "prev0" (a segment's first difference taken against 0), "ragged" (the carry over a ragged last segment is
    built with a^32 -- the kernel reads that carry nowhere, so the defect is planted where it would show: the carried last_output is taken from it), "last"
    (the carry into the last segment is dropped)."""
    x = np.asarray(x, f32); a = _a_of(a); n = x.size
    ns = -(-n // SEG)
    xp = np.zeros(ns * SEG, f32); xp[:n] = x
    rows = xp.reshape(ns, SEG)
    prev0 = np.empty(ns, f32); prev0[0] = f32(state[0]); prev0[1:] = rows[:-1, -1]
    if fault == "prev0":
        prev0[1:] = 0
    lens = np.minimum(SEG, n - SEG * np.arange(ns))

    def walk(y0, store):
        y = y0.astype(f32).copy(); prev = prev0.copy(); out = np.zeros((ns, SEG), f32)
        for i in range(SEG):
            live = i < lens
            v = rows[:, i]
            yn = (v - prev) + a * y
            y = np.where(live, yn, y); prev = np.where(live, v, prev)
            out[:, i] = y
        return (y, out, prev) if store else y
    with np.errstate(all="ignore"):
        e = walk(np.zeros(ns, f32), False)
        aL = f32(1)
        for _ in range(SEG):
            aL = f32(aL * a)
        carry = np.empty(ns, f32); c = f32(state[1])
        for j in range(ns):
            carry[j] = c
            ap = aL
            if lens[j] < SEG and fault != "ragged":
                ap = f32(1)
                for _ in range(int(lens[j])):
                    ap = f32(ap * a)
            c = f32(f32(ap * c) + e[j])
        if fault == "last" and ns > 1:
            carry[-1] = 0
        y, out, prev = walk(carry, True)
    return out.ravel()[:n].copy(), (prev[-1], c if fault == "ragged" else y[-1])


def dcblock_f64(x, a, state=None, bound=None):
    """x [s, n] -> (y float64 [s, n], B [s, n], state (last_in, last_out) float64 [s] each, final B [s]).
    B_i = a B_{i-1} + u (|x_i - x_{i-1}| + |a y_{i-1}| + |y_i|): the first-order error bound of the float32 recurrence, carried with the state."""
    x = np.atleast_2d(np.asarray(x, f32)).astype(f64); a = float(_a_of(a)); s, n = x.shape
    prev = np.zeros(s) if state is None else np.asarray(state[0], f64).copy()
    y = np.zeros(s) if state is None else np.asarray(state[1], f64).copy()
    B = np.zeros(s) if bound is None else np.asarray(bound, f64).copy()
    ys = np.empty((s, n)); Bs = np.empty((s, n))
    for i in range(n):
        v = x[:, i]
        d = v - prev; ay = a * y
        y = d + ay
        B = a * B + U * (np.abs(d) + np.abs(ay) + np.abs(y))
        ys[:, i] = y; Bs[:, i] = B; prev = v
    return ys, Bs, (prev, y), B


def dcblock_bound_any_order(x, a, y64):
    """the same bound for an evaluation that may sum x_i - x_{i-1} + a y_{i-1} in any order (the compiled reference under -ffast-math): an intermediate sum is
    then as large as |x_i| + |x_{i-1}| + |a y_{i-1}|, not |x_i - x_{i-1}| -- at a DC level of 100 that is the difference between u and 100 u"""
    x = np.atleast_2d(np.asarray(x, f32)).astype(f64); a = float(_a_of(a)); y64 = np.atleast_2d(y64)
    prev = np.concatenate([np.zeros((x.shape[0], 1)), x[:, :-1]], axis=1); yp = np.concatenate([np.zeros((x.shape[0], 1)), y64[:, :-1]], axis=1)
    t = U * (np.abs(x) + np.abs(prev) + 2 * np.abs(a * yp) + np.abs(y64))
    B = np.empty_like(t); b = np.zeros(x.shape[0])
    for i in range(x.shape[1]):
        b = a * b + t[:, i]; B[:, i] = b
    return B


def gate_ratio(got, want64, S, kappa=1.0):
    """worst |got - want| / (kappa S) (a non-finite value where the reference is finite is infinitely far off)"""
    got = np.asarray(got, f64); want64 = np.asarray(want64, f64)
    err = np.abs(got - want64)
    err[~np.isfinite(got)] = np.inf
    return float(np.max(err / (kappa * S))) if got.size else 0.0


# ================================================================== fastdcblock_ff
def fastdcblock_f64(x, block, last_dc):
    """x [s, nb * block] -> (y float64, S, last_dc float64 [s]).  S_i = u (mean|x| + |last| + |avg| + |x_i| + |y_i|)"""
    x = np.atleast_2d(np.asarray(x, f32)).astype(f64); s, n = x.shape; nb = n // block
    last = np.asarray(last_dc, f64).reshape(s).copy()
    y = np.empty((s, nb * block)); S = np.empty_like(y)
    ramp = (np.arange(block, dtype=f32) / f32(block)).astype(f64)                 # (float)i / n
    for b in range(nb):
        xb = x[:, b * block:(b + 1) * block]
        avg = xb.mean(axis=1)
        yb = xb - (last[:, None] + (avg - last)[:, None] * ramp)
        y[:, b * block:(b + 1) * block] = yb
        S[:, b * block:(b + 1) * block] = U * (np.abs(xb).mean(axis=1)[:, None] + np.abs(last)[:, None] + np.abs(avg)[:, None] + np.abs(xb) + np.abs(yb))
        last = avg
    return y, S, last


# ================================================================== fmdemod_quadri_cf
K_FM = 0.340447550238101026565118445432744920253753662109375


def _fm_num_den(x, last):
    x = np.asarray(x, c64)
    p = np.concatenate([np.array([last], c64), x[:-1]])
    xi, xq, pi_, pq = x.real.astype(f32), x.imag.astype(f32), p.real.astype(f32), p.imag.astype(f32)
    with np.errstate(all="ignore"):
        dq, di = xq - pq, xi - pi_
        num = xi * dq - xq * di
        den = xi * xi + xq * xq
    return num, den


def fmdemod_quadri_ref(x, last=0j):
    """the reference's value: float32 numerator and denominator, double scale and divide, one rounding; 0 where the power is 0"""
    num, den = _fm_num_den(x, last)
    with np.errstate(all="ignore"):
        v = (K_FM * num.astype(f64) / den.astype(f64)).astype(f32)
    v[den == 0] = 0
    return v


def ulp_of(v):
    return np.spacing(np.abs(np.asarray(v, f32))).astype(f64)


def fmdemod_quadri_ulp_bound(x, last=0j):
    """worst distance, in ulps of the reference value, of a float32 emulation of the fast path -- Kf num rounded, a reciprocal anywhere within 1 ulp of the
    correctly rounded one, the product rounded -- over the samples of x with a normal reference value and a power inside the fast path's window; plus 1 ulp"""
    num, den = _fm_num_den(x, last)
    ref = fmdemod_quadri_ref(x, last)
    ok = np.isfinite(ref) & (np.abs(ref) >= np.finfo(f32).tiny) & (den >= 2.0 ** -60) & (den <= 2.0 ** 60) & (np.abs(num) >= 2.0 ** -100)
    if not ok.any():
        return 1.0
    num, den, ref = num[ok], den[ok], ref[ok]
    a = f32(K_FM) * num
    r0 = (1.0 / den.astype(f64)).astype(f32)
    worst = 0.0
    for r in (r0, np.nextafter(r0, f32(np.inf)), np.nextafter(r0, f32(0))):
        worst = max(worst, float(np.max(np.abs((a * r).astype(f64) - ref.astype(f64)) / ulp_of(ref))))
    return worst + 1.0


def fmdemod_quadri_check(got, x, last, gate_ulps):
    """-> (worst ulp distance over the samples with a normal reference value, number of samples compared absolutely).  Wherever the reference is finite the
    result must be finite; zero / subnormal reference values are compared absolutely (within gate_ulps of the smallest subnormal spacing)."""
    ref = fmdemod_quadri_ref(x, last); got = np.asarray(got, f32)
    fin = np.isfinite(ref)
    assert np.all(np.isfinite(got[fin])), "non-finite output at %d samples where the reference is finite, first %d" % (np.sum(~np.isfinite(got[fin])), np.nonzero(fin & ~np.isfinite(got))[0][0])
    assert not bit_mismatches(np.where(fin, 0, got), np.where(fin, 0, ref)).size, "inf / NaN positions differ from the reference's"
    small = fin & (np.abs(ref) < np.finfo(f32).tiny)
    big = fin & ~small
    d = np.abs(got[big].astype(f64) - ref[big].astype(f64)) / ulp_of(ref[big])
    assert np.all(np.abs(got[small].astype(f64) - ref[small].astype(f64)) <= gate_ulps * 2.0 ** -149)
    return (float(d.max()) if d.size else 0.0), int(small.sum())


# ================================================================== fmdemod_atan_cf, amdemod_cf, logpower_cf
PI_F = float(f32(3.14159265358979323846))


def fmdemod_atan_f64(x, last_phase):
    """-> (out float64, S, last phase).  phases in float64, unwrapped against the float constant PI as the reference does; S_i = u (|ph_i| + |ph_i-1| + 3 |d_i|) / PI"""
    x = np.asarray(x, c64)
    ph = np.arctan2(x.imag.astype(f64), x.real.astype(f64))
    p0 = np.concatenate([[float(last_phase)], ph[:-1]])
    d = ph - p0
    d = np.where(d < -PI_F, d + 2 * PI_F, d)
    d = np.where(d > PI_F, d - 2 * PI_F, d)
    return d / PI_F, U * (np.abs(ph) + np.abs(p0) + 3 * np.abs(ph - p0)) / PI_F + 1e-300, ph[-1]


def amdemod_f64(x):
    x = np.asarray(x, c64)
    v = np.sqrt(x.real.astype(f64) ** 2 + x.imag.astype(f64) ** 2)
    return v, 2 * U * v + 2.0 ** -149


def logpower_f64(x, add_db):
    """S_i = u (3 * 10 / ln 10 + 2 |10 log10 s| + |out|): the power's three roundings through the logarithm, the rounding of log10 and of 10 *, the sum's"""
    x = np.asarray(x, c64)
    s = x.real.astype(f64) ** 2 + x.imag.astype(f64) ** 2
    l = 10 * np.log10(s)
    return l + add_db, U * (30 / np.log(10) + 2 * np.abs(l) + np.abs(l + add_db))


# ================================================================== input generators
def envelope_steps(rng, n, every=None):
    """uniform noise under an envelope that steps by +-40 dB (between 0.01, 1 and 100)"""
    every = every or max(n // 7, 3)
    env = np.ones(n)
    lv = [1.0, 100.0, 1.0, 0.01, 1.0, 0.01, 100.0, 1.0]
    for j, at in enumerate(range(0, n, every)):
        env[at:at + every] = lv[j % len(lv)]
    return (rng.uniform(-1, 1, n) * env).astype(f32)


def with_zero_runs(x, runs=((0, 1),)):
    """x with runs of exact zeros: (start, length) pairs, clipped to x"""
    x = np.array(x, f32)
    for at, ln in runs:
        x[max(at, 0):max(at + ln, 0)] = 0
    return x


def agc_signal(rng, n, block, kind):
    """kind 0: +-40 dB envelope steps; 1: the same with zero runs -- the signal's first sample, the first sample of a later call, a whole call, a short run
    inside a call; 2: all zeros"""
    if kind == 2:
        return np.zeros(n, f32)
    x = envelope_steps(rng, n, max(n // 9, 2))
    if kind == 1:
        x = with_zero_runs(x, ((0, 1), (block, 1), (2 * block, block), (3 * block + block // 2, max(block // 5, 1)), (n - 3, 2)))
    return x


def bursts(rng, n, period=97, length=11, amp=30.0):
    x = rng.uniform(-1, 1, n) * 0.01
    for at in range(period // 2, n, period):
        x[at:at + length] *= amp / 0.01
    return x.astype(f32)


def fm_signal(rng, n, mag=0.7):
    ph = np.cumsum(rng.uniform(-0.8, 0.8, n))
    return (mag * np.exp(1j * ph) * (1 + 0.05 * rng.uniform(-1, 1, n))).astype(c64)


def magnitude_sweep(rng, k_lo=-70, k_hi=60, cycles=3):
    """|x| = 2^k for k = k_lo .. k_hi (exactly: one of the two parts carries the power of two, the other is a random fraction of it), `cycles` times"""
    ks = np.tile(np.arange(k_lo, k_hi + 1), cycles)
    m = np.ldexp(1.0, ks)
    f = rng.uniform(0.1, 0.9, ks.size) * m * rng.choice([-1, 1], ks.size)
    sg = rng.choice([-1, 1], ks.size)
    swap = rng.random(ks.size) < 0.5
    re = np.where(swap, f, sg * m); im = np.where(swap, sg * m, f)
    return (re + 1j * im).astype(c64), ks


# ================================================================== oracle drivers that carry state (the Port methods keep it inside one call)
class _FastAgcState(C.Structure):
    _fields_ = [("buffer_1", C.c_void_p), ("buffer_2", C.c_void_p), ("buffer_input", C.c_void_p), ("peak_1", C.c_float), ("peak_2", C.c_float),
                ("input_size", C.c_int), ("reference", C.c_float), ("last_gain", C.c_float)]


def port_fastagc(port, x, block, reference, state):
    """fastagc_ff over whole blocks of one stream from `state` = the device layout [buffer_1 | buffer_2 | peak_1 peak_2 last_gain pad] -> (y, state after)"""
    x = np.ascontiguousarray(x, f32); nb = x.size // block
    bufs = [np.array(state[:block], f32), np.array(state[block:2 * block], f32), np.zeros(block, f32)]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    st = _FastAgcState(ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), state[2 * block], state[2 * block + 1], block, reference, state[2 * block + 2])
    y = np.zeros(nb * block, f32); ob = np.zeros(block, f32)
    for b in range(nb):
        C.memmove(st.buffer_input, ptr(x[b * block:]), 4 * block)
        port.L.orc_fastagc_ff(C.byref(st), ptr(ob))
        y[b * block:(b + 1) * block] = ob
    out = np.zeros(2 * block + 4, f32)
    by_addr = {a.ctypes.data: a for a in bufs}
    out[:block] = by_addr[st.buffer_1]; out[block:2 * block] = by_addr[st.buffer_2]
    out[2 * block:2 * block + 3] = (st.peak_1, st.peak_2, st.last_gain)
    return y, out


def fastagc_emulate(x, block, reference, state, gain_of_next=False):
    """the same in numpy (the block sequence buffer_1, buffer_2, in_0, in_1 ...: output block j is sequence block j under a gain ramped from g[j] to g[j + 1]).
    gain_of_next: the planted defect -- the ramp of block j ends at the target gain of block j + 1."""
    x = np.ascontiguousarray(x, f32); nb = x.size // block
    seq = np.concatenate([np.asarray(state[:2 * block], f32), x[:nb * block]]).reshape(nb + 2, block)
    pk = np.concatenate([np.asarray(state[2 * block:2 * block + 2], f32), np.abs(seq[2:]).max(axis=1)]).astype(f32)
    with np.errstate(all="ignore"):
        tg = [min(f32(reference) / max(pk[b], pk[b + 1], pk[b + 2]), f32(50)) for b in range(nb)]
    g = [f32(state[2 * block + 2])] + tg
    r = np.arange(block, dtype=f32) / f32(block)
    y = np.empty((nb, block), f32)
    for b in range(nb):
        g1 = g[min(b + 2, nb)] if gain_of_next else g[b + 1]
        y[b] = seq[b] * (f64(g[b]) * (1.0 - r.astype(f64)) + (g1 * r).astype(f64)).astype(f32)
    out = np.zeros(2 * block + 4, f32)
    out[:2 * block] = seq[nb:].ravel(); out[2 * block:2 * block + 3] = (pk[nb], pk[nb + 1], g[nb])
    return y.ravel(), out


class _FracDec(C.Structure):
    _fields_ = [("where", C.c_float), ("input_processed", C.c_int), ("output_size", C.c_int), ("num_poly_points", C.c_int), ("denom", C.c_float * 64),
                ("xifirst", C.c_int), ("xilast", C.c_int), ("rate", C.c_float), ("taps", C.c_void_p), ("taps_length", C.c_int)]


class PortFracdec:
    """one fractional_decimator_ff object of the oracle: call() continues from the state the previous call left"""

    def __init__(self, port, rate, num_poly_points, taps=None, bufsize=0):
        self.port, self.d, self.bufsize = port, _FracDec(), bufsize
        self.taps = None if taps is None else np.ascontiguousarray(taps, f32)
        port.L.orc_fractional_decimator_ff_init(C.byref(self.d), C.c_float(rate), num_poly_points,
                                                None if self.taps is None else self.taps.ctypes.data_as(C.c_void_p), 0 if self.taps is None else self.taps.size)

    @property
    def where(self):
        return self.d.where

    @where.setter
    def where(self, w):
        self.d.where = w

    def _one(self, x):
        x = np.ascontiguousarray(x, f32); y = np.zeros(x.size + 4, f32)
        self.port.L.orc_fractional_decimator_ff(x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), x.size, C.byref(self.d))
        return y[:self.d.output_size].copy(), self.d.input_processed

    def call(self, x):
        """-> (outputs, input_processed): one call over x, or the CLI's loop over bufsize-sample windows when x holds at least one"""
        if not (self.bufsize > 0 and x.size >= self.bufsize):
            return self._one(x)
        outs, base = [], 0
        while base + self.bufsize <= x.size:
            y, p = self._one(x[base:base + self.bufsize])
            outs.append(y)
            if p <= 0:
                break
            base += p
        return np.concatenate(outs), base


def asym_taps(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, n) / np.sqrt(n)).astype(f32)


# ================================================================== the cases both test files run
AGC_SHAPES = [      # (streams, n, block, path of one call over n)
    (1, 255, 64, "k_agc"), (1, 256, 64, "k_agc_coop"), (63, 2049, 1024, "k_agc_coop"), (64, 2049, 1024, "k_agc"), (130, 3000, 1000, "k_agc"),
    (5, 5000, 1000, "k_agc_coop"), (3, 4100, 1, "k_agc_coop"), (2, 3077, 1025, "k_agc_coop"), (3, 2500, 7, "k_agc_coop"),
]
AGC_PARAMS = [      # hang_time, reference, attack_rate, decay_rate, max_gain, attack_wait, filter_alpha
    dict(hang_time=200, reference=0.2, attack_rate=0.01, decay_rate=0.0001, max_gain=65536.0, attack_wait=0, filter_alpha=0.999),
    dict(hang_time=20, reference=0.5, attack_rate=0.05, decay_rate=0.001, max_gain=100.0, attack_wait=5, filter_alpha=0.99),
    dict(hang_time=0, reference=0.2, attack_rate=0.01, decay_rate=0.0001, max_gain=65536.0, attack_wait=0, filter_alpha=0.999),
    dict(hang_time=200, reference=0.2, attack_rate=0.01, decay_rate=0.0001, max_gain=2.0, attack_wait=0, filter_alpha=0.999),
]
AGC_GAINS = (1.0, 0.37, 20.0)


def agc_case(si, pi):
    """-> (x [s, n], initial gains [s], split point of the two-call run)"""
    s, n, block, _ = AGC_SHAPES[si]
    rng = np.random.default_rng(1000 + 10 * si + pi)
    kinds = [(r + si) % 2 for r in range(s)]
    if s > 1:
        kinds[-1] = 2
    x = np.stack([agc_signal(rng, n, block, k) for k in kinds])
    n1 = 2 * n // 5
    if block > 1 and n1 % block == 0:
        n1 += 1
    return x, np.array([AGC_GAINS[r % 3] for r in range(s)], f32), n1


def port_agc(port, x, block, params, gain, restart=True):
    """restart=False: the planted defect -- hang / attack-wait counters and the peak estimate run on across the call edges"""
    if restart:
        return port.agc_ff(x, block=block, last_gain=float(gain), **params)
    return port.agc_ff(x, block=max(x.size, 1), last_gain=float(gain), **params)


DEEMPH_TAUS = [(50e-6, 48000, 1), (50e-6, 240000, 2), (500e-6, 48000, 4), (1e-3, 48000, 8), (2e-3, 48000, 0)]      # (tau, fs, M)
DEEMPH_SHAPES = [(31, 2304), (32, 2304), (1, 2047), (1, 2048), (1, 2049), (2, 16383), (2, 16384), (2, 16385), (2, 32845), (130, 193)]
DEEMPH_STATES = (0.37, np.nan, 1e-40)


def deemph_repair_input(rng, n, kind):
    """|x| ~ 1e-3 with one sample that the run-in cannot forget: 1e30 at the last sample of chunk 2, a NaN mid-stream, or +inf"""
    x = (rng.uniform(-1, 1, n) * 1e-3).astype(f32)
    if kind == "1e30":
        x[3 * DW_L - 1] = 1e30
    elif kind == "nan":
        x[n // 2 + 17] = np.nan
    else:
        x[5 * DW_L + 100] = np.inf
    return x


DC_NS = (1, 31, 32, 33, 8191, 8192, 8193, 20011)
DC_AS = (0.0, 0.5, 0.95, 0.9999)
DC_CASES = [((1, 65, 130)[(i + j) % 3], n, a) for i, n in enumerate(DC_NS) for j, a in enumerate(DC_AS)]


def dc_input(s, n, seed):
    """rows alternate between the DC levels 0.25 and 100; noise, envelope steps and bursts on top"""
    rng = np.random.default_rng(seed)
    x = np.empty((s, n), f32)
    for r in range(s):
        base = (envelope_steps(rng, n), bursts(rng, n), rng.uniform(-1, 1, n).astype(f32))[r % 3]
        x[r] = base + f32(0.25 if r % 2 == 0 else 100.0)
    return x


@functools.lru_cache(maxsize=None)
def dc_case(ci):
    s, n, a = DC_CASES[ci]
    x = dc_input(s, n, 50 + ci)
    x.setflags(write=False)
    y64, B, st, _ = dcblock_f64(x, a)
    return x, y64, B, st


FASTDC_CASES = [(1, 1024, [1, 1, 1, 1]), (70, 1000, [3, 2]), (1, 257, [3, 2]), (70, 255, [1, 1, 1, 1]), (70, 1, [3, 2]), (1, 1, [1, 1, 1, 1]), (70, 1024, [3, 2]), (1, 1000, [1, 1, 1, 1])]

FASTAGC_BLOCKS = (1024, 1000, 1023, 257, 255, 6)
FASTAGC_CALLS = ([1] * 6, [3, 1, 2], [24])
FASTAGC_CASES = [((1, 3, 70)[(i + j) % 3], b, calls) for i, b in enumerate(FASTAGC_BLOCKS) for j, calls in enumerate(FASTAGC_CALLS)]


def fastagc_input(s, block, nb, seed):
    """block 0 silent (with a zero state: peak 0, gain capped at 50), block 1 small, a peak that appears only in block 2, then random levels"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (s, nb * block)).astype(f32)
    lv = np.ones(nb, f32); lv[0] = 0; lv[1:2] = 0.01; lv[2:3] = 5.0
    lv[3:] = rng.choice([0.02, 0.3, 1.0, 4.0], max(nb - 3, 0))
    return x * np.repeat(lv, block)[None, :]


def fastagc_state(s, block, zero, seed):
    st = np.zeros((s, 2 * block + 4), f32)
    if not zero:
        rng = np.random.default_rng(seed)
        st[:, :2 * block] = rng.uniform(-0.5, 0.5, (s, 2 * block))
        st[:, 2 * block] = np.abs(st[:, :block]).max(axis=1); st[:, 2 * block + 1] = np.abs(st[:, block:2 * block]).max(axis=1); st[:, 2 * block + 2] = 3.0
    return st


FRACDEC_CASES = [   # (rate, num_poly_points, prefilter taps, CLI window, path of the first call)
    (5.0, 12, 0, 0, "exact"), (2.5, 2, 33, 0, "exact"), (5.5, 4, 0, 0, "exact"), (2.5, 5, 0, 0, "exact"), (5.0, 20, 33, 0, "exact"),
    (4.17, 12, 33, 0, "walked"), (3.3, 2, 0, 0, "walked"), (1.0001, 4, 0, 0, "walked"), (50.37, 5, 33, 0, "walked"), (4.17, 20, 0, 0, "walked"),
    (3.3, 5, 33, 0, "walked"), (5.5, 12, 33, 1024, "exact"), (4.17, 12, 0, 1024, "walked"), (2.5, 20, 0, 1024, "exact"), (3.3, 4, 33, 1024, "walked"),
]
FRACDEC_CALLS = (3001, 2777)            # the first two calls; the third repeats the second's size from the second's `where`


# ================================================================== float64 forms of fastagc_ff and fractional_decimator_ff
# The kernels restate these two operation for operation and are held to the oracle's bits.  The compiled reference is built with -ffast-math, which reassociates
# the gain ramp and the Lagrange / FIR sums, so it can only be held to a gate; these are the float64 runs and structural bounds of those gates.
def fastagc_f64(x, block, reference, state):
    """-> (y float64, S).  Four roundings sit between the float inputs and an output (the target's division, g1 r, the ramp's sum, the product), all relative to
    the output, and the ramp position r = k / n has its own (an evaluation as k (1 / n) moves it by an ulp), which moves both ramp terms:
    S_i = u (4 |y_i| + 2 |x_i| r_i (|g_j| + |g_j+1|))"""
    x = np.ascontiguousarray(x, f32); nb = x.size // block
    seq = np.concatenate([np.asarray(state[:2 * block], f32), x[:nb * block]]).reshape(nb + 2, block).astype(f64)
    pk = np.concatenate([np.asarray(state[2 * block:2 * block + 2], f64), np.abs(seq[2:]).max(axis=1)])
    with np.errstate(all="ignore"):
        g = [float(state[2 * block + 2])] + [min(float(f32(reference)) / max(pk[b], pk[b + 1], pk[b + 2]), 50.0) for b in range(nb)]
    r = (np.arange(block, dtype=f32) / f32(block)).astype(f64)
    y = np.stack([seq[b] * (g[b] * (1.0 - r) + g[b + 1] * r) for b in range(nb)])
    S = np.stack([U * (4 * np.abs(y[b]) + 2 * np.abs(seq[b]) * r * (abs(g[b]) + abs(g[b + 1]))) for b in range(nb)])
    return y.ravel(), S.ravel() + 2.0 ** -149


def fracdec_positions(n, rate, num_poly_points, taps_length, where, bufsize=0):
    """the reference's float position bookkeeping -> (first input sample of every output's window, fractional position, where after, input_processed)"""
    P = num_poly_points & ~1; xifirst = -(num_poly_points // 2) + 1
    rate = f32(rate); where = f32(where); lo, fr = [], []

    def one(base, size):
        nonlocal where
        while True:
            hi = int(np.ceil(where))
            if not hi + P + taps_length < size:
                break
            lo.append(base + hi - 1); fr.append(f32(where - f32(hi - 1)))
            where = f32(where + rate)
        processed = hi - 1 + xifirst
        where = f32(where - f32(processed))
        return processed
    if bufsize > 0 and n >= bufsize:
        base = 0
        while base + bufsize <= n:
            p = one(base, bufsize)
            if p <= 0:
                break
            base += p
        return np.array(lo, int), np.array(fr, f32), float(where), base
    p = one(0, n)
    return np.array(lo, int), np.array(fr, f32), float(where), p


def fracdec_f64(x, rate, num_poly_points, taps, where, bufsize=0):
    """-> (y float64, S, where after, input_processed).  An output is sum_w c_w f_w: c_w takes P - 1 differences and P - 1 products and a division, f_w a
    taps-long sum of products (T + 1 roundings with its products' own), the result P products and sums: S = (3 P + T + 2) u sum_w |c_w| sum_t |taps_t x|"""
    x = np.asarray(x, f32).astype(f64); P = num_poly_points & ~1; xifirst = -(num_poly_points // 2) + 1
    T = 0 if taps is None else len(taps)
    lo, fr, w_after, proc = fracdec_positions(x.size, rate, num_poly_points, T, where, bufsize)
    if not lo.size:
        return np.zeros(0), np.zeros(0), w_after, proc
    if T:
        t64 = np.asarray(taps, f32).astype(f64)
        idx = lo[:, None, None] + np.arange(P)[None, :, None] + np.arange(T)[None, None, :]
        f = (x[idx] * t64).sum(axis=2); fa = (np.abs(x[idx]) * np.abs(t64)).sum(axis=2)
    else:
        f = x[lo[:, None] + np.arange(P)[None, :]]; fa = np.abs(f)
    xs = np.arange(xifirst, xifirst + P, dtype=f64)
    c = np.empty((lo.size, P))
    for w in range(P):
        others = np.delete(xs, w)
        c[:, w] = np.prod(fr.astype(f64)[:, None] - others[None, :], axis=1) / np.prod(xs[w] - others)
    return (c * f).sum(axis=1), (3 * P + T + 2) * U * (np.abs(c) * fa).sum(axis=1) + 2.0 ** -149, w_after, proc


# ================================================================== references that need live denormals
# The compiled reference library is built with -ffast-math: loading it (the `ref` fixture) switches the whole process to flush-to-zero, after which neither
# numpy nor the oracle can say what the reference does with subnormal values.  These few small references are therefore computed when the module is imported,
# before any fixture runs.
DENORMALS_LIVE = bool(f32(1e-38) * f32(0.5) != 0)


def _deemph_denormal_cases():
    """inputs at 1e-38 (products and states are subnormal throughout) for the run-in kernels M = 1 and M = 8 and for the tiled kernel"""
    cases = []
    for tau, fs, s, n in ((50e-6, 48000, 2, 2304), (1e-3, 48000, 2, 2304), (50e-6, 48000, 3, 193)):
        rng = np.random.default_rng(int(tau * 1e6) + n)
        x = (rng.uniform(-1, 1, (s, n)) * 1e-38).astype(f32)
        last = np.array([1e-40, 0.0, 3e-39][:s], f32)
        alpha = deemph_alpha(tau, fs)
        y = np.stack([deemph_serial(x[r], alpha, last[r])[0] for r in range(s)])
        cases.append((tau, fs, x, last, y))
    return cases


DEEMPH_DENORMAL = _deemph_denormal_cases()
_FM_RNG = np.random.default_rng(77)
FM_SWEEP_X, FM_SWEEP_K = magnitude_sweep(_FM_RNG)
FM_SWEEP_LAST = c64(2.0 ** -71 * (0.6 - 0.8j))
FM_SWEEP_REF = fmdemod_quadri_ref(FM_SWEEP_X, FM_SWEEP_LAST)


# ================================================================== inputs of the demodulator cases (shared, so that the CPU file measures what the GPU file runs)
FM_CASES = [(1, 1, [1]), (130, 1, [1]), (130, 255, [100, 1, 154]), (1, 262145, [262145]), (2, 262145, [1000, 1, 261144])]


def fm_case(s, n):
    """|x| ~ 0.7 with exact zeros planted -> (x [s, n], last [s], the planted positions)"""
    rng = np.random.default_rng(s + n)
    x = np.stack([fm_signal(rng, n) for _ in range(s)])
    zeros = sorted({k for k in (0, 7, 8, 100, n - 1) if 0 <= k < n})
    x[:, zeros] = 0
    return x, np.array([0.3 - 0.4j if r % 2 else 0j for r in range(s)], c64), zeros


ATAN_CASES = [(1, [1]), (256, [256]), (257, [257]), (700, [256, 1, 443])]


def atan_case(n):
    """3 streams: phase steps of exactly +pi and -pi, steps just past pi both ways, (0, 0) samples"""
    rng = np.random.default_rng(n)
    x = np.stack([fm_signal(rng, n) for _ in range(3)])
    if n >= 256:
        x[0, 10] = 1.0; x[0, 11] = -1.0; x[0, 12] = 1.0
        x[1, 10] = np.exp(1j * 0.5 * (np.pi + 1e-3)); x[1, 11] = np.exp(-1j * 0.5 * (np.pi + 1e-3)); x[1, 12] = np.exp(1j * 0.5 * (np.pi + 1e-3))
        x[2, 20:23] = 0
    return x, np.array([0.0, 1.5, -3.0], f32)


N_FLAT_F = 2048 * 1024 + 5            # one length past k_limit's / k_gain's grid cap (2048 blocks of 256 float4 lanes)
N_FLAT_C = 4096 * 256 + 3             # and past k_cf_to_f's (4096 blocks of 256)


def flat_f_input():
    x = np.random.default_rng(3).uniform(-3, 3, N_FLAT_F).astype(f32)
    x[:6] = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0]; x[-3:] = [np.nan, -np.inf, -0.0]
    return x


def flat_c_input():
    rng = np.random.default_rng(4)
    return (fm_signal(rng, N_FLAT_C) * np.exp(rng.uniform(-12, 6, N_FLAT_C))).astype(c64)       # magnitudes over 8 decades
