"""A numpy float32 model of the shared-rate shifters (csdr_amd/csrc/shift.hip): the rotator sequence of each of the five variants as
csdr_amd_rotator_generate defines it, the two mixing kernels, the decimating shifter, and the set of samples whose device sin / cos may round to the
other float (exempt).  One float32 operation per reference operation, in the reference's order; cos and sin are libm's double functions rounded to
float32.  The primitives (wraps, increments, the chunk step, the per-sample rotator of MATH / TABLE) are shiftbank_model's.  The chunked variants are
vectorised across chunks -- chunks are independent once their start phases are known -- and the per-sample scan of MATH / TABLE is a Python loop.

CASES, MIX and DSA list what tests/test_shift_gpu.py runs on the device; tests/test_shift_cpu.py walks the same lists against the C oracle."""
import functools
import numpy as np
import shiftbank_model as M

f32, c64, ld = np.float32, np.complex64, np.longdouble
PI, TWO_PI = M.PI, M.TWO_PI
Q90 = f32(PI / f32(2))
CHUNKED = ("addition", "addfast", "unroll")
VARIANTS = ("addition", "math", "table", "unroll", "addfast")
BAND = 1024                                              # double ulps around a float rounding tie inside which host and device may round apart


def fcos_all(p): return np.array([M.fcos(v) for v in np.atleast_1d(p)], f32)
def fsin_all(p): return np.array([M.fsin(v) for v in np.atleast_1d(p)], f32)


def cplx(re, im):
    """two float32 planes -> complex64, no arithmetic"""
    out = np.empty(np.shape(re), c64)
    out.real, out.imag = re, im
    return out


def chunk_phases(rate, phase, n, chunk):
    """the start phase of every chunk of n samples and the phase after the last one: p <- wrap_pm_pi(p + inc * len)"""
    p, out = f32(phase), []
    for pos in range(0, n, chunk):
        out.append(p)
        p = M.advance(p, rate, min(chunk, n - pos))
    return np.array(out, f32), p


def unroll_angles(rate, size):
    """shift_unroll_init's table angles: entry k is k + 1 increments, accumulated and wrapped in float"""
    inc, a, out = M.inc_of(rate), f32(0), []
    for _ in range(size):
        a = M.wrap_pm_pi(f32(a + inc))
        out.append(a)
    return np.array(out, f32)


@functools.lru_cache(maxsize=None)
def _stepper(variant, size):
    """shiftbank_model's per-sample rotator of MATH / TABLE (the quarter table is built once per size)"""
    return M.ShiftModel(variant, 0.0, table_size=size)


@functools.lru_cache(maxsize=64)
def scan(rate, phase, n):
    """MATH / TABLE: the phase of every sample and the phase after the last: p <- wrap_0_2pi(p + inc) per sample"""
    inc, p, out = M.inc_of(rate), f32(phase), np.empty(n, f32)
    for k in range(n):
        out[k] = p
        p = M.wrap_0_2pi(f32(p + inc))
    out.setflags(write=False)
    return out, p


def table_size(aux): return aux if aux > 0 else 65536
def unroll_size(chunk, aux): return aux if aux > 0 else chunk


def rot(variant, rate, phase, n, chunk=1024, aux=0, table=None):
    """-> (rot [n] complex64, end phase) as csdr_amd_rotator_generate writes them.  table: another quarter table for TABLE (exempt uses it)"""
    if variant in ("math", "table"):
        ph, end = scan(float(rate), float(phase), n)
        m = _stepper(variant, table_size(aux) if variant == "table" else 16)
        if table is not None:
            m = M.ShiftModel("math", 0.0); m.variant, m.table = "table", table
        c, s = np.empty(n, f32), np.empty(n, f32)
        for k in range(n):
            c[k], s[k] = m._rot(ph[k])
        return cplx(c, s), end
    starts, end = chunk_phases(rate, phase, n, chunk)
    nch, inc = starts.size, M.inc_of(rate)
    c0, s0 = fcos_all(starts), fsin_all(starts)
    c, s = np.ones((nch, chunk), f32), np.zeros((nch, chunk), f32)
    if variant == "addition":
        sd, cd = M.fsin(inc), M.fcos(inc)
        for k in range(min(chunk, n)):
            c[:, k], s[:, k] = c0, s0
            c0, s0 = c0 * cd - s0 * sd, s0 * cd + c0 * sd
    elif variant == "addfast":
        dsin = [M.fsin(f32(inc * f32(j + 1))) for j in range(4)]; dcos = [M.fcos(f32(inc * f32(j + 1))) for j in range(4)]
        for g in range(min(chunk, n) // 4):
            for j in range(4):
                c[:, 4 * g + j], s[:, 4 * g + j] = c0 * dcos[j] - s0 * dsin[j], s0 * dcos[j] + c0 * dsin[j]
            c0, s0 = c[:, 4 * g + 3].copy(), s[:, 4 * g + 3].copy()
        last = n - (nch - 1) * chunk                   # the last chunk's own length: its groups of four end sooner, the rest is 1 + 0j
        c[-1, last // 4 * 4:], s[-1, last // 4 * 4:] = 1, 0
    else:
        ang = unroll_angles(rate, unroll_size(chunk, aux))[:chunk]
        dsin, dcos = fsin_all(ang), fcos_all(ang)
        c = c0[:, None] * dcos[None, :] - s0[:, None] * dsin[None, :]
        s = s0[:, None] * dcos[None, :] + c0[:, None] * dsin[None, :]
    return cplx(c.ravel()[:n], s.ravel()[:n]), end


def addfast_written(n, chunk):
    """the samples shift_addfast_cc writes: all but each chunk's len % 4 tail"""
    w = np.zeros(n, bool)
    for pos in range(0, n, chunk):
        ln = min(chunk, n - pos)
        w[pos:pos + ln // 4 * 4] = True
    return w


def mix_cc(x, r):
    """out = x * rot with four float32 products and two float32 sums, x [n] or [streams, n]"""
    xr, xi, c, s = x.real.astype(f32), x.imag.astype(f32), r.real.astype(f32), r.imag.astype(f32)
    return cplx(c * xr - s * xi, s * xr + c * xi)


def mix_fc(x, r):
    """real input: (rot.i * x, rot.q * x)"""
    x = np.asarray(x, f32)
    return cplx(r.real.astype(f32) * x, r.imag.astype(f32) * x)


def dsa(x, rate, decimation, status=(0, 0.0, 0)):
    """decimating_shift_addition_cc (k_dsa / libcsdr_gpl.c:131-160): x [n], one rate, status (remain, phase, produced) -> (y, status); or x [streams, n],
    a rate and a status per stream -> ([streams] arrays, [streams] statuses), vectorised across the streams (which share `remain`: one history)"""
    if np.ndim(x) == 1:
        ys, sts = dsa(np.asarray(x)[None], [rate], decimation, [status])
        return ys[0], sts[0]
    x = np.asarray(x, c64)
    streams, n = x.shape
    remain = status[0][0]
    assert all(st[0] == remain for st in status)
    phase = np.array([st[1] for st in status], f32)
    rate2 = np.array([f32(f32(f32(r) * f32(decimation)) * f32(2)) for r in rate], f32)     # decimating_shift_addition_init: shift_addition_init(rate * decimation)
    inc = rate2 * PI
    sd, cd = fsin_all(inc), fcos_all(inc)
    c, s = fcos_all(phase), fsin_all(phase)
    xr, xi = x.real.astype(f32), x.imag.astype(f32)
    cols, pos = [], remain
    while pos < n:
        cols.append(cplx(c * xr[:, pos] - s * xi[:, pos], s * xr[:, pos] + c * xi[:, pos]))
        c, s = c * cd - s * sd, s * cd + c * sd
        pos += decimation
    k = len(cols)
    y = np.stack(cols, 1) if k else np.zeros((streams, 0), c64)
    end = [M.wrap_pm_pi(f32(phase[j] + f32(inc[j] * f32(k)))) for j in range(streams)]
    return [y[j] for j in range(streams)], [(pos - n, end[j], k) for j in range(streams)]


def near_tie(x, fn):
    """which of fn(x) (np.sin or np.cos of the float32 values x, taken in long double) lie within BAND double ulps of the midpoint of two neighbouring
    floats: there, and only there, two correctly working double functions may round to different floats"""
    x = np.atleast_1d(np.asarray(x, f32))
    v = fn(x.astype(ld))
    f = v.astype(f32)
    d = np.full(x.shape, np.inf, ld)
    for side in (np.inf, -np.inf):
        mid = (f.astype(ld) + np.nextafter(f, f32(side)).astype(ld)) / 2
        d = np.minimum(d, np.abs(v - mid))
    return d <= BAND * np.spacing(np.abs(v).astype(np.float64)).astype(ld)


def near_tie_any(x): return near_tie(x, np.sin) | near_tie(x, np.cos)


def quarter_angles(size):
    """the float angles k_quarter_table takes the sine of"""
    return np.array([f32(f32(f32(k) / f32(size)) * Q90) for k in range(size)], f32)


def exempt(variant, rate, phase, n, chunk=1024, aux=0):
    """-> bool [n]: the samples that depend on a device sin / cos evaluation next to a rounding tie.  MATH: the sample's own phase; TABLE: the quarter
    table entries it reads; the chunked variants: the chunk's start phase, and for UNROLL the table angle of its place in the chunk."""
    if variant == "math":
        return near_tie_any(scan(float(rate), float(phase), n)[0])
    if variant == "table":
        size = table_size(aux)
        marked = near_tie(quarter_angles(size), np.sin)
        if not marked.any():
            return np.zeros(n, bool)
        poisoned = _stepper("table", size).table.copy()
        poisoned[marked] = np.nan                      # whatever reads a marked entry comes out NaN
        r, _ = rot("table", rate, phase, n, chunk, aux, table=poisoned)
        return np.isnan(r.real) | np.isnan(r.imag)
    starts, _ = chunk_phases(rate, phase, n, chunk)
    e = np.repeat(near_tie_any(starts), chunk)[:n]
    if variant == "unroll":
        e = e | np.tile(near_tie_any(unroll_angles(rate, unroll_size(chunk, aux))[:chunk]), starts.size)[:n]
    return e


def ulps_apart(a, b):
    """float32 arrays -> how many floats lie between them (sign-magnitude words mapped to a line)"""
    def line(v):
        w = np.ascontiguousarray(v, f32).view(np.int32).astype(np.int64)
        return np.where(w < 0, -(w & 0x7FFFFFFF), w)
    return np.abs(line(a) - line(b))


# ---------------------------------------------------------------------------------------------------------------- what the GPU file runs
RATES = M.RATES
LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2 * 1024 + 17]
CHUNKS = [1024, 1000, 100, 7]


def _neighbours(v):
    v = f32(v)
    return [np.nextafter(v, f32(-np.inf)), v, np.nextafter(v, f32(np.inf))]


PHASES = [f32(0), f32(0.1), f32(-3.0), PI, f32(-PI), TWO_PI] + [p for k in (1, 2, 3) for p in _neighbours(f32(k) * Q90)] + [f32(7.0), f32(-7.0)]


def _cases():
    """(variant, rate, phase, n, chunk, aux): every length, chunk, rate and start phase meets every variant at least once (two passes with other strides,
    so that the pairs differ), then the cases that stand alone"""
    out = []
    for v, variant in enumerate(VARIANTS):
        for i in range(2 * len(PHASES)):
            n = LENGTHS[(i + v) % len(LENGTHS)]
            rate = RATES[(i + i // len(RATES) + v) % len(RATES)]
            phase = PHASES[(5 * i + v) % len(PHASES)]
            chunk = CHUNKS[(i + i // len(CHUNKS)) % len(CHUNKS)] if variant in CHUNKED else 1024
            aux = 0
            if variant == "table": aux = (65536, 16)[i % 2]
            if variant == "unroll": aux = (chunk, chunk + 24, 0)[i % 3]            # aux == chunk, aux > chunk, and the default (= chunk)
            out.append((variant, rate, phase, n, chunk, aux))
    # the command line's chunk.  UNROLL at another rate: at -0.085 one of its 16384 table angles has a sine next to a rounding tie (exempt), which a
    # chunked case must not have (tests/test_shift_cpu.py asserts it)
    for variant, rate in zip(CHUNKED, (-0.085, -0.085, 0.3141)):
        out.append((variant, rate, f32(0.1), 16384 + 5, 16384, 0))
    out.append(("unroll", 0.3141, f32(-3.0), 2 * 1024 + 17, 1000, 1024))
    return out


CASES = _cases()


def case_id(case):
    variant, rate, phase, n, chunk, aux = case
    return "%s-rate%g-phase%.9g-n%d-chunk%d-aux%d" % (variant, rate, float(phase), n, chunk, aux)


# the mixing kernels' cases share one rotator recipe; the mixed output is compared with mix_cc / mix_fc of the model's rotator
MIX_ROT = ("addition", -0.085, f32(0.1), 1024, 0)       # (variant, rate, phase, chunk, aux)
MIX_LENGTHS = [1, 4099, 4100, 4102, 4103, 512 * 256 + 257]


def mix_rot(n):
    variant, rate, phase, chunk, aux = MIX_ROT
    return rot(variant, rate, phase, n, chunk, aux)


# ShiftAhead: (variant, rate, n, the phase the caller sets or None for the one handed back, whether the call finds its scan done).  The rule of
# csdr_amd_rotator_generate: a call finds its scan done if the call before it on the context (MATH or TABLE, either) had the same rate and the same n and
# handed back the phase this call comes with.
def ahead_calls(first, other):
    return [(first, -0.085, 4096, f32(0.1), False),      # the first call: nothing was scanned ahead
            (first, -0.085, 4096, None, True),
            (first, -0.085, 4096, None, True),
            (first, -0.085, 1000, None, False),          # another length
            (first, -0.085, 1000, None, True),
            (first, 0.3141, 1000, None, False),          # another rate
            (first, 0.3141, 1000, f32(1.25), False),     # the caller changed the phase
            (other, 0.3141, 1000, None, True)]           # the other variant reads the same scan


# k_dsa: a rate and a start phase per stream; (streams, decimation, input_size, calls)
DSA = [(1, 1, 301, 2), (64, 3, 301, 2), (65, 7, 301, 2), (130, 3, 301, 2), (130, 1, 64, 1), (65, 100, 37, 6)]


def dsa_rate(s): return f32(0.0173 * (s + 1) / 13 - 0.09)
def dsa_phase(s): return f32(-3.0 + 0.046 * s)


def ahead_cases(first, other):
    """the calls of the ShiftAhead sequence as rotator cases: each starts from the phase the call before it handed back, or the one the caller sets"""
    out, p = [], None
    for variant, rate, n, phase, _ in ahead_calls(first, other):
        p = p if phase is None else phase
        out.append((variant, rate, f32(p), n, 1024, 0))
        p = scan(float(rate), float(p), n)[1]
    return out


# ADDFAST's tails: chunk 7 leaves three samples of every chunk unwritten, chunk 1000 only the ragged end's one
TAIL_CASES = [("addfast", 0.3141, f32(-3.0), 2 * 1024 + 17, chunk, 0) for chunk in (7, 1000)]
