"""Model of squelch_and_smeter_cc (csdr.c:2192-2243) and get_power_c / get_power_f (libcsdr.c:1144-1162): the float64 power, the gate every float32
evaluation has to pass, the library's own summation order in numpy float32, the block stream with its levels, the report schedule as a literal replay of
the reference's counter, the test vectors, and a ctypes loader for the reference library.

The gate.  The n = ceil(B / d) terms (i*i + q*q) / B are non-negative.  A float32 evaluation in any order performs n - 1 additions and at most a handful
of roundings per term (two products, their sum, the division or a multiplication by a rounded reciprocal), each a relative error of at most 2^-24 on a
partial result that is at most the exact power P: it lies within (n + 8) 2^-24 P of P.  The reference (built with -ffast-math: vectorised sum, reciprocal
multiplication), the library (512 chains by sample index, then a pairwise tree) and this model are all held to it."""
import ctypes as C
import os
import numpy as np

f32 = np.float32
c64 = np.complex64
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")
U = 2.0 ** -24
CHAINS = 512


def n_terms(B, d):
    return -(-B // d)


def power64(x, d=1):
    """the exact power of one block (complex or real): sum over samples 0, d, 2d, .. of |x|^2 / B in float64"""
    x = np.asarray(x)
    v = x[::d]
    if np.iscomplexobj(x):
        t = v.real.astype(np.float64) ** 2 + v.imag.astype(np.float64) ** 2
    else:
        t = v.astype(np.float64) ** 2
    return float(t.sum() / x.size)


def bound(B, d, P):
    """the gate on |P32 - P| for any float32 evaluation"""
    return (n_terms(B, d) + 8) * U * abs(P)


def undecidable(B, d, P, level):
    return abs(P - level) <= bound(B, d, P)


def terms32(x):
    """(i*i + q*q) / B (or x*x / B), every operation rounded to float32"""
    x = np.asarray(x)
    fB = f32(x.size)
    if np.iscomplexobj(x):
        x = x.astype(c64)
        i, q = x.real.astype(f32), x.imag.astype(f32)
        return ((i * i + q * q).astype(f32) / fB).astype(f32)
    x = x.astype(f32)
    return ((x * x).astype(f32) / fB).astype(f32)


def power32(x, d=1):
    """the library's order: chain c = the terms of the samples s with s mod 512 == c in increasing s (samples with s mod d != 0 add nothing), then
    chain[c] += chain[c + h] for h = 256 .. 1"""
    with np.errstate(all="ignore"):
        t = terms32(x)
        B = t.size
        keep = (np.arange(B) % d) == 0
        rows = -(-B // CHAINS)
        tt = np.zeros(rows * CHAINS, f32)
        tt[:B] = np.where(keep, t, f32(0))
        kk = np.zeros(rows * CHAINS, bool)
        kk[:B] = keep
        tt, kk = tt.reshape(rows, CHAINS), kk.reshape(rows, CHAINS)
        chain = np.zeros(CHAINS, f32)
        for r in range(rows):
            chain = np.where(kk[r], (chain + tt[r]).astype(f32), chain)
        h = CHAINS // 2
        while h >= 1:
            chain = (chain[:h] + chain[h:2 * h]).astype(f32)
            h //= 2
        return f32(chain[0])


def power32_seq(x, d=1):
    """the reference's source order: one sequential float32 chain"""
    t = terms32(x)[::d]
    return f32(np.cumsum(t, dtype=f32)[-1]) if t.size else f32(0)


def gate_open(power, level):
    """csdr.c:2230 (a NaN power closes the gate unless the level is 0)"""
    return bool(f32(level) == 0 or f32(power) >= f32(level))


def stream(x, B, d, level, changes=None, power=power32):
    """squelch_and_smeter_cc over the whole blocks of x.  level: the first level; changes: {k: new level read behind block k's output}, in force from
    block k + 1 on (csdr.c:2240).  -> (out, powers, flags)"""
    x = np.asarray(x, c64)
    nb = x.size // B
    out = np.zeros(nb * B, c64)
    pw, fl = np.zeros(nb, f32), np.zeros(nb, np.uint8)
    for k in range(nb):
        blk = x[k * B:(k + 1) * B]
        pw[k] = power(blk, d)
        fl[k] = gate_open(pw[k], level)
        if fl[k]:
            out[k * B:(k + 1) * B] = blk
        if changes and k in changes:
            level = changes[k]
    return out, pw, fl


def report_replay(report_every_nth, n_blocks):
    """a literal replay of csdr.c:2202, 2224-2226: the 0-based blocks that write a report line"""
    due, report_cntr = [], 0
    for k in range(n_blocks):
        c = report_cntr
        report_cntr += 1
        if c > report_every_nth:
            report_cntr = 0
            due.append(k)
    return due


def report_due(report_every_nth, k):
    return k % (report_every_nth + 2) == report_every_nth + 1


# ---------------------------------------------------------------- vectors
def noise_blocks(rng, n_blocks, B, powers):
    """complex Gaussian blocks scaled so that block k's float64 power (d = 1) is powers[k] up to the float32 rounding of its samples"""
    x = (rng.standard_normal((n_blocks, B)) + 1j * rng.standard_normal((n_blocks, B)))
    p = (np.abs(x) ** 2).mean(axis=1)
    x *= np.sqrt(np.asarray(powers, np.float64) / p)[:, None]
    return x.astype(c64).reshape(-1)


def two_class(rng, n_blocks, B, level=1e-3, ratio_db=6.0):
    """block powers in two classes, each at least ratio_db / 2 away from the level on its side: none undecidable"""
    r = 10 ** (ratio_db / 20)
    cls = rng.integers(0, 2, n_blocks)
    powers = np.where(cls == 1, level * r * rng.uniform(1.0, 4.0, n_blocks), level / r * rng.uniform(0.05, 1.0, n_blocks))
    return noise_blocks(rng, n_blocks, B, powers), cls.astype(np.uint8)


def near_threshold(rng, n_blocks, B, level=1e-3, spread=0.01):
    """block powers uniform over level (1 +- spread)"""
    return noise_blocks(rng, n_blocks, B, level * (1 + spread * rng.uniform(-1, 1, n_blocks)))


# ---------------------------------------------------------------- the reference library through ctypes
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ref_lib():
    if not os.path.exists(REF_LIB):
        return None
    L = C.CDLL(REF_LIB)
    L.get_power_c.restype = C.c_float
    L.get_power_c.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.get_power_f.restype = C.c_float
    L.get_power_f.argtypes = [C.c_void_p, C.c_int, C.c_int]
    return L


def ref_power(L, x, d=1):
    """get_power_c / get_power_f of a library with the reference's prototypes (the reference, or the drop-in symbols)"""
    if np.iscomplexobj(x):
        x = np.ascontiguousarray(x, c64)
        return f32(L.get_power_c(_p(x), x.size, d))
    x = np.ascontiguousarray(x, f32)
    return f32(L.get_power_f(_p(x), x.size, d))


def ref_stream(L, x, B, d, level, changes=None):
    """the reference's loop with its own get_power_c, block by block"""
    return stream(x, B, d, level, changes, power=lambda blk, dd: ref_power(L, blk, dd))
