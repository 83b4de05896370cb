"""Inputs, parameter sets and oracle compositions of the AM / SSB receive chain's tests (csdr_amd_amssb_*, amssb.hip).

The design never compares across agc_ff on unequal inputs: `pre_agc` (what goes into agc_ff) is compared with the oracle's demodulator stages, and the stages
from agc_ff on are compared on the library's own `pre_agc`, the same input on both sides, bit for bit."""
import numpy as np

import audio_model as am

f32, f64, c64 = np.float32, np.float64, np.complex64

# agc_ff's arguments in `csdr agc_ff`'s order: hang_time, reference, attack_rate, decay_rate, max_gain, attack_wait, filter_alpha
AGC_DEFAULT = (200, 0.2, 0.01, 0.0001, 65536.0, 0, 0.999)                 # csdr.c:1342-1361
AGC_ALT = (20, 0.5, 0.05, 0.001, 100.0, 5, 0.99)
AGC_SETS = {"default": AGC_DEFAULT, "alt": AGC_ALT}
GATE_AM = 1e-6                                                            # the project's gate for block-wise float audio (test_gpu_parity.py:239)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    differ = bits(got).ravel() != bits(want).ravel()
    if got.dtype.kind == "f":           # a NaN equals a NaN: IEEE 754 leaves the sign and payload of a NaN that an operation generates to the implementation
        differ &= ~(np.isnan(got).ravel() & np.isnan(want).ravel())      # (inf - inf is 0xffc00000 from x86 SSE and 0x7fc00000 from gfx950)
    bad = np.flatnonzero(differ)
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: %r against %r" % (what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


INPUT_KINDS = ("steps", "steps_zero_runs", "zeros", "envelope_steps", "zero_runs", "bursts", "inf_nan")


def real_signal(kind, n, block, seed):
    rng = np.random.default_rng(seed)
    if kind == "steps":
        return am.agc_signal(rng, n, block, 0)
    if kind == "steps_zero_runs":
        return am.agc_signal(rng, n, block, 1)
    if kind == "zeros":
        return am.agc_signal(rng, n, block, 2)
    if kind == "envelope_steps":
        return am.envelope_steps(rng, n)
    if kind == "zero_runs":
        return am.with_zero_runs(am.envelope_steps(rng, n, 50), ((0, 3), (block - 1, 2), (n // 2, block // 2)))
    if kind == "bursts":
        return am.bursts(rng, n)
    if kind == "inf_nan":                                                  # finite up to the last two blocks
        x = am.agc_signal(rng, n, block, 0)
        x[n - 2 * block + 5] = np.inf; x[n - 2 * block + 9] = -np.inf; x[n - block + 3] = np.nan
        return x
    raise ValueError(kind)


def complex_input(mode, kind, n, block, seed):
    """SSB: the real signal with an unrelated imaginary part.  AM: the real signal under a rotating carrier, so that the envelope is its magnitude (with a
    pedestal for the finite kinds, as an AM carrier has one: the DC block has something to take away)."""
    r = real_signal(kind, n, block, seed).astype(f64)
    rng = np.random.default_rng(seed + 1000)
    if mode == "ssb":
        return (r + 1j * rng.uniform(-1, 1, n)).astype(c64)
    ped = 0.0 if kind in ("zeros", "zero_runs", "steps_zero_runs") else 0.5
    ph = np.exp(2j * np.pi * (0.013 * np.arange(n) + rng.uniform()))
    with np.errstate(invalid="ignore"):
        x = ((np.abs(r) + ped) * ph)
    x = x.astype(c64)
    bad = ~np.isfinite(r)
    x[bad] = (r[bad] + 0j).astype(c64)                                      # Inf and NaN as they are, in the in-phase part
    return x


def finite_blocks(x, block):
    """the number of leading whole blocks of x without an Inf or NaN"""
    nb = x.size // block
    ok = np.isfinite(x[:nb * block].view(f32).reshape(nb, 2 * block)).all(axis=1)
    return nb if ok.all() else int(np.argmin(ok))


def oracle_pre_agc(lib, mode, x, block):
    """what the oracle's (or the compiled reference's) stages in front of agc_ff give for the whole blocks of x"""
    n = x.size // block * block
    if mode == "ssb":                                                      # (csdr.c:634-645 is a copy loop of the CLI: the compiled reference library has none)
        return lib.realpart_cf(x[:n]) if hasattr(lib, "realpart_cf") else np.ascontiguousarray(x[:n].real)
    return lib.fastdcblock_ff(lib.amdemod_cf(x[:n]), block)[0]


def f64_pre_agc_am(x, block):
    n = x.size // block * block
    env, _ = am.amdemod_f64(x[:n])
    y, _, _ = am.fastdcblock_f64(env.astype(f32), block, [0.0])           # the envelope as floats, as every implementation stores it
    return y[0], env


def oracle_tail(lib, pre, block, agc, limit_max=1.0, last_gain=1.0):
    """agc_ff | limit_ff | convert_f_s16 of the oracle on `pre` -> (s16, last_gain)"""
    y, g = lib.agc_ff(pre, block, *agc, last_gain=last_gain)
    return lib.convert_f_s16(lib.limit_ff(y, limit_max)), g


def relrms_to(got, want, scale):
    d = np.asarray(got, f64) - np.asarray(want, f64)
    return float(np.sqrt(np.mean(d * d)) / max(np.sqrt(np.mean(np.asarray(scale, f64) ** 2)), 1e-300))


def am_test_signal(n, seed=15, carrier=0.25, n_ch=1):
    """the AM signal of test_cli_am_and_ssb_chains as u8 IQ, [n_ch, 2n]: a 700 Hz tone at 50 % depth on a carrier at `carrier`, noise per channel"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    audio = 0.5 * np.sin(2 * np.pi * 700 / 2.4e6 * t)
    carrier = np.broadcast_to(np.asarray(carrier, f64), (n_ch,))
    out = np.empty((n_ch, 2 * n), np.uint8)
    for c in range(n_ch):
        sig = 0.5 * (1 + audio) * np.exp(2j * np.pi * carrier[c] * t) + 0.01 * (rng.normal(size=n) + 1j * rng.normal(size=n))
        iq = np.empty(2 * n, f32); iq[0::2] = sig.real; iq[1::2] = sig.imag
        out[c] = np.clip(np.round(127.5 * (iq + 1)), 0, 255).astype(np.uint8)
    return out
