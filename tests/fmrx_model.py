"""What the FM receive bank's tests share (csdr_amd_fmrx, csdr_amd/csrc/fmrx.hip): the inputs, the expected values and the gates.

Inputs are complex baseband at the audio rate, one kind per channel (KINDS, channel k gets KINDS[k % 4]):
  fm      tests/test_gpu_parity.py's fm_signal at the audio rate: a 1 kHz tone plus noise, deviation 5 kHz at 48 kS/s, amplitude 0.7, channel noise 0.01
  zeros   the same with two runs of exact (0, 0) samples, ZERO_RUNS: the demodulator's `den == 0` branch.  The first run crosses sample 341 (the first cut of
          the tests' ragged calls), the second sample 3072 (the end of the third call when a call is one block)
  limit   the same with two stretches (LIMIT_RUNS) in which the limiter sits at +limit and then at -limit, so the digits reach full scale +-8355711.  Deviation
          alone cannot do that at the default limit of 1: the demodulator gives Kf |p| / |x| sin(dphi) with Kf = 0.34, so in these stretches the phase steps by
          +-pi/2 AND the amplitude falls to a quarter from sample to sample: Kf * 4 = 1.36 > 1
  agc     an unmodulated carrier for the first AGC_SILENT samples (three blocks of 1024: the de-emphasised blocks 0 .. 2 hold the filter's zero prefix and
          channel noise only, fastagc's gain sits at its clamp of 50), then the fm signal, which the end of block 3 sees: the gain ramps down over the block
          that has the loud one two ahead

Expected values: the oracle's stages in turn, port.fmdemod_quadri_cf, limit_ff, deemphasis_nfm_ff_cli(x, taps), fastagc_ff(block, reference), convert_f_s16.
Gates (the project's own for this chain, tests/test_gpu_parity.py::test_nfm_chain_device_resident): float audio relrms <= 1e-5; s16 at most 1 LSB apart on fewer
than 5 % of the samples; the first 2 * agc_block samples exactly 0; the length is the oracle's whole blocks."""
import ctypes as C

import numpy as np

c64 = np.complex64
f32 = np.float32

RATES = (48000, 44100, 8000, 11025)
KINDS = ("fm", "zeros", "limit", "agc")
PREFIX = 1024
ZERO_RUNS = ((300, 400), (3042, 3122))
LIMIT_RUNS = ((1500, 1520, +1), (1540, 1560, -1), (4700, 4724, -1), (4740, 4764, +1))
AGC_SILENT = 3 * 1024
TOL = 1e-5


def taps_of(rate):
    """the de-emphasis taps of csdr_amd_nfm_deemph_taps (a host table: no GPU)"""
    import csdr_amd
    p = C.c_void_p()
    n = csdr_amd.lib().csdr_amd_nfm_deemph_taps(int(rate), C.byref(p))
    assert n > 0, rate
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (n,)).copy()


def fm_baseband(rng, n, dev=5e3 / 48e3, silent=0):
    t = np.arange(n)
    msg = np.sin(2 * np.pi * 1e3 / 48e3 * t) + 0.3 * rng.uniform(-1, 1, n)
    msg[:silent] = 0.0
    ph = 2 * np.pi * np.cumsum(dev * msg)
    return 0.7 * np.exp(1j * ph) + 0.01 * (rng.normal(size=n) + 1j * rng.normal(size=n))


def channel(kind, seed, n):
    """one channel of `kind`, n samples, complex64"""
    rng = np.random.default_rng(seed)
    x = fm_baseband(rng, n, silent=AGC_SILENT if kind == "agc" else 0)
    if kind == "zeros":
        for a, b in ZERO_RUNS:
            x[a:b] = 0
    if kind == "limit":
        for a, b, sign in LIMIT_RUNS:
            if b <= n:
                k = np.arange(b - a)
                x[a:b] = x[a - 1] * 0.25 ** (k + 1) * np.exp(sign * 0.5j * np.pi * (k + 1))
    return x.astype(c64)


def make_input(n_channels, n, seed=0):
    """[n_channels, n] complex64, channel k of kind KINDS[k % 4]"""
    return np.stack([channel(KINDS[k % len(KINDS)], 7000 + 131 * seed + k, n) for k in range(n_channels)])


def n_for_blocks(blocks, taps_length, block=1024, extra=37):
    """input samples after which a fresh object has written `blocks` blocks (and holds taps_length - 1 + extra samples short of the next)"""
    return blocks * block + taps_length - PREFIX + extra


def plan(fill, n_in, taps_length, block):
    """csdr_amd_fmrx_plan restated: (samples written per channel, samples held afterwards)"""
    ne = max(fill + n_in - taps_length, 0) // block * block if n_in else 0           # (a call without input does nothing)
    return ne, fill + n_in - ne


def limited(port, x, limit=1.0):
    """the oracle's limited demodulator output of one channel"""
    dem, _ = port.fmdemod_quadri_cf(x)
    return port.limit_ff(dem, limit)


def expected(port, x, taps, block=1024, reference=1.0, limit=1.0):
    """the oracle's chain on one channel -> (s16, float audio)"""
    de = port.deemphasis_nfm_ff_cli(limited(port, x, limit), taps)
    agc = port.fastagc_ff(de, block, reference)
    return port.convert_f_s16(agc), agc


def deemph_tiles(rate, lim, taps_length, block=1024, limit=1.0):
    """the de-emphasis of (1024 zeros ++ lim) for whole blocks through csdr_amd_debug_nfm_deemph_tile, 16 outputs at a time: the kernels' fixed-point arithmetic
    on the host"""
    import csdr_amd
    fn = csdr_amd.lib().csdr_amd_debug_nfm_deemph_tile
    fn.argtypes = [C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    ne, _ = plan(PREFIX, lim.size, taps_length, block)
    padded = np.concatenate([np.zeros(PREFIX, f32), np.ascontiguousarray(lim, f32), np.zeros(256, f32)])
    out = np.zeros(ne, f32)
    for o in range(0, ne, 16):
        w = np.ascontiguousarray(padded[o:o + 256])
        assert fn(int(rate), float(limit), w.ctypes.data, out[o:o + 16].ctypes.data) == 0
    return out


def gate_figures(s16, af, want_s16, want_af, block=1024):
    """(relrms of the float audio, largest s16 difference, fraction of s16 samples that differ); lengths and the two zero blocks are asserted here"""
    from oracle import relrms
    assert af.shape == want_af.shape and s16.shape == want_s16.shape, (af.shape, want_af.shape)
    assert want_af.size >= 2 * block and want_af.size % block == 0
    assert np.all(af[:2 * block] == 0) and np.all(s16[:2 * block] == 0)
    d = np.abs(s16.astype(np.int32) - want_s16.astype(np.int32))
    return relrms(af, want_af), int(d.max()), float((d > 0).mean())


def assert_gates(s16, af, want_s16, want_af, block=1024, what=""):
    r, dmax, frac = gate_figures(s16, af, want_s16, want_af, block)
    print("%s: relrms %.3g, s16 max diff %d, differing %.3f %%" % (what, r, dmax, 100 * frac))
    assert r <= TOL, (what, r)
    assert dmax <= 1 and frac < 0.05, (what, dmax, frac)


def bank_composition(ctx, x, tbw, decimation, rates, per, retunes=None, resets=None):
    """ctx.fastddc_bank -> FmRx with `per` blocks per call; retunes {call: [(channel, rate), ...]} and resets {call: [channel, ...]} are applied in front of that
    call -> the s16 audio of every call, [n_channels, count] each"""
    import csdr_amd
    y = ctx.fastddc_bank(x, tbw, decimation, rates, blocks_per_call=per, retunes=retunes)
    assert all(np.all(c == c[0]) for c in ctx.ddc_call_counts)           # the channelizer's counts do not depend on the rate
    counts = [int(c[0]) for c in ctx.ddc_call_counts]
    out, at = [], 0
    with csdr_amd.FmRx(ctx, len(rates), max_samples_per_call=max(counts)) as o:
        for call, k in enumerate(counts):
            for ch in (resets or {}).get(call, []):
                o.reset_channel(ch)
            out.append(o.process(np.stack([row[at:at + k] for row in y]))[0])
            at += k
    return out


if __name__ == "__main__":
    # python fmrx_model.py <in.npz> <out.npz>: bank_composition in a process of its own.  The channelizer's small geometries transform with hipFFT, and a process
    # that has imported torch resolves hipFFT to the copy torch ships, whose last bits differ from those of the system's copy the `csdr` binary links: a
    # composition that is to equal the command byte for byte runs with CSDR_AMD_NO_TORCH_PRELOAD=1, on the same library.
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import csdr_amd
    a = np.load(sys.argv[1])
    c = csdr_amd.Context(0)
    args = (c, a["x"], float(a["tbw"]), int(a["decimation"]), [float(r) for r in a["rates"]], int(a["per"]))
    lines = bank_composition(*args, retunes={1: [(int(a["retune_channel"]), float(a["retune_rate"]))]}, resets={1: [int(a["reset_channel"])]})
    plain = bank_composition(*args)
    np.savez(sys.argv[2], first=lines[0], second=lines[1], plain=np.concatenate(plain, axis=1), torch_loaded="torch" in sys.modules)
    c.close()
