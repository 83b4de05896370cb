"""Pins the C restatement (oracle/csdr_oracle.c) against the compiled, unmodified reference
(oracle/_ref/libcsdr_ref.so).  CPU only.  Bit-exact for converters / integer geometry; <=1e-5 relative
RMS (usually far tighter) for float paths -- the reference build uses -ffast-math, so float paths are
not expected to be bit-identical."""
import numpy as np
import pytest
from oracle import relrms

c64 = np.complex64
f32 = np.float32


def crand(rng, n):
    return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(c64)


# ---------------------------------------------------------------- converters: bit exact, exhaustive
def test_convert_u8_s8_s16_exhaustive(port, ref):
    u8 = np.arange(256, dtype=np.uint8)
    assert np.array_equal(port.convert_u8_f(u8).view(np.uint32), ref.convert_u8_f(u8).view(np.uint32))
    s8 = np.arange(-128, 128, dtype=np.int8)
    assert np.array_equal(port.convert_s8_f(s8).view(np.uint32), ref.convert_s8_f(s8).view(np.uint32))
    s16 = np.arange(-32768, 32768, dtype=np.int16)
    assert np.array_equal(port.convert_s16_f(s16).view(np.uint32), ref.convert_s16_f(s16).view(np.uint32))


def float_probe_set():
    rng = np.random.default_rng(7)
    grid = np.linspace(-1, 1, 65537, dtype=f32)
    special = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(f32(1), f32(0)), -np.nextafter(f32(1), f32(0)),
                        1.5, -1.5, 3.0, -3.0, 1e-40, -1e-40, 1e-30, 0.999999, 2.0, -2.0, 100.0, -100.0,
                        65535.9, -65536.2, 7e4, -7e4], dtype=f32)
    wide = rng.uniform(-4, 4, 20000).astype(f32)
    return np.concatenate([grid, special, wide])


@pytest.mark.parametrize("name", ["convert_f_u8", "convert_f_s8", "convert_f_s16"])
def test_convert_f_int_bit_exact(port, ref, name):
    x = float_probe_set()
    assert np.array_equal(getattr(port, name)(x), getattr(ref, name)(x))


@pytest.mark.parametrize("big", [0, 1])
def test_convert_s24_bit_exact(port, ref, big):
    x = float_probe_set()
    a, b = port.convert_f_s24(x, big), ref.convert_f_s24(x, big)
    assert np.array_equal(a, b)
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 256, 3 * 50000, dtype=np.uint8)
    fa, fb = port.convert_s24_f(raw, big), ref.convert_s24_f(raw, big)
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))


# ---------------------------------------------------------------- design helpers
def test_filter_len_pow2(port, ref):
    for tbw in [0.05, 0.005, 0.03, 0.001, 0.002, 0.01, 0.1, 0.25, 4.0 / 63, 4.0 / 4095]:
        assert port.firdes_filter_len(tbw) == ref.firdes_filter_len(tbw)
    for x in list(range(0, 70)) + [127, 128, 129, 65535, 65536, 65537, 1 << 20]:
        assert port.next_pow2(x) == ref.next_pow2(x)
        assert port.log2n(x) == ref.log2n(x)
    assert port.firdes_filter_len(0.05) == 79 and port.firdes_filter_len(0.005) == 801


@pytest.mark.parametrize("window", ["HAMMING", "BLACKMAN", "BOXCAR"])
@pytest.mark.parametrize("length,cutoff", [(79, 0.05), (801, 0.01), (133, 0.125), (8193, 0.5 / 256)])
def test_firdes_lowpass(port, ref, window, length, cutoff):
    a, b = port.firdes_lowpass_f(length, cutoff, window), ref.firdes_lowpass_f(length, cutoff, window)
    assert relrms(a, b) < 5e-6          # float normalisation sum is reassociated by the reference's -ffast-math
    assert abs(a.sum() - 1) < 1e-5


def test_firdes_bandpass(port, ref):
    for (length, lo, hi) in [(79, -0.1, 0.2), (4095, -0.1, 0.2), (63, 0.1, 0.3), (8193, 0.3 - 0.5 / 256, 0.3 + 0.5 / 256)]:
        a, b = port.firdes_bandpass_c(length, lo, hi), ref.firdes_bandpass_c(length, lo, hi)
        assert relrms(a, b) < 3e-6


# ---------------------------------------------------------------- shifters
@pytest.mark.parametrize("rate", [-0.085, 0.3141, 4e-4, 0.5, -0.5])
def test_shift_addition_stream(port, ref, rate):
    rng = np.random.default_rng(11)
    x = crand(rng, 1024 * 200)
    (a, pa), (b, pb) = port.shift_addition_cc(x, rate), ref.shift_addition_cc(x, rate)
    assert relrms(a, b) < 2e-6
    assert abs(pa - pb) < 1e-5


@pytest.mark.parametrize("chunk", [1000, 777, 4096 + 3, 1])
def test_shift_addition_odd_chunks(port, ref, chunk):
    """The phase advance `starting_phase += d.rate*PI*input_size` (libcsdr_gpl.c:48) for chunk lengths that are not 1024 (the association of that
    product): oracle and compiled reference walk the same stream in `chunk`-sample calls (a ragged last call included) and must agree on samples and on the phase."""
    rng = np.random.default_rng(14)
    x = crand(rng, (chunk * 37 + 5) if chunk > 1 else 3000)
    for rate in (-0.085, 0.3141, 0.03125, 0.4999):
        (a, pa), (b, pb) = port.shift_addition_cc(x, rate, chunk=chunk), ref.shift_addition_cc(x, rate, chunk=chunk)
        assert relrms(a, b) < 2e-6
        assert abs(pa - pb) < 1e-5


@pytest.mark.parametrize("name", ["shift_math_cc", "shift_table_cc", "shift_unroll_cc", "shift_addfast_cc"])
@pytest.mark.parametrize("rate", [-0.085, 0.3141, 4e-4])
def test_shift_variants(port, ref, name, rate):
    rng = np.random.default_rng(12)
    x = crand(rng, 1024 * 64)
    (a, pa), (b, pb) = getattr(port, name)(x, rate), getattr(ref, name)(x, rate)
    tol = 2e-4 if name == "shift_table_cc" else 2e-6    # table index truncation can flip an entry under fast-math
    assert relrms(a, b) < tol
    assert abs(pa - pb) < 1e-4


def test_shift_addition_fc_and_decimating(port, ref):
    rng = np.random.default_rng(13)
    xr = rng.uniform(-1, 1, 4096 * 4).astype(f32)
    (a, _), (b, _) = port.shift_addition_fc(xr, 0.11), ref.shift_addition_fc(xr, 0.11)
    assert relrms(a, b) < 2e-6
    x = crand(rng, 448)
    st_a = st_b = (0, 0.0, 0)
    for _ in range(50):
        ya, st_a = port.decimating_shift_addition_cc(x, 0.0123, 3, st_a)
        yb, st_b = ref.decimating_shift_addition_cc(x, 0.0123, 3, st_b)
        assert st_a[0] == st_b[0] and st_a[2] == st_b[2]
        assert relrms(ya, yb) < 2e-6


# ---------------------------------------------------------------- FIR decimator
@pytest.mark.parametrize("D,ntaps", [(10, 79), (50, 801), (2, 133), (256, 3999), (10, 1023)])
def test_fir_decimate_stream(port, ref, D, ntaps):
    rng = np.random.default_rng(1234)
    x = crand(rng, 16384 * 5 + 777)
    taps = ref.firdes_lowpass_f(ntaps, 0.5 / D)
    a = port.fir_decimate_cc(x, D, taps)
    b = ref.fir_decimate_cc(x, D, taps)
    assert a.size == b.size == (x.size - ntaps) // D + 1
    assert relrms(a, b) < 2e-6


def test_fir_decimate_c1_block(port, ref):
    """BASELINE config 1: one 16384 block, decim 10, 79 taps -> 1631 outputs."""
    rng = np.random.default_rng(1234)
    x = crand(rng, 16384)
    taps = ref.firdes_lowpass_f(79, 0.05)
    b = ref.fir_decimate_cc_block(x, 10, taps)
    assert b.size == 1631
    assert relrms(port.fir_decimate_cc(x, 10, taps), b) < 2e-6


# ---------------------------------------------------------------- demod + audio
def fm_signal(rng, n, dev=0.03125):
    t = np.arange(n)
    msg = np.sin(2 * np.pi * 1e3 / 2.4e6 * t) + 0.3 * rng.uniform(-1, 1, n)
    ph = 2 * np.pi * np.cumsum(dev * msg)
    return (0.7 * np.exp(1j * ph) + 0.01 * (rng.normal(size=n) + 1j * rng.normal(size=n))).astype(c64)


def test_fmdemod(port, ref):
    rng = np.random.default_rng(21)
    x = fm_signal(rng, 1024 * 40)
    x[100] = 0; x[5000:5003] = 0                      # denominator-zero branch
    (a, la), (b, lb) = port.fmdemod_quadri_cf(x), ref.fmdemod_quadri_cf(x)
    assert relrms(a, b) < 1e-6 and la == lb
    assert a[100] == 0 and b[100] == 0
    (c, _) = ref.fmdemod_quadri_novect_cf(x[1:], (float(x[0].real), float(x[0].imag)))
    ok = np.isfinite(c)
    assert relrms(a[1:][ok], c[ok]) < 1e-6


def test_fractional_decimator(port, ref):
    rng = np.random.default_rng(22)
    x = rng.uniform(-1, 1, 1024 * 30).astype(f32)
    a = port.fractional_decimator_ff(x, 5.0)
    b_cli = ref.fractional_decimator_ff(x, 5.0, bufsize=1024)
    b_one = ref.fractional_decimator_ff(x, 5.0)
    n = b_cli.size
    assert n > 6000
    assert np.array_equal(a[:n], x[10:10 + 5 * n:5])            # exact gather x[5k+10]
    assert np.array_equal(b_cli, x[10:10 + 5 * n:5])
    assert np.array_equal(b_one, a)
    for rate in [2.5, 4.17]:
        a = port.fractional_decimator_ff(x, rate); b = ref.fractional_decimator_ff(x, rate)
        assert a.size == b.size and relrms(a, b) < 1e-5
    taps = ref.firdes_lowpass_f(133, 0.5 / (2.5 - 0.03))
    a = port.fractional_decimator_ff(x, 2.5, taps=taps); b = ref.fractional_decimator_ff(x, 2.5, taps=taps)
    assert a.size == b.size and relrms(a, b) < 1e-5
    # the CLI's window loop (csdr.c:1511-1524): for rates that are not exact in float its positions differ from one call over the whole array
    for rate in [3.3, 4.17, 2.5]:
        a = port.fractional_decimator_ff(x, rate, bufsize=1024); b = ref.fractional_decimator_ff(x, rate, bufsize=1024)
        m = min(a.size, b.size)
        assert m >= b.size - 1024 and relrms(a[:m], b[:m]) < 1e-5
    a = port.fractional_decimator_ff(x, 3.3, bufsize=1024); one = port.fractional_decimator_ff(x, 3.3)
    assert relrms(a[:200], one[:200]) < 1e-4 and relrms(a, one[:a.size]) > 1e-2                                # the two models start together and drift apart
    g, w = _prefix(_ref_pipeline(["fractional_decimator_ff 3.3"], x), f32, a)                                 # ... and the reference binary follows the window loop
    assert relrms(g, w) < 1e-5


def test_deemphasis_limit_gain_agc(port, ref):
    rng = np.random.default_rng(23)
    x = rng.uniform(-1.5, 1.5, 1024 * 20).astype(f32)
    (a, la), (b, lb) = port.deemphasis_wfm_ff(x, 50e-6, 48000), ref.deemphasis_wfm_ff(x, 50e-6, 48000)
    assert relrms(a, b) < 1e-6
    assert np.array_equal(port.limit_ff(x, 1.0), ref.limit_ff(x, 1.0))
    assert np.array_equal(port.gain_ff(x, 0.37), ref.gain_ff(x, 0.37))
    for sr in [48000, 44100, 8000, 11025]:
        taps = ref.nfm_taps(sr)
        a = port.deemphasis_nfm_ff(x[:4096], taps); b = ref.deemphasis_nfm_ff(x[:4096], sr)
        assert a.size == b.size == 4096 - taps.size and relrms(a, b) < 2e-6
    assert ref.deemphasis_nfm_ff(x[:1024], 12345).size == 0
    env = (0.05 + np.abs(np.sin(np.arange(x.size) / 3000.0))).astype(f32)
    a = port.fastagc_ff(x * env); b = ref.fastagc_ff(x * env)
    assert np.all(a[:2048] == 0) and np.all(b[:2048] == 0)
    assert relrms(a, b) < 1e-6


# ---------------------------------------------------------------- FFT paths
def test_fft_shim_vs_numpy(port):
    rng = np.random.default_rng(31)
    for n in [8, 512, 65536, 12]:
        x = crand(rng, n)
        assert relrms(port.fft_c2c(x, True), np.fft.fft(x.astype(np.complex128))) < 2e-7
        assert relrms(port.fft_c2c(x, False), np.fft.ifft(x.astype(np.complex128)) * n) < 2e-7


@pytest.mark.parametrize("ntaps,fft_size", [(63, 1024), (255, 4096), (4095, 65536), (63, 65536)])
def test_bandpass_fir_fft(port, ref, ntaps, fft_size):
    rng = np.random.default_rng(3)
    inp = fft_size - ntaps + 1
    x = crand(rng, inp * 4)
    taps = ref.firdes_bandpass_c(ntaps, -0.1, 0.2)
    a = port.bandpass_fir_fft_cc(x, taps, fft_size); b = ref.bandpass_fir_fft_cc(x, taps, fft_size)
    assert relrms(a, b) < 2e-6
    if fft_size <= 4096:
        direct = np.convolve(x.astype(np.complex128), taps.astype(np.complex128))[:a.size]
        assert relrms(a, direct) < 2e-6


def test_fastddc_geometry(port, ref):
    # (D = 5 .. 2048 and tbw = 0.01 .. 0.000125: the geometry classes of tests/test_fastddc_geometries_gpu.py -- pre_decimation 1 .. 1024, post_decimation 2, 3, 5, 25)
    for D in [2, 3, 4, 6, 8, 10, 16, 24, 50, 64, 100, 128, 256, 5, 32, 40, 48, 384, 512, 640, 768, 1024, 2048]:
        for tbw in [0.05, 0.005, 0.001, 0.01, 0.0025, 0.002, 0.0005, 0.00025, 0.000125]:
            for s in [0.0, -0.1, 0.4, 0.123456, -0.5 + 0.5 / 256, 0.25]:
                da, ea = port.fastddc_init(tbw, D, s); db, eb = ref.fastddc_init(tbw, D, s)
                A, B = da.as_dict(), db.as_dict()
                assert ea == eb
                for k in A:
                    if k in ("output_scrape",):
                        continue               # never initialised by the reference (fastddc.c:38-72)
                    if isinstance(A[k], int):
                        assert A[k] == B[k], (D, tbw, s, k, A[k], B[k])
                    elif isinstance(A[k], tuple):
                        assert np.allclose(A[k], B[k], rtol=0, atol=2e-6), (D, tbw, s, k)
                    else:
                        assert abs(A[k] - B[k]) <= 1e-6 * max(1, abs(B[k])), (D, tbw, s, k)
    d, _ = port.fastddc_init(0.001, 256, 0.0)
    assert (d.fft_size, d.taps_length, d.input_size, d.fft_inv_size, d.scrap, d.post_input_size,
            d.pre_decimation, d.post_decimation) == (65536, 8193, 57344, 512, 64, 448, 128, 2)


@pytest.mark.parametrize("D,tbw,shift", [(16, 0.05, -0.1), (256, 0.005, 0.3 + 0.5 / 256), (6, 0.05, 0.2),
                                         # BASELINE config 4's exact geometry (fft 65536 / inverse 512), channels 0, 127, 255 of -0.5 + (c + 0.5) / 256
                                         (256, 0.001, -0.5 + 0.5 / 256), (256, 0.001, -0.5 + 127.5 / 256), (256, 0.001, -0.5 + 255.5 / 256),
                                         # one per geometry class of tests/test_fastddc_geometries_gpu.py (its cases a .. k: fft / pre_decimation / post_decimation),
                                         # shifts at both band edges, at 0, on and off the 1 / fft grid, either sign
                                         (16, 0.01, 0.1234),                                                    # a  4096 / 8 / 2
                                         (24, 0.01, -0.4999), (40, 0.01, 0.4999),                               # b  4096 / 8 / 3, 5
                                         (32, 0.005, -0.3711), (64, 0.0025, 0.0), (128, 0.002, 0.25),           # c  8192 / 16, 16384 / 32, 32768 / 64; post 2
                                         (48, 0.005, 0.0517),                                                   # d  8192 / 16 / 3
                                         (512, 0.0005, -0.2222), (768, 0.0005, 0.3711),                         # e  131072 / 256 / 2, 3
                                         (384, 0.001, -0.5 + 100.5 / 256),                                      # f  65536 / 128 / 3
                                         (640, 0.001, 0.125),                                                   # g  65536 / 128 / 5
                                         (1024, 0.00025, -0.1234),                                              # h  262144 / 512 / 2
                                         (2048, 0.000125, 0.3333),                                              # i  524288 / 1024 / 2
                                         (5, 0.05, -0.41), (2, 0.05, 0.2),                                      # j  1024 / 1 / 5, 2
                                         (50, 0.05, 0.33)])                                                     # k  1024 / 2 / 25
def test_fastddc_stream(port, ref, D, tbw, shift):
    rng = np.random.default_rng(4)
    da, _ = port.fastddc_init(tbw, D, shift); db, _ = ref.fastddc_init(tbw, D, shift)
    x = crand(rng, da.input_size * (12 if da.fft_size < 65536 else 5 if da.fft_size == 65536 else 3))
    sa = port.fastddc_fwd_cc(x, da); sb = ref.fastddc_fwd_cc(x, db)
    assert relrms(sa, sb) < 1e-6
    ta = port.fastddc_taps_fft(da, shift, D); tb = ref.fastddc_taps_fft(db, shift, D)
    assert relrms(ta, tb) < 5e-6
    ya = port.fastddc_inv_cc(sa, da, ta); yb = ref.fastddc_inv_cc(sb, db, tb)
    assert ya.size == yb.size and ya.size > 0
    assert relrms(ya, yb) < 1e-5
    # ... and block by block (the GPU tests of the geometry classes hold every call of every channel to the float gate: a whole-stream ratio hides one bad block)
    ba = port.fastddc_inv_cc(sa, da, ta, per_block=True); bb = ref.fastddc_inv_cc(sb, db, tb, per_block=True)
    assert [a.size for a in ba] == [b.size for b in bb]
    worst = max(relrms(a, b) for a, b in zip(ba, bb))
    print("fastddc oracle vs reference D %d tbw %g shift %g: stream %.3g, worst block %.3g" % (D, tbw, shift, relrms(ya, yb), worst))
    assert worst < 1e-5


# ---------------------------------------------------------------- the WFM chain
def test_wfm_chain(port, ref):
    rng = np.random.default_rng(1000)
    n = 16384 * 12
    sig = fm_signal(rng, n) * np.exp(2j * np.pi * 0.085 * np.arange(n))
    iq = np.empty(2 * n, f32); iq[0::2] = sig.real; iq[1::2] = sig.imag
    u8 = np.clip(np.round(127.5 * (iq + 1)), 0, 255).astype(np.uint8)
    taps = ref.firdes_lowpass_f(79, 0.05)
    (sa, fa), (sb, fb) = port.wfm_chain(u8, -0.085, 10, taps), ref.wfm_chain(u8, -0.085, 10, taps)
    n = min(fa.size, fb.size)
    assert n >= 16384 * 12 // 50 - 8
    assert relrms(fa[:n], fb[:n]) < 1e-5
    d = np.abs(sa[:n].astype(np.int32) - sb[:n].astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 0.05


def test_nfm_chain_vs_reference_cli(port):
    """BASELINE config 5 / README.md:87 as EIGHT processes of the unmodified reference binary connected by real pipes, against the oracle's
    stage-by-stage stream model (port.nfm_chain) that the GPU parity tests of the NFM chain use."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "oracle", "_ref", "csdr")
    if not os.path.exists(cli):
        pytest.skip("oracle/_ref/csdr not built")
    sys.path.insert(0, os.path.join(root, "tests"))
    from tests_helpers import nfm_signal_u8
    n = 1024 * 400
    iq = nfm_signal_u8(91, n, offset=-0.11)
    pipe = " | ".join("%s %s" % (cli, c) for c in ("convert_u8_f", "shift_addition_cc 0.11", "fir_decimate_cc 50 0.005 HAMMING", "fmdemod_quadri_cf", "limit_ff",
                                                    "deemphasis_nfm_ff 48000", "fastagc_ff", "convert_f_s16"))
    p = subprocess.run(pipe, shell=True, input=iq.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=120)
    got = np.frombuffer(p.stdout[:len(p.stdout) // 2 * 2], np.int16)
    taps = np.load(os.path.join(root, "tests", "golden", "nfm_deemph_taps.npz"))["sr48000"]
    want, _ = port.nfm_chain(iq, 0.11, taps)
    m = min(got.size, want.size)
    assert m >= 4 * 1024 and want.size - m <= 2048            # the process pipeline may hold back / repeat its last blocks at EOF
    assert np.any(got[2048:4096] != 0)                        # (fastagc's two zero blocks, then audio)
    d = np.abs(got[:m].astype(np.int32) - want[:m].astype(np.int32))
    assert d.max() <= 1 and np.mean(d != 0) < 0.02, (d.max(), np.mean(d != 0))


def _ref_pipeline(cmds, data):
    """The commands as separate processes of the unmodified reference binary connected by pipes (skips when it was not built)."""
    import os
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "csdr")
    if not os.path.exists(cli):
        pytest.skip("oracle/_ref/csdr not built")
    pipe = " | ".join("%s %s" % (cli, c) for c in cmds)
    return subprocess.run(pipe, shell=True, input=np.ascontiguousarray(data).tobytes(), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout


def _prefix(out, dtype, want):
    """The reference processes repeat / hold back their last blocks at EOF: compare the common prefix, which must cover
    the oracle's output up to a few buffers."""
    isz = np.dtype(dtype).itemsize
    got = np.frombuffer(out[:len(out) // isz * isz], dtype)
    m = min(got.size, want.size)
    assert m > 0 and want.size - m <= 4096, (got.size, want.size)
    return got[:m], want[:m]


def test_am_and_ssb_chains_vs_reference_cli(port):
    """README.md:95 (AM) and :110 (SSB) as process pipelines of the reference binary against the oracle's stage-by-stage stream models
    (the ones the GPU tests of the CLI chains and of the fused front end are compared with)."""
    rng = np.random.default_rng(15)
    n = 400000
    t = np.arange(n)
    audio = 0.5 * np.sin(2 * np.pi * 700 / 2.4e6 * t)
    am = 0.5 * (1 + audio) * np.exp(2j * np.pi * 0.25 * t) + 0.01 * (rng.normal(size=n) + 1j * rng.normal(size=n))
    iq = np.empty(2 * n, f32); iq[0::2] = am.real; iq[1::2] = am.imag
    iq = np.clip(np.round(127.5 * (iq + 1)), 0, 255).astype(np.uint8)
    front = ["convert_u8_f", "shift_addition_cc -0.25", "fir_decimate_cc 50 0.005 HAMMING"]
    xf = port.convert_u8_f(iq).view(c64)
    sh, _ = port.shift_addition_cc(xf, -0.25)
    dec = port.fir_decimate_cc(sh, 50, port.firdes_lowpass_f(port.firdes_filter_len(0.005), 0.5 / 50))
    g, w = _prefix(_ref_pipeline(front, iq), c64, dec)
    assert relrms(g, w) < 1e-5
    d, _ = port.fastdcblock_ff(port.amdemod_cf(dec))
    g, w = _prefix(_ref_pipeline(front + ["amdemod_cf", "fastdcblock_ff"], iq), f32, d)
    assert relrms(g, w) < 1e-5
    want = port.convert_f_s16(port.limit_ff(port.agc_ff(d)[0], 1.0))
    g, w = _prefix(_ref_pipeline(front + ["amdemod_cf", "fastdcblock_ff", "agc_ff", "limit_ff", "convert_f_s16"], iq), np.int16, want)
    dd = np.abs(g.astype(np.int32) - w.astype(np.int32))
    assert dd.max() <= 2 and np.mean(dd != 0) < 0.03
    nt = port.firdes_filter_len(0.05); fft = port.next_pow2(nt)
    if fft - nt < 200:
        fft *= 2                                                # csdr.c:1834-1836
    bp = port.bandpass_fir_fft_cc(dec, port.firdes_bandpass_c(nt, 0.0, 0.1), fft)
    g, w = _prefix(_ref_pipeline(front + ["bandpass_fir_fft_cc 0 0.1 0.05"], iq), c64, bp)
    assert relrms(g, w) < 1e-5
    want = port.convert_f_s16(port.limit_ff(port.gain_ff(port.realpart_cf(bp), 3.0), 1.0))
    g, w = _prefix(_ref_pipeline(front + ["bandpass_fir_fft_cc 0 0.1 0.05", "realpart_cf", "gain_ff 3", "limit_ff", "convert_f_s16"], iq), np.int16, want)
    dd = np.abs(g.astype(np.int32) - w.astype(np.int32))
    assert dd.max() <= 1 and np.mean(dd != 0) < 0.03


@pytest.mark.parametrize("D,tbw,shift", [(16, 0.05, 0.2), (8, 0.05, -0.31)])
def test_fastddc_vs_reference_cli(port, D, tbw, shift):
    """`csdr fastddc_fwd_cc | csdr fastddc_inv_cc` (csdr.c:2255-2378) as two reference processes against the oracle's stream model."""
    rng = np.random.default_rng(44)
    x = crand(rng, 300000)
    pd, _ = port.fastddc_init(tbw, D, shift)
    spec = port.fastddc_fwd_cc(x, pd)
    g, w = _prefix(_ref_pipeline(["fastddc_fwd_cc %d %g" % (D, tbw)], x), c64, spec.reshape(-1))
    assert relrms(g, w) < 1e-5
    y = port.fastddc_inv_cc(spec, pd, port.fastddc_taps_fft(pd, shift, D))
    g, w = _prefix(_ref_pipeline(["fastddc_fwd_cc %d %g" % (D, tbw), "fastddc_inv_cc %g %d %g" % (shift, D, tbw)], x), c64, y)
    assert relrms(g, w) < 1e-5


def _first(y):
    return y[0] if isinstance(y, tuple) else y


def test_single_commands_vs_reference_cli(port):
    """Every hot-path `csdr <command>` as ONE process of the reference binary against the oracle's stream model of that command's loop
    (what the GPU tests of csdr_amd/csdr are compared with): block framing, re-feed and carried state are part of what is pinned here."""
    rng = np.random.default_rng(8)
    x = crand(rng, 70000)
    r = rng.uniform(-1.3, 1.3, 70000).astype(f32)
    bp_nt = port.firdes_filter_len(0.01); bp_fft = port.next_pow2(bp_nt)
    if bp_fft - bp_nt < 200:
        bp_fft *= 2
    dsa = []; st = (0, 0.0, 0)
    for at in range(0, x.size, 16384):                          # decimating_shift_addition_cc: one call per 16384-sample buffer, status carried (csdr.c:851-875)
        y, st = port.decimating_shift_addition_cc(x[at:at + 16384], 0.07, 6, st); dsa.append(y)
    cases = [
        ("shift_addition_cc 0.123", x, c64, lambda: port.shift_addition_cc(x, 0.123)[0]),
        ("shift_math_cc 0.123", x, c64, lambda: port.shift_math_cc(x, 0.123)[0]),
        ("shift_addfast_cc 0.123", x, c64, lambda: port.shift_addfast_cc(x, 0.123)[0]),
        ("shift_unroll_cc 0.123", x, c64, lambda: port.shift_unroll_cc(x, 0.123)[0]),
        ("shift_table_cc 0.123 4096", x, c64, lambda: port.shift_table_cc(x, 0.123, 4096)[0]),
        ("shift_addition_fc 0.2", r, c64, lambda: port.shift_addition_fc(r, 0.2)[0]),
        ("decimating_shift_addition_cc 0.07 6", x, c64, lambda: np.concatenate(dsa)),
        ("fir_decimate_cc 7 0.03 HAMMING", x, c64, lambda: port.fir_decimate_cc(x, 7, port.firdes_lowpass_f(port.firdes_filter_len(0.03), 0.5 / 7))),
        ("fmdemod_quadri_cf", x, f32, lambda: _first(port.fmdemod_quadri_cf(x))),
        ("fmdemod_atan_cf", x, f32, lambda: _first(port.fmdemod_atan_cf(x))),
        ("amdemod_cf", x, f32, lambda: port.amdemod_cf(x)),
        ("amdemod_estimator_cf", x, f32, lambda: _first(port.amdemod_estimator_cf(x))),
        ("realpart_cf", x, f32, lambda: port.realpart_cf(x)),
        ("logpower_cf -70", x, f32, lambda: port.logpower_cf(x, -70.0)),
        ("fractional_decimator_ff 5", r, f32, lambda: port.fractional_decimator_ff(r, 5.0, bufsize=1024)),
        ("fractional_decimator_ff 3.3", r, f32, lambda: port.fractional_decimator_ff(r, 3.3, bufsize=1024)),
        ("deemphasis_wfm_ff 48000 50e-6", r, f32, lambda: port.deemphasis_wfm_ff(r, 50e-6, 48000)[0]),
        ("deemphasis_wfm_ff 44100 75e-6", r, f32, lambda: port.deemphasis_wfm_ff(r, 75e-6, 44100)[0]),
        ("limit_ff 0.7", r, f32, lambda: port.limit_ff(r, 0.7)),
        ("gain_ff 2.5", r, f32, lambda: port.gain_ff(r, 2.5)),
        ("fastagc_ff", r, f32, lambda: port.fastagc_ff(r, 1024, 1.0)),
        ("fastagc_ff 512 0.5", r, f32, lambda: port.fastagc_ff(r, 512, 0.5)),
        ("dcblock_ff", r, f32, lambda: _first(port.dcblock_ff(r))),
        ("fastdcblock_ff", r, f32, lambda: _first(port.fastdcblock_ff(r))),
        ("agc_ff", r, f32, lambda: _first(port.agc_ff(r))),
        ("fft_cc 1024 300", x, c64, lambda: np.asarray(_first(port.fft_cc(x, 1024, 300))).reshape(-1)),
        ("fft_cc 512 1200 BLACKMAN", x, c64, lambda: np.asarray(_first(port.fft_cc(x, 512, 1200, "BLACKMAN"))).reshape(-1)),
        ("bandpass_fir_fft_cc -0.2 0.1 0.01", x, c64, lambda: port.bandpass_fir_fft_cc(x, port.firdes_bandpass_c(bp_nt, -0.2, 0.1), bp_fft)),
    ]
    for cmd, data, dt, model in cases:
        want = np.asarray(model())
        out = _ref_pipeline([cmd], data)
        isz = np.dtype(dt).itemsize
        got = np.frombuffer(out[:len(out) // isz * isz], dt)
        m = min(got.size, want.size)
        assert m > 0 and want.size - m <= 20000, (cmd, got.size, want.size)      # at EOF the reference drops / repeats up to one (big) buffer
        assert relrms(got[:m], want[:m]) < 1e-5, (cmd, relrms(got[:m], want[:m]))
    # bit exact ones
    b24 = rng.integers(0, 256, 3 * 20000, dtype=np.uint8)
    for cmd, data, dt, model in [("convert_f_s24", r, np.uint8, lambda: port.convert_f_s24(r, 0)), ("convert_f_s24 --bigendian", r, np.uint8, lambda: port.convert_f_s24(r, 1)),
                                 ("convert_s24_f --bigendian", b24, f32, lambda: port.convert_s24_f(b24, 1)), ("convert_f_s16", r, np.int16, lambda: port.convert_f_s16(r)),
                                 ("convert_f_u8", r, np.uint8, lambda: port.convert_f_u8(r))]:
        want = np.asarray(model())
        out = _ref_pipeline([cmd], data)
        got = np.frombuffer(out[:len(out) // np.dtype(dt).itemsize * np.dtype(dt).itemsize], dt)
        m = min(got.size, want.size)
        assert m >= want.size - 4096 and np.array_equal(got[:m].view(np.uint8), want[:m].view(np.uint8)), cmd


# ---------------------------------------------------------------- f2 blocks
def test_f2_elementwise(port, ref):
    rng = np.random.default_rng(31)
    x = (rng.normal(size=20000) + 1j * rng.normal(size=20000)).astype(np.complex64)
    x[:4] = [0, 1, -1j, 1e-20]
    assert relrms(port.amdemod_cf(x), ref.amdemod_cf(x)) <= 1e-6
    assert np.array_equal(port.amdemod_estimator_cf(x), ref.amdemod_estimator_cf(x))
    assert np.array_equal(port.amdemod_estimator_cf(x, 0.9, 0.4), ref.amdemod_estimator_cf(x, 0.9, 0.4))
    a, pa = port.fmdemod_atan_cf(x, 0.3); b, pb = ref.fmdemod_atan_cf(x, 0.3)
    assert relrms(a, b) <= 1e-6 and abs(pa - pb) <= 1e-6
    with np.errstate(divide="ignore"):
        lp, lr = port.logpower_cf(x[4:], 3.0), ref.logpower_cf(x[4:], 3.0)       # (a denormal power is flushed by the reference build)
    assert relrms(lp, lr) <= 1e-6
    for w in ("HAMMING", "BLACKMAN", "BOXCAR"):
        assert np.abs(port.precalculate_window(1024, w) - ref.precalculate_window(1024, w)).max() <= 1e-6
    w = port.precalculate_window(512)
    out = np.zeros(512, np.complex64)
    import ctypes as C
    port.L.orc_apply_precalculated_window_c(x[:512].ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 512, w.ctypes.data_as(C.c_void_p))
    assert np.array_equal(out, ref.apply_precalculated_window_c(x[:512], w))


def test_f2_recursive_blocks(port, ref):
    rng = np.random.default_rng(32)
    a = (rng.uniform(-1, 1, 30000) + 0.3).astype(np.float32)
    (y, s), (yr, sr) = port.dcblock_ff(a, 0, (0.1, 0.2)), ref.dcblock_ff(a, 0, (0.1, 0.2))
    assert relrms(y, yr) <= 5e-6 and np.allclose(s, sr, atol=2e-6)
    (y, s), (yr, sr) = port.dcblock_ff(a, 0.95), ref.dcblock_ff(a, 0.95)
    assert relrms(y, yr) <= 5e-6
    (y, l), (yr, lr) = port.fastdcblock_ff(a, 1024, 0.1), ref.fastdcblock_ff(a, 1024, 0.1)
    assert relrms(y, yr) <= 1e-6 and abs(l - lr) <= 1e-6
    sig = (rng.uniform(-1, 1, 40000) * np.repeat(rng.uniform(0.01, 1, 400), 100)).astype(np.float32)
    sig[1000:1010] = 0
    for kw in ({}, dict(hang_time=20, reference=0.5, attack_rate=0.05, decay_rate=0.001, max_gain=100.0, attack_wait=5, filter_alpha=0.99)):
        (y, g), (yr, gr) = port.agc_ff(sig, 1024, **kw), ref.agc_ff(sig, 1024, **kw)
        assert relrms(y, yr) <= 5e-6 and abs(g - gr) <= 1e-5 * max(1, abs(gr))


# ---------------------------------------------------------------- f3: IMA ADPCM (bit exact)
def test_f3_adpcm_bit_exact(port, ref):
    rng = np.random.default_rng(33)
    smooth = (8000 * np.sin(np.arange(20001) * 0.01) + rng.integers(-3000, 3000, 20001)).astype(np.int16)
    wild = rng.integers(-32768, 32768, 5001).astype(np.int16)
    for x, st in ((smooth, (0, 0)), (smooth, (5, -100)), (wild, (88, 32767)), (wild[:1], (0, 0)), (wild[:0], (3, 3))):
        (a, sa), (b, sb) = port.encode_ima_adpcm_i16_u8(x, st), ref.encode_ima_adpcm_i16_u8(x, st)
        assert np.array_equal(a, b) and sa == sb
        (c, sc), (d, sd) = port.decode_ima_adpcm_u8_i16(a, (3, 77)), ref.decode_ima_adpcm_u8_i16(a, (3, 77))
        assert np.array_equal(c, d) and sc == sd
    codes = rng.integers(0, 256, 4000, dtype=np.uint8)
    (c, sc), (d, sd) = port.decode_ima_adpcm_u8_i16(codes), ref.decode_ima_adpcm_u8_i16(codes)
    assert np.array_equal(c, d) and sc == sd


def test_f3_compress_fft_vs_reference_cli(port):
    """compress_fft_adpcm_f_u8 only exists as a CLI loop (csdr.c:1745-1768): pin the restatement to the reference binary's bytes."""
    import os
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "csdr")
    if not os.path.exists(cli):
        pytest.skip("oracle/_ref/csdr not built")
    rng = np.random.default_rng(34)
    x = (rng.uniform(-120, 10, 6 * 1024) + 20 * np.sin(np.arange(6 * 1024) * 0.05)).astype(np.float32)
    p = subprocess.run([cli, "compress_fft_adpcm_f_u8", "1024"], input=x.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=30)
    want = port.compress_fft_adpcm_f_u8(x, 1024)
    got = np.frombuffer(p.stdout, np.uint8)
    assert got.size >= want.size and np.array_equal(got[:want.size], want)      # the reference CLI repeats its last block at EOF
