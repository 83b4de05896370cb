"""The pulse-shaped symbol modem on the GPU: both kernels of the transmit object against the float32 model (pulse_model.py) bit for bit and against float64
within the dot-product gate, cut and batch invariance, output bounds, the composed device path, the flat operators, the drop-in functions and the CLI
against the compiled reference, the round trip through a matched filter and the slicer, lifecycle and argument errors."""
import ctypes as C
import functools
import os
import subprocess
import numpy as np
import pytest

import pulse_model as pm
import test_pulse_cpu as tc
from test_pulse_cpu import bits_eq

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")
REF_CSDR = os.path.join(ROOT, "oracle", "_ref", "csdr")
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
POLY, GENERIC = "k_pulsetx_poly", "k_pulsetx_generic"
N_SYM = 300
# (interpolation, taps): the CPU list, a history longer than a call's symbols at 5 per call, 16 and 17 taps per phase (the most k_pulsetx_poly keeps in
# registers, and one more) and taps that do not fit LDS beside a tile (4 K I + 8 (4096 / I + K + 4) > 63 KiB)
SHAPES = tc.SHAPES + [(3, 200), (2, 32), (2, 33), (4, 63), (64, 16000)]
CHANNELS = [1, 3, 65]


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def fits_lds(I, T):
    K = (T + I - 1) // I
    return 4 * ((K * I + 1) & ~1) + 8 * (4096 // I + K + 4) <= 63 * 1024


def name_of(I, T, last="shape", forced=False):
    return POLY if last == "shape" and not forced and fits_lds(I, T) else GENERIC


@functools.lru_cache(maxsize=None)
def case(I, T, n_psk=4, channels=65, n=N_SYM):
    """one shape's inputs and expected streams, computed once: bytes, their symbols, free complex symbols, taps, the float32 streams of both"""
    rng = np.random.default_rng(31 * I + T + n_psk)
    idx = rng.integers(0, 256, (channels, n)).astype(np.uint8)
    free = (rng.standard_normal((channels, n)) + 1j * rng.standard_normal((channels, n))).astype(np.complex64)
    taps = tc.test_taps(I, T)
    sym = pm.symbols(n_psk)
    d = dict(idx=idx, sym=sym[idx], free=free, taps=taps, y_idx=pm.shape32(sym[idx], I, taps), y_free=pm.shape32(free, I, taps))
    for v in d.values():
        v.setflags(write=False)
    return d


# ------------------------------------------------------------------ both kernels against the float32 model
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_model(ctx, shape):
    I, T = shape
    m = case(I, T)
    assert (name_of(I, T) == GENERIC) == (shape == (64, 16000))
    for ch in CHANNELS:
        for forced in (False, True):
            with ctx.pulse_tx(ch, 4, I, m["taps"], "mod", "shape") as o:
                o.force_generic(forced)
                y = o.process(m["idx"][:ch])
                assert o.kernel_name() == name_of(I, T, forced=forced)
                assert y.shape == (ch, pm.n_outputs(N_SYM, I, T)) and bits_eq(y, m["y_idx"][:ch]), (ch, forced)
            with ctx.pulse_tx(ch, 4, I, m["taps"], "shape", "shape") as o:
                o.force_generic(forced)
                y = o.process(m["free"][:ch])
                assert o.kernel_name() == name_of(I, T, forced=forced) and bits_eq(y, m["y_free"][:ch]), (ch, forced)
        with ctx.pulse_tx(ch, 4, I, None, "mod", "mod") as o:
            y = o.process(m["idx"][:ch])
            assert o.kernel_name() == GENERIC and bits_eq(y, m["sym"][:ch]) and o.max_out(10) == 10


@pytest.mark.parametrize("n_psk", [2, 8, 256])
def test_other_n_psk(ctx, n_psk):
    m = case(8, 65, n_psk, 3)
    with ctx.pulse_tx(3, n_psk, 8, m["taps"]) as o:
        assert bits_eq(o.process(m["idx"]), m["y_idx"]) and o.kernel_name() == POLY


# ------------------------------------------------------------------ cuts and batch position
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("shape", [(8, 65), (5, 21), (64, 33), (2, 5)])
def test_cut_at_tile_edges(ctx, shape, forced):
    """the same stream in one call and cut at tile() - 1, tile(), tile() + 1, 0 and 1 symbols: equal by bits, and equal to the model"""
    I, T = shape
    with ctx.pulse_tx(3, 4, I, tc.test_taps(I, T)) as o:
        tile = o.tile()
        assert tile == max(1, 4096 // I)
        m = case(I, T, 4, 3, 3 * tile + 40)
        o.force_generic(forced)
        one = o.process(m["idx"])
        assert o.kernel_name() == name_of(I, T, forced=forced)
        o.reset()
        cut = o.process(m["idx"], calls=[tile - 1, tile, tile + 1, 0, 1, 39])
    assert bits_eq(one, m["y_idx"]) and bits_eq(cut, one)


@pytest.mark.parametrize("forced", [False, True])
def test_calls_shorter_than_the_history(ctx, forced):
    I, T = 3, 200
    m = case(I, T)
    with ctx.pulse_tx(3, 4, I, m["taps"], "shape", "shape") as o:
        o.force_generic(forced)
        cut = o.process(m["free"][:3], calls=[5] * (N_SYM // 5))
        assert o.kernel_name() == name_of(I, T, forced=forced)
    assert bits_eq(cut, m["y_free"][:3])


@pytest.mark.parametrize("forced", [False, True])
def test_batch_position(ctx, forced):
    """a channel gives the same bits alone and at index 64 of 65; a reset starts the stream again"""
    m = case(8, 65)
    with ctx.pulse_tx(65, 4, 8, m["taps"]) as o:
        o.force_generic(forced)
        full = o.process(m["idx"], calls=[100, 200])
        o.reset()
        again = o.process(m["idx"])
    with ctx.pulse_tx(1, 4, 8, m["taps"]) as o:
        o.force_generic(forced)
        alone = o.process(m["idx"][64])
    assert bits_eq(full[64], alone) and bits_eq(full, again) and bits_eq(full, m["y_idx"])


# ------------------------------------------------------------------ bounds
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("shape", [(8, 65), (7, 7), (1, 1), (64, 33), (5, 21)])
def test_nothing_written_beyond_n_out(ctx, shape, forced):
    """rows an odd number of samples apart (every second row starts on an odd complex sample: the kernel's other store alignment), sentinels behind
    n_out and between the rows untouched, in two calls"""
    I, T = shape
    m = case(I, T)
    ch, calls = 3, [101, N_SYM - 101]
    with ctx.pulse_tx(ch, 4, I, m["taps"]) as o:
        o.force_generic(forced)
        pitch = o.max_out(max(calls)) + 5
        pitch += 1 - pitch % 2
        can = (np.arange(ch * pitch) + 1j * 7).astype(np.complex64)
        di = ctx.upload(m["idx"][:ch])
        pos, done = 0, 0
        for n in calls:
            do = ctx.upload(can)
            k = o.process_dev(di.at(pos), n, N_SYM, do.ptr, pitch)
            y = ctx.download(do, np.complex64, ch * pitch).reshape(ch, pitch)
            assert k == pm.n_outputs(pos + n, I, T) - pm.n_outputs(pos, I, T)
            assert bits_eq(y[:, :k], m["y_idx"][:ch, done:done + k])
            assert bits_eq(y[:, k:], can.reshape(ch, pitch)[:, k:])
            pos += n; done += k


def test_out_pitch_below_max_out_consumes_nothing(ctx):
    import csdr_amd
    m = case(8, 65)
    with ctx.pulse_tx(2, 4, 8, m["taps"]) as o:
        di, do = ctx.upload(m["idx"][:2]), ctx.alloc(8 * 2 * o.max_out(N_SYM) + 64)
        assert o.max_out(N_SYM) == 8 * N_SYM
        with pytest.raises(csdr_amd.CsdrAmdError):
            o.process_dev(di.ptr, N_SYM, N_SYM, do.ptr, o.max_out(N_SYM) - 1)
        with pytest.raises(csdr_amd.CsdrAmdError):
            o.process_dev(di.ptr, N_SYM, N_SYM - 1, do.ptr, o.max_out(N_SYM))          # in_pitch below n_in
        assert o.kernel_name() == ""                                                  # nothing was launched
        assert bits_eq(o.process(m["idx"][:2]), m["y_idx"][:2])                        # and nothing was consumed: the stream starts here


# ------------------------------------------------------------------ float64 and the composed device path
@pytest.mark.parametrize("shape", tc.SHAPES + [(3, 200)])
def test_against_float64_and_composed_path(ctx, shape):
    """gate of the object: K 2^-24 1.01 sum |c_k tap_k| per output and component (a chain of K fused multiply-adds).  The composed path
    plain_interpolate_cc -> apply_real_fir_cc adds T products (all but K of them zero) in the FIR kernel's own order: gate T 2^-24 1.01 of the same sum;
    the two paths differ by at most the sum of both gates."""
    I, T = shape
    m = case(I, T)
    K = (T + I - 1) // I
    want, mr, mi = pm.shape64(m["free"][:3], I, m["taps"])
    with ctx.pulse_tx(3, 4, I, m["taps"], "shape", "shape") as o:
        y = o.process(m["free"][:3])
    assert pm.within(y, want, pm.dot_gate(K, mr), pm.dot_gate(K, mi))
    x = ctx.plain_interpolate_cc(m["free"][:3], I)
    assert bits_eq(x, pm.stuffed(m["free"][:3], I))
    z = ctx.apply_real_fir_cc(x, m["taps"])
    assert z.shape == y.shape
    assert pm.within(z, want, pm.dot_gate(T, mr), pm.dot_gate(T, mi))
    assert pm.within(z, y.astype(np.complex128), pm.dot_gate(K + T, mr), pm.dot_gate(K + T, mi))


# ------------------------------------------------------------------ flat operators
@pytest.mark.parametrize("rows,n", [(3, 1000), (1, 7)])
def test_flat_operators(ctx, rows, n):
    rng = np.random.default_rng(rows + n)
    x = rng.uniform(-1.5, 1.5, (rows, n)).astype(np.float32)
    x[0, :5] = [np.nan, np.inf, -np.inf, 0.0, -0.0]
    for ns in tc.SLICER_N:
        lo, hi = pm.slicer_limits(ns)
        x[-1, 5:7] = [lo[0], hi[-1]]
        assert np.array_equal(ctx.generic_slicer_f_u8(x, ns), pm.slicer(x, ns)), ns
    c = (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))).astype(np.complex64)
    for I in (1, 3, 8):
        assert bits_eq(ctx.plain_interpolate_cc(c, I), pm.stuffed(c, I))
    b = rng.integers(0, 256, (rows, n)).astype(np.uint8)
    assert np.array_equal(ctx.pack_bits_1to8(b), pm.pack_1to8(b))
    g = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), (rows, 8 * n))
    assert np.array_equal(ctx.pack_bits_8to1(g), pm.pack_8to1(g))
    assert bits_eq(ctx.pack_bits_1to8(b[0]), pm.pack_1to8(b[0]))                       # 1-D in, 1-D out


def test_flat_operator_errors(ctx):
    import csdr_amd
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.pack_bits_8to1(np.zeros(12, np.uint8))                                    # not a multiple of 8
    for ns in (1, 257):
        with pytest.raises(csdr_amd.CsdrAmdError):
            ctx.generic_slicer_f_u8(np.zeros(4, np.float32), ns)
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.plain_interpolate_cc(np.zeros(4, np.complex64), 0)
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.apply_real_fir_cc(np.zeros(4, np.complex64), np.zeros(0, np.float32))
    assert ctx.apply_real_fir_cc(np.zeros(4, np.complex64), np.ones(5, np.float32)).size == 0


def test_slicer_threshold_points(ctx):
    """every limit -2 .. +2 ulp, the random inputs and the specials: the kernel equals the float32 model everywhere"""
    for ns in tc.SLICER_N:
        x, _ = tc.slicer_points(ns, 20000)
        assert np.array_equal(ctx.generic_slicer_f_u8(x, ns), pm.slicer(x, ns)), ns


# ------------------------------------------------------------------ drop-in functions
def test_dropin_functions_vs_reference(ctx):
    import csdr_amd
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built (oracle/_ref/libcsdr_ref.so)")
    A = tc.bind_modem(C.CDLL(csdr_amd.lib()._name)); R = tc.bind_modem(C.CDLL(REF_LIB))
    rng = np.random.default_rng(9)
    c = (rng.standard_normal(700) + 1j * rng.standard_normal(700)).astype(np.complex64)
    assert bits_eq(tc.lib_interpolate(A, c[:100], 7), tc.lib_interpolate(R, c[:100], 7))
    taps = tc.test_taps(1, 65)
    ya, yr = tc.lib_fir(A, c, taps), tc.lib_fir(R, c, taps)
    want, mr, mi = pm.shape64(c, 1, taps)
    assert ya.size == yr.size == 700 - 64
    assert pm.within(ya, want, pm.dot_gate(65, mr), pm.dot_gate(65, mi)) and pm.within(yr, want, pm.dot_gate(65, mr), pm.dot_gate(65, mi))
    assert tc.lib_fir(A, c[:10], taps).size == 0 == tc.lib_fir(R, c[:10], taps).size
    for ns in (2, 4, 16):
        x, near = tc.slicer_points(ns, 5000)
        got = tc.lib_slicer(A, x, ns, fill=77)
        assert np.array_equal(got, pm.slicer(x, ns)) and np.array_equal(got[~near], tc.lib_slicer(R, x, ns)[~near])
    assert tc.lib_slicer(A, np.array([np.nan, 0.9], np.float32), 4, fill=77).tolist() == [0, 3]
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(tc.lib_pack_1to8(A, every), tc.lib_pack_1to8(R, every))
    g = rng.choice(np.array([0, 1, 2, 255], np.uint8), (300, 8))
    assert np.array_equal(tc.lib_pack_8to1(A, g), tc.lib_pack_8to1(R, g))
    for (sps, T, beta) in tc.RRC_CASES:
        a, r = tc.lib_rrc(A, T, sps, beta), tc.lib_rrc(R, T, sps, beta)
        assert a[T] == r[T] == np.float32(12345.0) and np.max(np.abs(a[:T] - r[:T])) <= 1e-6 * np.max(np.abs(r[:T]))
    for sps in tc.COSINE_SPS:
        a, r = tc.lib_cosine(A, sps), tc.lib_cosine(R, sps)
        assert np.max(np.abs(a - r)) <= 1e-6 * np.max(np.abs(r))


# ------------------------------------------------------------------ CLI
def _run(cmd, data, shell=False, timeout=120):
    r = subprocess.run(cmd, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, shell=shell)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr.decode()


def _ref(args, data):
    if not os.path.exists(REF_CSDR):
        pytest.skip("reference binary not built (oracle/_ref/csdr)")
    return subprocess.run([REF_CSDR] + args, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120).stdout


def test_cli_commands_vs_reference_binary(ctx):
    """whole blocks of the reference's 1024-element buffer through real pipes; behind them the reference writes a stale block at EOF, so its
    output is compared over the whole blocks only"""
    rng = np.random.default_rng(17)
    B = 1024
    c = (rng.standard_normal(3 * B) + 1j * rng.standard_normal(3 * B)).astype(np.complex64)
    out, _ = _run([CSDR, "plain_interpolate_cc", "5"], c.tobytes())
    assert out == pm.stuffed(c, 5)[0].tobytes() and _ref(["plain_interpolate_cc", "5"], c.tobytes())[:len(out)] == out
    x = rng.uniform(-1.5, 1.5, 3 * B).astype(np.float32)
    out, _ = _run([CSDR, "generic_slicer_f_u8", "4"], x.tobytes())
    assert out == pm.slicer(x, 4).tobytes() and _ref(["generic_slicer_f_u8", "4"], x.tobytes())[:len(out)] == out
    b = rng.integers(0, 256, 3 * B).astype(np.uint8)
    out, _ = _run([CSDR, "pack_bits_1to8_u8_u8"], b.tobytes())
    assert out == pm.pack_1to8(b).tobytes() and _ref(["pack_bits_1to8_u8_u8"], b.tobytes())[:len(out)] == out
    g = rng.choice(np.array([0, 1, 2, 255], np.uint8), 3 * B)
    out, _ = _run([CSDR, "pack_bits_8to1_u8_u8"], g.tobytes())
    assert out == pm.pack_8to1(g).tobytes() and _ref(["pack_bits_8to1_u8_u8"], g.tobytes())[:len(out)] == out
    # the filter: the stream's valid correlation; the reference consumes 1024 - T + 1 samples per pass, so it has written at least the outputs of
    # the samples in front of the last pass
    for args, taps in [(["RRC", "8", "65", "0.35"], pm.firdes_rrc(65, 8, 0.35)), (["COSINE", "4"], pm.firdes_cosine(4))]:
        out, _ = _run([CSDR, "pulse_shaping_filter_cc"] + args, c.tobytes())
        y = np.frombuffer(out, np.complex64)
        want, mr, mi = pm.shape64(c, 1, taps)
        assert y.size == c.size - taps.size + 1 and pm.within(y, want, pm.dot_gate(taps.size, mr), pm.dot_gate(taps.size, mi))
        out, _ = _run([CSDR, "firdes_pulse_shaping_filter_f"] + args, b"")
        assert out == b"".join(b"%f " % float(v) for v in taps)
        if args[0] == "COSINE":
            continue                                          # (the reference's cosine design normalises two taps it never wrote: whatever malloc held)
        r = np.frombuffer(_ref(["pulse_shaping_filter_cc"] + args, c.tobytes()), np.complex64)
        k = min(r.size, y.size)
        assert k >= c.size - 2 * B and pm.within(r[:k], want[:k], pm.dot_gate(taps.size, mr[:k]), pm.dot_gate(taps.size, mi[:k]))
        rt = np.array(_ref(["firdes_pulse_shaping_filter_f"] + args, b"").split(), np.float64)
        assert rt.size == taps.size and np.max(np.abs(rt - np.array(out.split(), np.float64))) <= 1.5e-6      # ("%f": six decimals)


def test_cli_chain_is_fused(ctx):
    rng = np.random.default_rng(23)
    idx = rng.integers(0, 4, 3000).astype(np.uint8)
    taps = pm.firdes_rrc(65, 8, 0.35)
    pipe = "%s psk_modulator_u8_c 4 | %s plain_interpolate_cc 8 | %s pulse_shaping_filter_cc RRC 8 65 0.35" % ((CSDR,) * 3)
    three, _ = _run(pipe, idx.tobytes(), shell=True)
    out, err = _run([CSDR, "chain", "psk_modulator_u8_c 4 | plain_interpolate_cc 8 | pulse_shaping_filter_cc RRC 8 65 0.35"], idx.tobytes())
    assert "fused pulse-shaping transmit object" in err and "psk_modulator_u8_c .. pulse_shaping_filter_cc recognised" in err
    y = np.frombuffer(out, np.complex64)
    sym = pm.symbols(4)[idx]
    assert bits_eq(y, pm.shape32(sym, 8, taps))                                        # the object's stream, to the bit
    z = np.frombuffer(three, np.complex64)
    want, mr, mi = pm.shape64(sym, 8, taps)
    assert z.size == y.size == 3000 * 8 - 64
    assert pm.within(z, y.astype(np.complex128), pm.dot_gate(9 + 65, mr), pm.dot_gate(9 + 65, mi))
    # the two-stage run takes complex symbols
    out2, err2 = _run([CSDR, "chain", "plain_interpolate_cc 8 | pulse_shaping_filter_cc RRC 8 65 0.35"], sym.tobytes())
    assert "plain_interpolate_cc .. pulse_shaping_filter_cc recognised" in err2 and out2 == out


@pytest.mark.parametrize("args,message", [
    (["plain_interpolate_cc"], b"required parameter <interpolation> is missing."),
    (["plain_interpolate_cc", "0"], b"interpolation should be >0"),
    (["pulse_shaping_filter_cc"], b"required parameter <pulse_shaping_filter_type> is missing."),
    (["pulse_shaping_filter_cc", "RRC"], b"required parameter <samples_per_symbol> is missing."),
    (["pulse_shaping_filter_cc", "RRC", "8"], b"required parameter <num_taps> is missing."),
    (["pulse_shaping_filter_cc", "RRC", "8", "65"], b"required parameter <beta> is missing."),
    (["pulse_shaping_filter_cc", "RRC", "8", "64", "0.35"], b"num_taps should be odd"),
    (["pulse_shaping_filter_cc", "COSINE"], b"required parameter <samples_per_symbol> is missing."),
    (["firdes_pulse_shaping_filter_f"], b"required parameter <pulse_shaping_filter_type> is missing."),
    (["generic_slicer_f_u8"], b"required parameter <n_symbols> is missing."),
    (["generic_slicer_f_u8", "1"], b"n_symbols should be between 2 and 256"),
    (["chain", "psk_modulator_u8_c 4 | plain_interpolate_cc 8 | pulse_shaping_filter_cc RRC 8"], b"required parameter <num_taps> is missing."),
])
def test_cli_bad_syntax(ctx, args, message):
    r = subprocess.run([CSDR] + args, input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode != 0 and message in r.stderr and r.stdout == b""


# ------------------------------------------------------------------ round trip
def test_round_trip_through_matched_filter_and_slicer(ctx):
    """64 channels x 512 QPSK symbols (+-1 +-1j), root raised cosine 8 / 65 / 0.35 on both sides: the pair's response peaks 64 samples in, symbol m sits
    at output 8 m - 64 of the second filter; its I and Q sliced into two levels are the sent bits (the eye at beta 0.35 is open by far more than any
    float error, so no tolerance)"""
    import csdr_amd
    rng = np.random.default_rng(41)
    bits = rng.integers(0, 2, (64, 512, 2)).astype(np.uint8)
    c = ((2.0 * bits[..., 0] - 1) + 1j * (2.0 * bits[..., 1] - 1)).astype(np.complex64)
    taps = csdr_amd.firdes_rrc_f(65, 8, 0.35)
    with ctx.pulse_tx(64, 4, 8, taps, "shape", "shape") as o:
        y = o.process(c)
        assert o.kernel_name() == POLY and y.shape == (64, 512 * 8 - 64)
    z = ctx.apply_real_fir_cc(y, taps)
    assert z.shape == (64, 512 * 8 - 128)
    m = np.arange(8, 504)
    at = z[:, 8 * m - 64]
    assert np.array_equal(ctx.generic_slicer_f_u8(np.ascontiguousarray(at.real), 2), bits[:, 8:504, 0])
    assert np.array_equal(ctx.generic_slicer_f_u8(np.ascontiguousarray(at.imag), 2), bits[:, 8:504, 1])


# ------------------------------------------------------------------ lifecycle and arguments
def test_argument_errors(ctx):
    import csdr_amd
    t = np.ones(5, np.float32)
    for bad in [dict(first="shape", last="mod"), dict(first=0, last=2), dict(first=-1, last=1), dict(interpolation=0), dict(taps=np.zeros(0, np.float32)),
                dict(taps=None), dict(n_psk=0), dict(n_psk=257), dict(n_channels=0)]:
        with pytest.raises(csdr_amd.CsdrAmdError):
            ctx.pulse_tx(**{**dict(n_channels=2, n_psk=4, interpolation=2, taps=t), **bad})
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.pulse_tx(1, 0, 1, None, "mod", "mod")


def test_lifecycle(ctx):
    import csdr_amd
    import torch
    m = case(8, 65)
    o = ctx.pulse_tx(3, 4, 8, m["taps"])
    o.process(m["idx"][:3])
    o.close(); o.close()                                                               # twice
    c2 = csdr_amd.Context(0)
    o2 = c2.pulse_tx(1, 4, 8, m["taps"])
    c2.close(); o2.close()                                                             # after its context

    def cycle():
        with ctx.pulse_tx(65, 4, 8, m["taps"]) as p:
            p.process(m["idx"])
    cycle(); ctx.sync()
    f0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(30):
        cycle()
    assert torch.cuda.mem_get_info(0)[0] >= f0 - (4 << 20)
