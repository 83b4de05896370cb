"""GPU checks of the RTTY receive chain (rtty.hip): every stage range against the CPU walk of the same step functions bit for bit and the discriminator
against float64 within its gate, the fused object against the reference library, cut and batch invariance, channel reset, the matrix-core and generic
discriminators bit for bit, the CLI commands and `csdr chain` fusion against the reference binary, the drop-in symbols, and lifecycle."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import rtty_model as rm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_CSDR = os.path.join(ROOT, "oracle", "_ref", "csdr")
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
TEXT = "RYRY CQ DE TEST 0123456789 THE QUICK BROWN FOX, ?/ ()"
B = 4096
RANGES = [("bfsk", "bfsk"), ("bfsk", "serial"), ("bfsk", "baudot"), ("serial", "serial"), ("serial", "baudot"), ("baudot", "baudot")]


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _params(**kw):
    import csdr_amd
    kw.setdefault("cli_bufsize", B)
    return csdr_amd.rtty_params(**kw)


def _signals(n_ch, n=None, snr=12):
    """n_ch generated channels of equal length, each ending in at least 2 B idle samples"""
    kws = [dict(snr_db=snr, carrier=0.0004 * ((k % 5) - 2), bit_phase=0.13 * k, seed=k, lead=1000 + 37 * k) for k in range(n_ch)]
    lens = [len(rm.rtty_signal(TEXT, **kw)) for kw in kws]
    total = max(lens) + 2 * B
    out = np.stack([rm.rtty_signal(TEXT, tail=total - lens[k], **kws[k]) for k in range(n_ch)])
    return out[:, :n] if n else out


def _inputs(p, x):
    """each stage's input for one channel, from the CPU walk"""
    import csdr_amd
    y = csdr_amd.rtty_debug_walk(p, "bfsk", "bfsk", x)
    codes = csdr_amd.rtty_debug_walk(p, "serial", "serial", y)
    return {"bfsk": x, "serial": y, "baudot": codes}


def test_every_stage_range_vs_walk(ctx):
    """all six stage ranges on the GPU equal csdr_amd_debug_rtty_walk bit for bit; the discriminator is within the float64 gate"""
    import csdr_amd
    x = _signals(3)
    p = _params()
    m, s = rm.bfsk_taps(0.02125, 101)
    for first, last in RANGES:
        o = ctx.rtty(p, 3, first, last)
        ins = [_inputs(p, x[k])[first] for k in range(3)]
        n = min(len(v) for v in ins)
        got = o.process(np.stack([v[:n] for v in ins]))
        for k in range(3):
            want = csdr_amd.rtty_debug_walk(p, first, last, ins[k][:n])
            assert got[k].dtype == want.dtype and np.array_equal(got[k].view(np.uint8), want.view(np.uint8)), (first, last, k)
            if last == "baudot":
                assert bytes(got[k]) == TEXT.upper().encode()
        if first == "bfsk":
            assert o.kernel_name() == "k_bfsk_mfma"
            if last == "bfsk":
                for k in range(3):
                    y64 = rm.bfsk64(x[k], m, s)
                    assert got[k].size == y64.size and np.all(np.abs(got[k] - y64) <= rm.bfsk_gate(x[k], m, s))
        else:
            assert o.kernel_name() == ("k_rtty_baudot" if first == "baudot" else "k_rtty_walk")
        o.close()


def test_walk_exact_on_gpu_floats(ctx):
    """the serial decoder and Baudot lookup on the GPU's own discriminator rows: exactly the model"""
    x = _signals(2, snr=6)
    p = _params()
    yb = ctx.rtty(p, 2, "bfsk", "bfsk").process(x)
    codes = ctx.rtty(p, 2, "bfsk", "serial").process(x)
    text = ctx.rtty(p, 2, "bfsk", "baudot").process(x)
    for k in range(2):
        want = rm.serial_stream(yb[k], 176.0176, 5, 1.5, B)
        assert list(codes[k]) == want
        assert bytes(text[k]) == rm.baudot(want)


def test_fused_vs_reference(ctx):
    """the fused object gives the reference functions' text on clean and moderate-SNR signals"""
    L = rm.ref_lib()
    if L is None:
        pytest.skip("reference library not built")
    for snr in (None, 20, 8):
        xs = [rm.rtty_signal(TEXT, snr_db=snr, carrier=0.0007 + 0.0002 * k, bit_phase=0.29 * k, seed=40 + k, tail=2 * 16384) for k in range(4)]
        n = min(len(v) for v in xs)
        x = np.stack([v[:n] for v in xs])
        got = ctx.rtty(_params(cli_bufsize=16384), 4, "bfsk", "baudot").process(x)
        for k in range(4):
            assert bytes(got[k]) == rm.ref_chain(L, x[k]) == TEXT.upper().encode(), (snr, k)


def test_cut_invariance(ctx):
    """output does not depend on the call cuts: cuts shorter than L and than B, single samples"""
    x = _signals(2)
    n = x.shape[1]
    p = _params()
    for first, last in [("bfsk", "bfsk"), ("bfsk", "baudot"), ("bfsk", "serial")]:
        whole = ctx.rtty(p, 2, first, last).process(x)
        rng = np.random.default_rng(1)
        for calls in ([1] * 150 + [50, 99, 100, 101, B - 1, B, B + 1], list(rng.integers(0, B, 12))):
            calls = [int(c) for c in calls]
            calls.append(n - sum(calls))
            assert calls[-1] >= 0
            cut = ctx.rtty(p, 2, first, last).process(x, calls)
            for k in range(2):
                assert np.array_equal(cut[k].view(np.uint8), whole[k].view(np.uint8)), (first, last, k)


def test_batch_position_and_reset_channel(ctx):
    """a channel's output does not depend on its batch position; reset_channel starts it afresh"""
    x = _signals(37)
    p = _params()
    o = ctx.rtty(p, 37)
    got = o.process(x)
    single = ctx.rtty(p, 1)
    for k in (0, 1, 17, 36):
        single.reset()
        assert bytes(single.process(x[k])) == bytes(got[k])
    h = x.shape[1] // 2
    o.reset()
    first = o.process(x[:, :h])
    o.reset_channel(5)
    second = o.process(x[:, h:])
    fresh = ctx.rtty(p, 1).process(x[5, h:])
    assert bytes(second[5]) == bytes(fresh)
    assert bytes(np.concatenate([first[6], second[6]])) == bytes(got[6])


def test_force_generic_identical_bits(ctx):
    """k_bfsk_generic gives the matrix-core kernel's bits; kernel_name names the instance that ran"""
    x = _signals(5)
    p = _params()
    a = ctx.rtty(p, 5, "bfsk", "bfsk")
    ya = a.process(x)
    assert a.kernel_name() == "k_bfsk_mfma"
    g = ctx.rtty(p, 5, "bfsk", "bfsk")
    g.force_generic(True)
    yg = g.process(x, [777, 1, 5000, x.shape[1] - 5778])
    assert g.kernel_name() == "k_bfsk_generic"
    for k in range(5):
        assert np.array_equal(ya[k].view(np.uint32), yg[k].view(np.uint32))
    # a filter too long for the matrix cores runs generic and still matches the CPU walk
    import csdr_amd
    pl = _params(filter_length=301)
    o = ctx.rtty(pl, 2, "bfsk", "bfsk")
    yl = o.process(x[:2, :20000])
    assert o.kernel_name() == "k_bfsk_generic"
    assert np.array_equal(yl[1].view(np.uint32), csdr_amd.rtty_debug_walk(pl, "bfsk", "bfsk", x[1, :20000]).view(np.uint32))


def test_batch_functions(ctx):
    """csdr_amd_bfsk_demod_cf (caller taps, stateless), binary_slicer_f_u8 and rtty_line_decoder_u8_u8 against the model"""
    import csdr_amd
    x = _signals(3, n=30000)
    m, s = csdr_amd.firdes_peak_c(101, 0.010625), csdr_amd.firdes_peak_c(101, -0.010625)
    p = _params()
    for gen in (False, True):
        y = ctx.bfsk_demod_cf(x, m, s, force_generic=gen)
        assert ctx.last_bfsk_kernel == ("k_bfsk_generic" if gen else "k_bfsk_mfma")
        for k in range(3):
            assert np.array_equal(y[k].view(np.uint32), csdr_amd.rtty_debug_walk(p, "bfsk", "bfsk", x[k]).view(np.uint32))
    # the bit-per-sample variant
    rng = np.random.default_rng(3)
    lines = np.stack([np.repeat(2.0 * rng.integers(0, 2, 4000) - 1, 1) * rng.uniform(0.1, 2, 4000) for _ in range(2)]).astype(np.float32)
    bits = ctx.binary_slicer_f_u8(lines)
    assert np.array_equal(bits, (lines > 0).astype(np.uint8))
    txt = ctx.rtty_line_decoder_u8_u8(bits, [1, 999, 3000])
    for k in range(2):
        assert bytes(txt[k]) == rm.line_decoder(bits[k])


def _run(cmd, data, timeout=120, env=None):
    r = subprocess.run(cmd, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr.decode()


def test_cli_commands_and_chain(ctx):
    """the six commands and the fused chain against oracle/_ref/csdr through pipes (streams end in >= 2 B idle samples: the reference's stale last
    window adds nothing)"""
    if not os.path.exists(REF_CSDR):
        pytest.skip("reference binary not built")
    x = rm.rtty_signal(TEXT, snr_db=15, carrier=0.0006, bit_phase=0.4, seed=77, tail=3 * 16384)
    raw = x.tobytes()

    def ref(args, data):
        return subprocess.run([REF_CSDR] + args, input=data, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=120).stdout

    out, err = _run([CSDR, "bfsk_demod_cf", "0.02125", "101"], raw)
    y = np.frombuffer(out, np.float32)
    yr = np.frombuffer(ref(["bfsk_demod_cf", "0.02125", "101"], raw), np.float32)
    m, s = rm.bfsk_taps(0.02125, 101)
    # the whole valid correlation here; the reference stops at its last whole buffer (its feof check follows the short read): a prefix of it
    y64, gate = rm.bfsk64(x, m, s), rm.bfsk_gate(x, m, s)
    assert y.size == x.size - 100 and x.size - 100 - 1024 < yr.size <= y.size
    assert np.all(np.abs(yr - y64[:yr.size]) <= gate[:yr.size])
    assert np.all(np.abs(y - y64) <= gate)
    codes, _ = _run([CSDR, "serial_line_decoder_f_u8", "176.0176", "5", "1.5"], y.tobytes())
    assert codes == bytes(ref(["serial_line_decoder_f_u8", "176.0176", "5", "1.5"], y.tobytes()))
    text, _ = _run([CSDR, "rtty_baudot2ascii_u8_u8"], codes)
    assert text == ref(["rtty_baudot2ascii_u8_u8"], codes) == TEXT.upper().encode()
    lines = np.sign(np.sin(np.arange(20000) * 0.013)).astype(np.float32) + 0.25
    b, _ = _run([CSDR, "binary_slicer_f_u8"], lines.tobytes())
    assert len(b) == lines.size and b == ref(["binary_slicer_f_u8"], lines.tobytes())[:lines.size]     # (the reference pads its last buffer)
    rng = np.random.default_rng(8)
    bits = rng.integers(0, 2, 30000).astype(np.uint8)
    bits[::5] = 1
    t2, _ = _run([CSDR, "rtty_line_decoder_u8_u8"], bits.tobytes())
    assert t2 == rm.line_decoder(bits)
    pk, _ = _run([CSDR, "firdes_peak_c", "0.010625", "101"], b"")
    parse = lambda t: np.array([complex(v.replace(")+(", "+").replace(")*i", "j").lstrip("(").replace("+-", "-")) for v in t.decode().split()])
    assert np.allclose(parse(pk), parse(ref(["firdes_peak_c", "0.010625", "101"], b"")), rtol=0, atol=2e-6)
    r = subprocess.run([CSDR, "firdes_peak_c", "0.01", "11", "HAMMING", "--octave"], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode != 0
    # the fused chain, and the same commands through three reference processes
    chain = "bfsk_demod_cf 0.02125 101 | serial_line_decoder_f_u8 176.0176 5 1.5 | rtty_baudot2ascii_u8_u8"
    out, err = _run([CSDR, "chain", chain], raw)
    assert "rtty_rx" in err
    want = subprocess.run(["sh", "-c", "%s bfsk_demod_cf 0.02125 101 | %s serial_line_decoder_f_u8 176.0176 5 1.5 | %s rtty_baudot2ascii_u8_u8" % ((REF_CSDR,) * 3)],
                          input=raw, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=120).stdout
    assert out == want == TEXT.upper().encode()
    # the device hand-off between two of our processes
    piped = subprocess.run(["sh", "-c", "%s bfsk_demod_cf 0.02125 101 | %s serial_line_decoder_f_u8 176.0176 5 1.5 | %s rtty_baudot2ascii_u8_u8" % ((CSDR,) * 3)],
                           input=raw, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert piped.returncode == 0 and piped.stdout == want


def test_argument_errors(ctx):
    import csdr_amd
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.rtty(_params(cli_bufsize=1000), 1)
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.rtty(_params(databits=9), 1)
    for args in (["serial_line_decoder_f_u8", "0.5"], ["serial_line_decoder_f_u8", "10", "9"], ["serial_line_decoder_f_u8", "10", "5", "0.5"],
                 ["serial_line_decoder_f_u8", "3000", "8", "2"], ["bfsk_demod_cf", "0.02"], ["firdes_peak_c", "0.01", "10"]):
        r = subprocess.run([CSDR] + args, input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode != 0, args


def test_lifecycle_no_growth(ctx):
    import torch
    x = np.zeros((64, 8192), np.complex64)

    def cycle():
        o = ctx.rtty(_params(), 64)
        o.process(x)
        o.close()
    cycle()
    f0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        cycle()
    f1 = torch.cuda.mem_get_info(0)[0]
    assert f1 >= f0 - (4 << 20)


def test_dropin_symbols_vs_reference(ctx):
    """bfsk_demod_cf, firdes_add_peak_c, serial_line_decoder_f_u8 (8- and 12-bit), binary_slicer_f_u8 and the Baudot functions of libcsdr_amd.so through
    ctypes, as a client built against the reference's headers calls them, against the reference library"""
    import csdr_amd
    A = C.CDLL(csdr_amd.lib()._name)
    A.bfsk_demod_cf.restype = C.c_int
    A.bfsk_demod_cf.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    A.firdes_add_peak_c.restype = None
    A.firdes_add_peak_c.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int]
    A.serial_line_decoder_f_u8.restype = None
    A.serial_line_decoder_f_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    A.binary_slicer_f_u8.restype = None
    A.binary_slicer_f_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    A.rtty_baudot_decoder_lookup.restype = C.c_char
    A.rtty_baudot_decoder_lookup.argtypes = [C.c_void_p, C.c_ubyte]
    A.rtty_baudot_decoder_push.restype = C.c_char
    A.rtty_baudot_decoder_push.argtypes = [C.c_void_p, C.c_ubyte]
    L = rm.ref_lib()
    x = rm.rtty_signal(TEXT, snr_db=15, carrier=0.0006, seed=5, tail=2 * 16384)
    m = rm.ref_peak(A, 101, 0.010625)
    s = rm.ref_peak(A, 101, -0.010625)
    assert np.array_equal(m, csdr_amd.firdes_peak_c(101, 0.010625))
    acc = np.zeros(101, np.complex64)
    A.firdes_add_peak_c(rm._p(acc), 101, 0.01, 2, 1, 0)
    A.firdes_add_peak_c(rm._p(acc), 101, -0.02, 2, 1, 1)
    y = rm.ref_bfsk(A, x, m, s)
    assert np.all(np.abs(y - rm.bfsk64(x, m, s)) <= rm.bfsk_gate(x, m, s))
    assert rm.ref_chain(A, x) == TEXT.upper().encode()
    for db in (5, 12):
        lines = np.concatenate([np.ones(50), -np.ones(30), np.ones(10), -np.ones(40), np.ones(300)] * 8).astype(np.float32)
        got = rm.ref_serial_window(A, lines, 9.5, db, 1.0)
        if L is not None:
            assert got == rm.ref_serial_window(L, lines, 9.5, db, 1.0)
            if db == 5:
                ra, rb = np.zeros(64, np.complex64), np.zeros(64, np.complex64)
                L.firdes_add_peak_c(rm._p(rb), 64, C.c_float(0.01), 2, 1, 0)
                L.firdes_add_peak_c(rm._p(rb), 64, C.c_float(-0.02), 2, 1, 1)
                A.firdes_add_peak_c(rm._p(ra), 64, 0.01, 2, 1, 0)
                A.firdes_add_peak_c(rm._p(ra), 64, -0.02, 2, 1, 1)
                assert np.allclose(ra, rb, rtol=0, atol=1e-6)
        assert got == rm.serial_window(lines, 9.5, db, 1.0)
    sl = np.zeros(lines.size, np.uint8)
    A.binary_slicer_f_u8(rm._p(lines), rm._p(sl), lines.size)
    assert np.array_equal(sl, (lines > 0).astype(np.uint8))
    st = rm.BaudotDecoder()
    out = [A.rtty_baudot_decoder_push(C.byref(st), int(b))[0] for b in sl]
    assert bytes(o for o in out if o) == rm.line_decoder(sl)
