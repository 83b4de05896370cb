"""CPU checks of the RTTY receive chain: the float32 model (rtty_model.py) against the reference library stage by stage, the discriminator's float64
gate (accepts float32 sums, rejects wrong filters), and the library's host side (the kernels' step functions through csdr_amd_debug_rtty_walk, the
Baudot functions, the filter design, the drop-in struct layouts, the parameter checks) against the model and the reference."""
import ctypes as C
import os
import numpy as np
import pytest

import rtty_model as rm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TEXT = "RYRY CQ CQ DE TEST 0123456789 THE QUICK BROWN FOX, ?/ ()"


@pytest.fixture(scope="module")
def ref():
    L = rm.ref_lib()
    if L is None:
        pytest.skip("reference library not built (oracle/_ref/libcsdr_ref.so)")
    return L


def line_signal(n_chars, spb, databits, stopbits, seed, lead=300, noise=0.15):
    """a discriminator-like line: +level idle, frames of start / data / stop bits with random gaps, random levels and noise (no exact zeros)"""
    rng = np.random.default_rng(seed)
    lv = []
    for _ in range(n_chars):
        lv += [1] * int(rng.integers(0, int(3 * spb)))
        bits = [0] + list(rng.integers(0, 2, databits)) + [1]
        for k, b in enumerate(bits):
            ln = spb * (stopbits if k == len(bits) - 1 else 1)
            lv += [b] * int(round(ln + rng.uniform(-0.3, 0.3)))
    lv = [1] * lead + lv + [1] * 400
    sgn = 2 * np.asarray(lv, np.float64) - 1
    y = sgn * rng.uniform(0.5, 1.5, len(sgn)) + noise * rng.standard_normal(len(sgn))
    y[y == 0] = 1e-3
    return y.astype(np.float32)


def _params(**kw):
    import csdr_amd
    return csdr_amd.rtty_params(**kw)


# ---------------------------------------------------------------- the model against the reference
def test_firdes_peak_c_matches_reference(ref):
    """firdes_add_peak_c within a few ulp of the reference's -ffast-math build, in the model and in the library"""
    import csdr_amd
    for L, r in [(101, 0.010625), (101, -0.010625), (31, 0.2), (255, 0.0013), (7, -0.4)]:
        want = rm.ref_peak(ref, L, r)
        for got in (rm.firdes_peak_c(L, r), csdr_amd.firdes_peak_c(L, r)):
            d = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
            scale = np.abs(want.view(np.float32)).max()
            assert np.all((d <= 64) | (np.abs(got.view(np.float32) - want.view(np.float32)) <= 1e-6 * scale)), (L, r, d.max())


@pytest.mark.parametrize("spb,databits,stopbits", [(176.0176, 5, 1.5), (9.7, 8, 1.0), (13.3, 5, 2.0), (21.0, 7, 1.5), (6.25, 5, 1.0)])
def test_serial_decoder_windows_match_reference(ref, spb, databits, stopbits):
    """window by window at several B: the model equals the reference bit for bit, with edges spread across the windows"""
    for seed in range(3):
        y = line_signal(60, spb, databits, stopbits, seed)
        for B in (int(spb * (databits + stopbits + 1)) + 4, 1024, 4096, 16384):
            if 2 + spb * (1 + databits + stopbits) >= B:
                continue
            want = rm.ref_serial_stream(ref, y, spb, databits, stopbits, B)
            assert rm.serial_stream(y, spb, databits, stopbits, B) == want, (seed, B)


def test_serial_decoder_lost_edge_and_reentry(ref):
    """a start edge on a window boundary is never seen; a character that does not fit re-enters 2 samples before its start bit"""
    spb, B = 10.5, 256
    y = np.ones(3 * B, np.float32)
    y[B:B + 40] = -1                                    # a start bit whose edge lies between two windows: never seen
    assert rm.ref_serial_stream(ref, y, spb, 5, 1.5, B) == rm.serial_stream(y, spb, 5, 1.5, B) == []
    y[B + 1:B + 40] = -1; y[B] = 1                      # one sample later it is seen
    assert rm.ref_serial_stream(ref, y, spb, 5, 1.5, B) == rm.serial_stream(y, spb, 5, 1.5, B) == [0b00011]
    o, used = rm.ref_serial_window(ref, np.concatenate([np.ones(150, np.float32), -np.ones(40, np.float32)]), spb, 5, 1.5)
    assert used == 148 and not o


def test_baudot_matches_reference(ref):
    """rtty_baudot_decoder_lookup and _push, model and library, bit for bit"""
    import csdr_amd
    for fig in (0, 1):
        for c in range(256):
            f = C.c_ubyte(fig)
            r = ref.rtty_baudot_decoder_lookup(C.byref(f), c)[0]
            got, f2 = csdr_amd.rtty_baudot_decoder_lookup(fig, c)
            assert (got, f2) == (r, f.value), (fig, c)
            assert rm.baudot([c], fig) == (bytes([r]) if r else b"")
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, 20000).astype(np.uint8)
    bits[::7] = 1
    st, mine = rm.BaudotDecoder(), csdr_amd.RttyPushState()
    want, got = [], []
    for b in bits:
        r = ref.rtty_baudot_decoder_push(C.byref(st), int(b))[0]
        if r:
            want.append(r)
        g = csdr_amd.rtty_baudot_decoder_push(mine, int(b))
        if g:
            got.append(g)
    assert bytes(got) == bytes(want) == rm.line_decoder(bits)


def test_generator_decodes_in_reference(ref):
    """the generator's signals (moderate SNR, carrier offsets, bit phases) decode to their text through the reference functions and the model"""
    for k, (snr, cf, ph) in enumerate([(20, 0.0007, 0.0), (10, -0.0011, 0.37), (6, 0.0003, 0.81)]):
        x = rm.rtty_signal(TEXT, snr_db=snr, carrier=cf, bit_phase=ph, seed=k, tail=2 * 16384)
        want = TEXT.upper().encode()
        assert rm.ref_chain(ref, x) == want
        assert rm.chain(x) == want


def test_binary_slicer_and_line_decoder_model(ref):
    x = rm.rtty_signal("HELLO 123", spb=1.0, snr_db=None)
    y = rm.bfsk64(x, *rm.bfsk_taps(0.02125, 101)).astype(np.float32)
    out = np.zeros(len(y), np.uint8)
    ref.binary_slicer_f_u8(rm._p(y), rm._p(out), len(y))
    assert np.array_equal(out, (y > 0).astype(np.uint8))


# ---------------------------------------------------------------- the discriminator's gate
def _signal():
    return rm.rtty_signal(TEXT[:20], snr_db=8, carrier=0.0009, bit_phase=0.3, seed=9)


def test_gate_accepts_float32_sums():
    """sequential and pairwise float32 sums, at the default and at other filter lengths, stay inside the gate"""
    x = _signal()
    for L in (101, 33, 257, 7):
        m, s = rm.bfsk_taps(0.02125, L)
        y64, g = rm.bfsk64(x, m, s), rm.bfsk_gate(x, m, s)
        for pw in (False, True):
            y = rm.bfsk32_seq(x, m, s, pairwise=pw)
            assert np.all(np.abs(y - y64) <= g), (L, pw)


def test_gate_rejects_wrong_filters():
    x = _signal()
    m, s = rm.bfsk_taps(0.02125, 101)
    y64, g = rm.bfsk64(x, m, s), rm.bfsk_gate(x, m, s)
    bad = {
        "swapped": rm.bfsk64(x, s, m),
        "reversed": rm.bfsk64(x, m[::-1].copy(), s[::-1].copy()),
        "conjugated": rm.bfsk64(x, np.conj(m), s),
        "dropped end tap": rm.bfsk64(x, np.concatenate([m[:-1], [0]]).astype(np.complex64), np.concatenate([s[:-1], [0]]).astype(np.complex64)),
        "misaligned": np.concatenate([rm.bfsk64(x, m, s)[1:], [0.0]]),
    }
    for name, y in bad.items():
        assert np.mean(np.abs(y - y64) > g) > 0.2, name


# ---------------------------------------------------------------- the library's host side
def test_debug_walk_equals_model_any_cuts():
    """csdr_amd_debug_rtty_walk: the discriminator within the gate of float64, and serial / Baudot exactly the model's on its own floats, whatever the cuts"""
    import csdr_amd
    B = 4096
    x = rm.rtty_signal(TEXT, snr_db=12, carrier=0.0005, seed=2, tail=2 * B)
    p = _params(cli_bufsize=B)
    m, s = rm.bfsk_taps(0.02125, 101)
    y = csdr_amd.rtty_debug_walk(p, "bfsk", "bfsk", x)
    y64 = rm.bfsk64(x, m, s)
    assert y.shape == y64.shape and np.all(np.abs(y - y64) <= rm.bfsk_gate(x, m, s))
    codes = rm.serial_stream(y, 176.0176, 5, 1.5, B)
    text = rm.baudot(codes)
    assert text == TEXT.upper().encode()
    rng = np.random.default_rng(0)
    for cuts in ([], [1, 1, 50, 99, 100, 101, 4095, 4096, 4097], list(rng.integers(0, 3000, 40)), [7] * 300):
        assert np.array_equal(csdr_amd.rtty_debug_walk(p, "bfsk", "bfsk", x, cuts).view(np.uint32), y.view(np.uint32))
        assert bytes(csdr_amd.rtty_debug_walk(p, "bfsk", "baudot", x, cuts)) == text
        assert list(csdr_amd.rtty_debug_walk(p, "serial", "serial", y, cuts)) == codes
        assert bytes(csdr_amd.rtty_debug_walk(p, "serial", "baudot", y, cuts)) == text
    c8 = np.asarray(codes + [27, 1, 2, 31, 1, 200, 0], np.uint8)
    assert bytes(csdr_amd.rtty_debug_walk(p, "baudot", "baudot", c8, [3, 1])) == rm.baudot(c8)


@pytest.mark.parametrize("spb,databits,stopbits,B", [(9.7, 8, 1.0, 1024), (13.3, 5, 2.0, 512), (6.25, 7, 1.5, 4096)])
def test_debug_walk_serial_equals_model(spb, databits, stopbits, B):
    import csdr_amd
    y = line_signal(80, spb, databits, stopbits, 4)
    p = _params(samples_per_bits=spb, databits=databits, stopbits=stopbits, cli_bufsize=B)
    want = rm.serial_stream(y, spb, databits, stopbits, B)
    for cuts in ([], [1] * 50 + [B - 1, B, B + 1], [333] * 20):
        assert list(csdr_amd.rtty_debug_walk(p, "serial", "serial", y, cuts)) == want


def test_argument_errors_cpu():
    """refused parameter sets, the "got stuck" window among them, fail through csdr_amd_debug_rtty_walk without a device"""
    import csdr_amd
    x = np.zeros(300, np.complex64)
    for kw in [dict(samples_per_bits=0.5), dict(databits=0), dict(databits=9), dict(stopbits=0.5), dict(filter_length=0),
               dict(cli_bufsize=0), dict(bit_sampling_width_ratio=1.5), dict(cli_bufsize=1322), dict(samples_per_bits=100.0, cli_bufsize=752)]:
        with pytest.raises(csdr_amd.CsdrAmdError):
            csdr_amd.rtty_debug_walk(_params(**kw), "bfsk", "baudot", x)
    csdr_amd.rtty_debug_walk(_params(cli_bufsize=1323), "bfsk", "baudot", x)      # 2 + 176.0176 * 7.5 = 1322.13: B = 1322 gets stuck, 1323 does not
    with pytest.raises(csdr_amd.CsdrAmdError):
        csdr_amd.rtty_debug_walk(_params(), "serial", "bfsk", x.real)
    y = np.zeros(100, np.float32)
    assert csdr_amd.rtty_debug_walk(_params(databits=16), "serial", "serial", y).dtype == np.uint16


def test_compat_struct_layout():
    """serial_line_t and rtty_baudot_decoder_t as libcsdr.h:252-284 lays them out (the drop-in header declares the same)"""
    hdr = open(os.path.join(ROOT, "include", "libcsdr_amd_compat.h")).read()
    for name in ("serial_line_t", "rtty_baudot_decoder_t", "bfsk_demod_cf", "firdes_add_peak_c", "serial_line_decoder_f_u8", "binary_slicer_f_u8",
                 "rtty_baudot_decoder_lookup", "rtty_baudot_decoder_push"):
        assert name in hdr
    assert C.sizeof(rm.SerialLine) == 24 and [getattr(rm.SerialLine, f[0]).offset for f in rm.SerialLine._fields_] == [0, 4, 8, 12, 16, 20]
    assert C.sizeof(rm.BaudotDecoder) == 12 and [getattr(rm.BaudotDecoder, f[0]).offset for f in rm.BaudotDecoder._fields_] == [0, 1, 2, 4, 8]
