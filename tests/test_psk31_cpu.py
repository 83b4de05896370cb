"""CPU checks of the BPSK31 receive chain: the float32 model (psk31_model.py) against the reference library stage by stage, the signal generator against
the reference's transmit helpers, and the library's host side (the kernel's step functions through csdr_amd_debug_psk31_walk, the varicode table and
decoder, the drop-in struct layout) against the model and the reference."""
import ctypes as C
import os
import numpy as np
import pytest

import psk31_model as pm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")
TIMING_GRID = [(D, alg, q) for D in (256, 8, 12, 40) for alg in (pm.GARDNER, pm.EARLYLATE) for q in (True, False)]


class TRState(C.Structure):                 # timing_recovery_state_t (libcsdr.h:319-333)
    _fields_ = [("algorithm", C.c_int), ("decimation_rate", C.c_int), ("output_size", C.c_int), ("input_processed", C.c_int), ("use_q", C.c_int),
                ("debug_phase", C.c_int), ("debug_every_nth", C.c_int), ("debug_writefiles_path", C.c_char_p), ("last_correction_offset", C.c_int),
                ("earlylate_ratio", C.c_float), ("loop_gain", C.c_float), ("max_error", C.c_float)]


class VItem(C.Structure):                   # psk31_varicode_item_t (libcsdr.h:267-272)
    _fields_ = [("code", C.c_ulonglong), ("bitcount", C.c_int), ("ascii", C.c_ubyte)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built (oracle/_ref/libcsdr_ref.so)")
    L = C.CDLL(REF_LIB)
    L.simple_agc_cc.restype = None
    L.simple_agc_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p]
    L.timing_recovery_init.restype = TRState
    L.timing_recovery_init.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_char_p]
    L.timing_recovery_cc.restype = None
    L.timing_recovery_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(TRState)]
    L.dbpsk_decoder_c_u8.restype = None
    L.dbpsk_decoder_c_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.psk31_varicode_decoder_push.restype = C.c_char
    L.psk31_varicode_decoder_push.argtypes = [C.POINTER(C.c_ulonglong), C.c_ubyte]
    L.psk31_varicode_encoder_u8_u8.restype = None
    L.psk31_varicode_encoder_u8_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.differential_codec.restype = C.c_ubyte
    L.differential_codec.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_ubyte]
    return L


# ------------------------------------------------------------------ reference wrappers (shared with the GPU tests)
def ref_agc(L, x, rate, reference=1.0, max_gain=65535.0, gain=1.0):
    x = np.ascontiguousarray(x, np.complex64)
    y = np.empty_like(x)
    g = C.c_float(gain)
    L.simple_agc_cc(_p(x), _p(y), x.size, rate, reference, max_gain, C.byref(g))
    return y, g.value


def ref_timing(L, x, algorithm, decimation, loop_gain=0.5, max_error=2.0, use_q=False):
    """one timing_recovery_cc call over the whole of x -> (symbols, errors, indexes, input_processed)"""
    x = np.ascontiguousarray(x, np.complex64)
    st = L.timing_recovery_init(algorithm, decimation, int(use_q), loop_gain, max_error, -1, None)
    out = np.zeros(x.size, np.complex64); err = np.zeros(x.size, np.float32); idx = np.zeros(x.size, np.int32)
    L.timing_recovery_cc(_p(x), _p(out), x.size, _p(err), _p(idx), C.byref(st))
    k = st.output_size
    return out[:k], err[:k], idx[:k].astype(np.int64), st.input_processed


def ref_dbpsk(L, s):
    z = np.zeros(1, np.complex64); zb = np.zeros(1, np.uint8)
    L.dbpsk_decoder_c_u8(_p(z), _p(zb), 1)                     # the function-level static last_input back to 0 + 0i
    s = np.ascontiguousarray(s, np.complex64)
    b = np.zeros(max(s.size, 1), np.uint8)
    if s.size:
        L.dbpsk_decoder_c_u8(_p(s), _p(b), s.size)
    return b[:s.size]


def ref_varicode(L, bits):
    shr = C.c_ulonglong(0)
    out = bytearray()
    for b in np.asarray(bits).tolist():
        c = L.psk31_varicode_decoder_push(C.byref(shr), b)
        if c != b"\x00":
            out += c
    return bytes(out)


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a); b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def _sig(n, seed, amp=0.3):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * amp
    x[::97] = 0                                                # zero amplitude: the gain goes to max_gain
    return x.astype(np.complex64)


# ------------------------------------------------------------------ the model against the reference
def test_agc_model_vs_ref(ref):
    x = _sig(30000, 1)
    for rate, refl, mg in [(0.001, 0.5, 65535.0), (0.05, 1.0, 3.0), (0.3, 0.2, 100.0)]:
        want, gw = ref_agc(ref, x, rate, refl, mg)
        got, gg = pm.agc(x, rate, refl, mg)
        for a, b in [(got.real, want.real), (got.imag, want.imag)]:
            close = (ulp_diff(a, b) <= 4) | (np.abs(a - b) <= 1e-6 * np.abs(b))
            assert close.all(), (rate, np.flatnonzero(~close)[:5])
        assert abs(gg - gw) <= 1e-6 * abs(gw)


@pytest.mark.parametrize("D,alg,use_q", TIMING_GRID)
def test_timing_model_vs_ref(ref, D, alg, use_q):
    x = pm.psk31_signal("cq cq de test " * 3, decimation=D, carrier=0.0007, phase=0.4, timing_offset=D // 3 + 1, snr_db=15, seed=D)
    a, _ = ref_agc(ref, x, 0.001, 0.5, 65535.0)                 # fed the reference's own AGC output
    ws, we, wi, wp = ref_timing(ref, a, alg, D, 0.5, 2.0, use_q)
    gs, ge, gi, gp, _ = pm.timing(a, alg, D, 0.5, 2.0, use_q)
    assert ws.size > 50
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
    assert np.array_equal(ge.view(np.uint32), we.view(np.uint32))
    assert np.array_equal(gi, wi) and gp == wp


def test_dbpsk_model_vs_ref(ref):
    rng = np.random.default_rng(3)
    s = ((rng.standard_normal(20000) + 1j * rng.standard_normal(20000))).astype(np.complex64)
    s[5] = 0; s[6] = -1; s[7] = 1j; s[8] = -1j                # exact axes and the origin
    assert np.array_equal(pm.dbpsk(s), ref_dbpsk(ref, s))


def test_varicode_model_vs_ref(ref):
    rng = np.random.default_rng(4)
    bits = (rng.random(1_000_000) < 0.6).astype(np.uint8)
    got, _ = pm.varicode_decode(bits[:200_000])                # the model's table scan is slow in Python: 2e5 bits here, 1e6 through the library below
    assert got == ref_varicode(ref, bits[:200_000])


def test_varicode_table_vs_ref(ref):
    n = C.c_int.in_dll(ref, "n_psk31_varicode_items").value
    items = (VItem * n).in_dll(ref, "psk31_varicode_items")
    tab = {it.ascii: (it.code, it.bitcount) for it in items}
    assert len(tab) == n == 128
    for a, c in enumerate(pm.VARICODE):
        assert tab[a] == (int(c, 2), len(c)), a
    import csdr_amd
    lt = csdr_amd.psk31_varicode_table()
    for a in range(128):
        assert (lt[a, 0], lt[a, 1]) == tab[a], a


def test_library_varicode_push_vs_ref(ref):
    """the O(1) lookup against the reference's table scan: 1e6 random bits, and every table entry between separators"""
    import csdr_amd
    L = csdr_amd.lib()
    rng = np.random.default_rng(5)
    bits = (rng.random(1_000_000) < 0.55).astype(np.uint8).tolist()
    for a in range(128):
        bits += [int(b) for b in pm.VARICODE[a]] + [0, 0]
    rs, ls = C.c_ulonglong(0), C.c_ulonglong(0)
    for k, b in enumerate(bits):
        r = ref.psk31_varicode_decoder_push(C.byref(rs), b)
        g = L.csdr_amd_psk31_varicode_decoder_push(C.byref(ls), b)
        if r != g or rs.value != ls.value:
            raise AssertionError("bit %d: ref %r lib %r" % (k, r, g))


# ------------------------------------------------------------------ the generator against the reference's transmit helpers
def test_generator_vs_ref(ref):
    text = b"Hello, PSK31 {|}~ \x01 world"
    inp = np.frombuffer(text, np.uint8).copy()
    out = np.zeros(len(text) * 12 + 8, np.uint8)
    ip, op = C.c_int(0), C.c_int(0)
    ref.psk31_varicode_encoder_u8_u8(_p(inp), _p(out), inp.size, out.size, C.byref(ip), C.byref(op))
    enc = pm.varicode_encode(text)
    assert np.array_equal(out[:op.value], enc)
    d = np.zeros(enc.size, np.uint8)
    ref.differential_codec(_p(enc), _p(d), enc.size, 1, 0)
    assert np.array_equal(d, pm.differential_encode(enc))
    ref.psk31_interpolate_sine_cc.restype = None                # returns complexf by value: compare the samples only
    sym = np.where(d == 1, -1.0, 1.0).astype(np.complex64)
    y = np.zeros(sym.size * 16, np.complex64)
    class CF(C.Structure):
        _fields_ = [("i", C.c_float), ("q", C.c_float)]
    ref.psk31_interpolate_sine_cc.restype = CF
    ref.psk31_interpolate_sine_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, CF]
    ref.psk31_interpolate_sine_cc(_p(sym), _p(y), sym.size, 16, CF(0, 0))
    g = pm.interpolate_sine(sym, 16)
    assert np.abs(g - y).max() <= 1e-6


def test_generated_signal_decodes_in_model():
    x = pm.psk31_signal("the quick brown fox", decimation=64, carrier=0.0003, timing_offset=17, snr_db=20, seed=2)
    r = pm.chain(x, decimation=64)
    assert b"the quick brown fox" in r["text"]


# ------------------------------------------------------------------ the kernel's step functions (CPU run) against the model
def _params(**kw):
    import csdr_amd
    return csdr_amd.psk31_params(**kw)


@pytest.mark.parametrize("D,alg,use_q", TIMING_GRID[:6])
def test_debug_walk_vs_model(D, alg, use_q):
    import csdr_amd
    x = pm.psk31_signal("walk test 123", decimation=D, carrier=0.0011, timing_offset=D // 2 + 3, snr_db=12, seed=7 + D)
    P = _params(rate=0.001, reference=0.5, max_gain=65535.0, algorithm=alg, decimation=D, loop_gain=0.5, max_error=2.0, use_q=use_q)
    a, g = pm.agc(x, 0.001, 0.5)
    ws, we, wi, _, _ = pm.timing(a, alg, D, 0.5, 2.0, use_q)
    wb = pm.dbpsk(ws)
    wt, _ = pm.varicode_decode(wb)
    # every stage range, one call
    ga = csdr_amd.psk31_debug_walk(P, "agc", "agc", x)
    assert np.array_equal(ga.view(np.uint32), a.view(np.uint32))
    gs, ge, gi = csdr_amd.psk31_debug_walk(P, "agc", "timing", x, with_extras=True)
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)) and np.array_equal(ge.view(np.uint32), we.view(np.uint32))
    assert np.array_equal(gi.astype(np.int64), wi)
    st, _, _ = csdr_amd.psk31_debug_walk(P, "timing", "timing", a, with_extras=True)
    assert np.array_equal(st.view(np.uint32), ws.view(np.uint32))
    assert np.array_equal(csdr_amd.psk31_debug_walk(P, "agc", "dbpsk", x), wb)
    assert np.array_equal(csdr_amd.psk31_debug_walk(P, "dbpsk", "dbpsk", ws), wb)
    assert csdr_amd.psk31_debug_walk(P, "agc", "varicode", x).tobytes() == wt
    assert csdr_amd.psk31_debug_walk(P, "varicode", "varicode", wb).tobytes() == wt
    # cut invariance: random cuts, 0- and 1-sample calls, cuts inside a symbol and inside the tail
    rng = np.random.default_rng(D)
    cuts = list(rng.integers(0, 3 * D, 40)) + [0, 1, 1, D // 2 + 1, 0, 3]
    cs, ce, ci = csdr_amd.psk31_debug_walk(P, "agc", "timing", x, cuts=cuts, with_extras=True)
    assert np.array_equal(cs.view(np.uint32), ws.view(np.uint32)) and np.array_equal(ci.astype(np.int64), wi)
    assert csdr_amd.psk31_debug_walk(P, "agc", "varicode", x, cuts=cuts).tobytes() == wt


def test_debug_walk_agc_state_carried():
    import csdr_amd
    x = _sig(5000, 9)
    P = _params(rate=0.01, reference=0.7, max_gain=50.0)
    st = csdr_amd.Psk31Chan(); st.gain = 2.5
    y = csdr_amd.psk31_debug_walk(P, "agc", "agc", x, cuts=[100, 0, 1, 2000], state=st)
    want, g = pm.agc(x, 0.01, 0.7, 50.0, gain=2.5)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32)) and st.gain == g


def test_argument_errors_cpu():
    import csdr_amd
    x = np.zeros(100, np.complex64)
    for kw in [dict(decimation=6), dict(decimation=4), dict(loop_gain=1.0, max_error=2.0), dict(rate=0.0), dict(algorithm=2)]:
        with pytest.raises(csdr_amd.CsdrAmdError):
            csdr_amd.psk31_debug_walk(_params(**kw), "agc", "varicode", x)
    with pytest.raises(csdr_amd.CsdrAmdError):
        csdr_amd.psk31_debug_walk(_params(), "dbpsk", "timing", x)


def test_compat_struct_layout():
    """timing_recovery_state_t and the algorithm enum as libcsdr.h:314-336 lays them out (the drop-in header declares the same)"""
    hdr = open(os.path.join(ROOT, "include", "libcsdr_amd_compat.h")).read()
    assert "TIMING_RECOVERY_ALGORITHM_GARDNER" in hdr and "timing_recovery_state_t" in hdr
    assert C.sizeof(TRState) == 56
    offs = [getattr(TRState, f[0]).offset for f in TRState._fields_]
    assert offs == [0, 4, 8, 12, 16, 20, 24, 32, 40, 44, 48, 52]
