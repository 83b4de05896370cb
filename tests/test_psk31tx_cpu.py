"""CPU checks of the BPSK31 transmit chain: the float32 model (psk31tx_model.py) against the reference library stage by stage and as a chain, the
library's host tables against both, and the kernel's step functions (csdr_amd_debug_psk31tx_walk) against the model for every stage range and cut."""
import ctypes as C
import os
import numpy as np
import pytest

import psk31tx_model as tm
import psk31_model as pm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")
INTERPOLATIONS = [256, 16, 5, 1]
# every byte 0..255 (the ones without a varicode are skipped) and some plain text
TEXT = bytes(range(256)) + b"CQ CQ de MI355X pse k " + bytes(range(255, -1, -1))


class Cf(C.Structure):
    _fields_ = [("i", C.c_float), ("q", C.c_float)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def bind_tx(L):
    """the five transmit functions with the reference's prototypes (libcsdr.h:343-347), on the reference library or on the drop-in"""
    L.psk31_varicode_encoder_u8_u8.restype = None
    L.psk31_varicode_encoder_u8_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.differential_codec.restype = C.c_ubyte
    L.differential_codec.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_ubyte]
    L.psk_modulator_u8_c.restype = None
    L.psk_modulator_u8_c.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.duplicate_samples_ntimes_u8_u8.restype = None
    L.duplicate_samples_ntimes_u8_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.psk31_interpolate_sine_cc.restype = Cf
    L.psk31_interpolate_sine_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, Cf]
    return L


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built (oracle/_ref/libcsdr_ref.so)")
    return bind_tx(C.CDLL(REF_LIB))


# ------------------------------------------------------------------ wrappers (shared with the GPU tests)
def ref_varicode(L, text, room=None):
    x = np.frombuffer(bytes(text), np.uint8).copy()
    room = 12 * x.size if room is None else room
    out = np.zeros(room + 16, np.uint8)
    done, n = C.c_int(0), C.c_int(0)
    L.psk31_varicode_encoder_u8_u8(_p(x), _p(out), x.size, room, C.byref(done), C.byref(n))
    return out[:n.value].copy(), done.value


def ref_codec(L, x, encode, state=0):
    x = np.ascontiguousarray(x, np.uint8)
    out = np.zeros(max(x.size, 1), np.uint8)
    st = L.differential_codec(_p(x), _p(out), x.size, encode, state)
    return out[:x.size], st


def ref_modulate(L, idx, n_psk):
    idx = np.ascontiguousarray(idx, np.uint8)
    out = np.zeros(max(idx.size, 1), np.complex64)
    L.psk_modulator_u8_c(_p(idx), _p(out), idx.size, n_psk)
    return out[:idx.size]


def ref_shape(L, sym, interpolation, last=0j):
    sym = np.ascontiguousarray(sym, np.complex64)
    out = np.zeros(max(sym.size * interpolation, 1), np.complex64)
    r = L.psk31_interpolate_sine_cc(_p(sym), _p(out), sym.size, interpolation, Cf(np.float32(np.real(last)), np.float32(np.imag(last))))
    return out[:sym.size * interpolation], np.complex64(complex(r.i, r.q))


def ref_duplicate(L, x, sample_size, ntimes):
    x = np.ascontiguousarray(x, np.uint8)
    out = np.zeros(max(x.size * ntimes, 1), np.uint8)
    L.duplicate_samples_ntimes_u8_u8(_p(x), _p(out), x.size, sample_size, ntimes)
    return out[:x.size * ntimes]


def bits_eq(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    if a.dtype == np.complex64:
        return b.dtype == np.complex64 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return a.dtype == b.dtype and np.array_equal(a, b)


# ------------------------------------------------------------------ the model against the reference
def test_model_constants():
    t = tm.symbol_table(2)
    assert t[0] == 1 + 0j
    assert t[1].real == -1 and t[1].imag == np.float32(-8.742278e-8) and t[1].imag != 0
    for I in INTERPOLATIONS:
        assert tm.rate_table(I)[-1] == 1.0                     # the last sample of a symbol is the symbol itself
    assert tm.varicode_encode(b"\x80\xff").size == 0
    assert tm.varicode_encode(b" e").tolist() == [1, 0, 0, 1, 1, 0, 0]


def test_byte_stages_model_vs_ref(ref):
    bits, done = ref_varicode(ref, TEXT)
    assert done == len(TEXT) and np.array_equal(bits, tm.varicode_encode(TEXT))
    for state in (0, 1):
        want, st = ref_codec(ref, bits, 1, state)
        got, gs = tm.differential_encode(bits, state)
        assert np.array_equal(got, want) and gs == st
    rng = np.random.default_rng(5)
    x = rng.integers(0, 3, 500).astype(np.uint8)
    for state in (0, 1, 2):
        want, st = ref_codec(ref, x, 0, state)
        got, gs = tm.differential_decode(x, state)
        assert np.array_equal(got, want) and gs == st
    y = rng.integers(0, 256, 120).astype(np.uint8)
    for ss in (1, 3, 8):
        for nt in (1, 5):
            assert np.array_equal(tm.duplicate_samples(y, ss, nt), ref_duplicate(ref, y, ss, nt)), (ss, nt)


def _table_vs_ref(ref, n_psk):
    want = ref_modulate(ref, np.arange(256), n_psk)
    got = tm.symbol_table(n_psk)
    d = np.abs(got.view(np.float32).astype(np.float64) - want.view(np.float32).astype(np.float64)).max()
    differ = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(256, 2).any(axis=1))[0]
    print("n_psk = %d: max |model - reference| over the 256 table entries = %g, entries that differ: %s" % (n_psk, d, differ.tolist()))
    return got, want, d


def test_symbol_table_bpsk_vs_ref(ref):
    """n_psk = 2: the two symbols of the alphabet are the reference's to the bit, 1 + 0j and -1 - 8.742278e-8j.  The compiled reference (-ffast-math)
    evaluates the float phase with the float sine: of the 254 entries outside the alphabet (bytes 2..255, which the differential encoder never
    produces) one, byte 37, differs from the double evaluation in the last bit of its imaginary part (measured: 1.14e-13 absolute)."""
    got, want, d = _table_vs_ref(ref, 2)
    assert bits_eq(got[:2], want[:2])
    assert bits_eq(want[:2], np.array([1 + 0j, complex(-1, np.float32(-8.742278e-8))], np.complex64))
    assert d <= 2.0 ** -23


@pytest.mark.parametrize("n_psk", [4, 8, 3])
def test_symbol_table_other_n_psk_vs_ref(ref, n_psk):
    """The reference's -ffast-math build takes the float cosine and sine.  Measured against the compiled reference over all 256 entries: the maximum
    absolute difference is 5.96e-8 = 2^-24 for n_psk = 8 and 3 and 1.14e-13 for n_psk = 4 (10, 9 and 2 entries differ in a last bit), within the
    2^-23 held here; the n_psk entries of the alphabet itself are bit-equal for all three, and that is held too."""
    got, want, d = _table_vs_ref(ref, n_psk)
    assert d <= 2.0 ** -23
    assert bits_eq(got[:n_psk], want[:n_psk])


@pytest.mark.parametrize("I", INTERPOLATIONS)
def test_rate_table_vs_ref(ref, I):
    # the shaper on the symbol 1 + 0j from last_input 0: the output's real part is rate[j] * 1 + 0 * (1 - rate[j]) = rate[j]
    out, _ = ref_shape(ref, np.array([1 + 0j], np.complex64), I)
    assert np.array_equal(out.real.view(np.uint32), tm.rate_table(I).view(np.uint32))


@pytest.mark.parametrize("I", INTERPOLATIONS)
def test_shape_and_chain_model_vs_ref(ref, I):
    text = TEXT[:300] if I == 256 else TEXT
    bits, _ = ref_varicode(ref, text)
    st, _ = ref_codec(ref, bits, 1)
    sym = ref_modulate(ref, st, 2)
    want, wl = ref_shape(ref, sym, I)
    m = tm.chain(text, 2, I)
    assert bits_eq(m["varicode"], bits) and bits_eq(m["diff"], st) and bits_eq(m["mod"], sym) and bits_eq(m["shape"], want)
    # the shaper alone, from a carried last symbol
    got, gl = tm.shape(sym[:50], I, last=sym[7])
    want, wl = ref_shape(ref, sym[:50], I, last=sym[7])
    assert bits_eq(got, want) and bits_eq(np.array([gl]), np.array([wl]))


def test_round_trip_on_the_model():
    """every I-th sample from offset I - 1 of the transmit signal is the symbol to the bit (rate[I - 1] = 1), and the receive decoder returns the text"""
    text = bytes(range(1, 128)) + b"Hello"
    for I in INTERPOLATIONS:
        m = tm.chain(text, 2, I)
        sym = m["shape"][I - 1::I]
        assert bits_eq(sym, m["mod"])
        assert pm.varicode_decode(pm.dbpsk(sym))[0] == text


# ------------------------------------------------------------------ the library's host side against the model
def test_library_tables_vs_model():
    import csdr_amd
    for n_psk in (2, 4, 8, 3, 1, 256):
        sym, _ = csdr_amd.psk31tx_tables(n_psk, 1)
        assert bits_eq(sym, tm.symbol_table(n_psk)), n_psk
    for I in INTERPOLATIONS:
        _, rate = csdr_amd.psk31tx_tables(2, I)
        assert np.array_equal(rate.view(np.uint32), tm.rate_table(I).view(np.uint32)), I
    vt = csdr_amd.psk31_varicode_table()
    assert [format(int(c), "b").zfill(int(l)) for c, l in vt] == pm.VARICODE


def _stage_input(first, m, text):
    return {"varicode": np.frombuffer(text, np.uint8), "diff": m["varicode"], "mod": m["diff"], "shape": m["mod"]}[first]


@pytest.mark.parametrize("n_psk,I", [(2, 16), (2, 5), (4, 16), (2, 1)])
def test_debug_walk_vs_model_every_range_and_cut(n_psk, I):
    import csdr_amd
    m = tm.chain(TEXT, n_psk, I)
    for f in range(4):
        for l in range(f, 4):
            x = _stage_input(tm.STAGES[f], m, TEXT)
            want, (ds, ls) = tm.run(x, tm.STAGES[f], tm.STAGES[l], n_psk, I)
            assert bits_eq(want, m[tm.STAGES[l]])
            one = csdr_amd.psk31tx_debug_walk(x, n_psk, I, f, l)
            assert bits_eq(one, want), (f, l)
            st = csdr_amd.Psk31TxChan()
            cut = csdr_amd.psk31tx_debug_walk(x, n_psk, I, f, l, cuts=[0, 1, 3, 64], state=st)
            assert bits_eq(cut, want), (f, l)
            if l >= 1 and f <= 1:
                assert st.diff_state == ds
            if l == 3:
                assert bits_eq(np.array([complex(st.last_i, st.last_q)], np.complex64), np.array([ls], np.complex64))


def test_debug_walk_carries_state():
    import csdr_amd
    st = csdr_amd.Psk31TxChan(1, 0.25, -0.5)
    got = csdr_amd.psk31tx_debug_walk(b"ab", 2, 5, "varicode", "shape", state=st)
    want, (ds, ls) = tm.run(b"ab", "varicode", "shape", 2, 5, state=(1, complex(0.25, -0.5)))
    assert bits_eq(got, want) and st.diff_state == ds and complex(st.last_i, st.last_q) == complex(ls)
    with pytest.raises(csdr_amd.CsdrAmdError):
        csdr_amd.psk31tx_debug_walk(b"a", 0, 5)
    with pytest.raises(csdr_amd.CsdrAmdError):
        csdr_amd.psk31tx_debug_walk(b"a", 2, 0)
    with pytest.raises(csdr_amd.CsdrAmdError):
        csdr_amd.psk31tx_debug_walk(b"a", 2, 4, "shape", "mod")
