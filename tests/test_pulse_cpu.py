"""CPU checks of the pulse-shaped symbol modem: the model (pulse_model.py) against the compiled reference (transmit stream, designs, slicer, packers,
plain_interpolate_cc), the library's host designs against both, and the transmit object's step functions (csdr_amd_debug_pulsetx_walk) against the
float32 model, bit for bit, for every shape and cut.  Measured figures: profiles/pulse_gates.md."""
import ctypes as C
import os
import numpy as np
import pytest

import pulse_model as pm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")
SHAPES = [(1, 1), (2, 5), (5, 21), (8, 65), (64, 33), (7, 7)]          # (interpolation, taps)
N_PSK = [2, 4, 8]
RRC_CASES = [(4, 33, 0.25), (8, 65, 0.5), (8, 65, 0.35), (2, 9, 0.2), (16, 129, 0.35)]   # (sps, taps, beta); the first two take the closed-form branch
COSINE_SPS = [1, 4, 25]
SLICER_N = [2, 3, 4, 8, 16, 256]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def bind_modem(L):
    """the modem's functions with the reference's prototypes (libcsdr.h:401-410), on the reference library or on the drop-in"""
    L.psk_modulator_u8_c.restype = None; L.psk_modulator_u8_c.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.firdes_cosine_f.restype = C.c_int; L.firdes_cosine_f.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.firdes_rrc_f.restype = C.c_int; L.firdes_rrc_f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float]
    L.matched_filter_get_type_from_string.restype = C.c_int; L.matched_filter_get_type_from_string.argtypes = [C.c_char_p]
    L.apply_real_fir_cc.restype = C.c_int; L.apply_real_fir_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.generic_slicer_f_u8.restype = None; L.generic_slicer_f_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.plain_interpolate_cc.restype = None; L.plain_interpolate_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.pack_bits_1to8_u8_u8.restype = None; L.pack_bits_1to8_u8_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.pack_bits_8to1_u8_u8.restype = C.c_ubyte; L.pack_bits_8to1_u8_u8.argtypes = [C.c_void_p]
    return L


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built (oracle/_ref/libcsdr_ref.so)")
    return bind_modem(C.CDLL(REF_LIB))


# ------------------------------------------------------------------ wrappers (shared with the GPU tests: L is the reference library or the drop-in)
def lib_modulate(L, idx, n_psk):
    idx = np.ascontiguousarray(idx, np.uint8)
    out = np.zeros(max(idx.size, 1), np.complex64)
    L.psk_modulator_u8_c(_p(idx), _p(out), idx.size, n_psk)
    return out[:idx.size]


def lib_interpolate(L, x, interpolation):
    x = np.ascontiguousarray(x, np.complex64)
    out = np.full(max(x.size * interpolation, 1), 7 + 7j, np.complex64)
    L.plain_interpolate_cc(_p(x), _p(out), x.size, interpolation)
    return out[:x.size * interpolation]


def lib_fir(L, x, taps):
    x = np.ascontiguousarray(x, np.complex64); taps = np.ascontiguousarray(taps, np.float32)
    out = np.zeros(max(x.size, 1), np.complex64)
    n = L.apply_real_fir_cc(_p(x), _p(out), x.size, _p(taps), taps.size)
    return out[:max(n, 0)]


def lib_rrc(L, n_taps, sps, beta, guard=1):
    t = np.full(n_taps + guard, 12345.0, np.float32)
    L.firdes_rrc_f(_p(t), n_taps, sps, beta)
    return t


def lib_cosine(L, sps):
    t = np.zeros(2 * sps + 1, np.float32)                    # (zeroed: the reference never writes the two end taps)
    L.firdes_cosine_f(_p(t), t.size, sps)
    return t


def lib_slicer(L, x, n_symbols, fill=0):
    x = np.ascontiguousarray(x, np.float32)
    out = np.full(max(x.size, 1), fill, np.uint8)
    L.generic_slicer_f_u8(_p(x), _p(out), x.size, n_symbols)
    return out[:x.size]


def lib_pack_1to8(L, x):
    x = np.ascontiguousarray(x, np.uint8)
    out = np.zeros(max(8 * x.size, 1), np.uint8)
    L.pack_bits_1to8_u8_u8(_p(x), _p(out), x.size)
    return out[:8 * x.size]


def lib_pack_8to1(L, x):
    x = np.ascontiguousarray(x, np.uint8).reshape(-1, 8)
    return np.array([L.pack_bits_8to1_u8_u8(_p(np.ascontiguousarray(r))) for r in x], np.uint8)


def bits_eq(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    if a.dtype == np.complex64:
        return b.dtype == np.complex64 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    if a.dtype == np.float32:
        return b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return a.dtype == b.dtype and np.array_equal(a, b)


def test_taps(interpolation, n_taps, seed=5):
    """asymmetric taps of both signs, so that a reversed or shifted filter shows"""
    rng = np.random.default_rng(seed + 1000 * interpolation + n_taps)
    return (rng.uniform(-1, 1, n_taps) * np.linspace(1.0, 0.25, n_taps)).astype(np.float32)


test_taps.__test__ = False


def slicer_points(n_symbols, n_random=100000, seed=3):
    """(inputs, is_threshold_point): random floats in [-1.5, 1.5], +-0, +-inf, and every limit -2 .. +2 ulp (those five per limit are the threshold points)"""
    rng = np.random.default_rng(seed + n_symbols)
    lo, hi = pm.slicer_limits(n_symbols)
    lim = np.unique(np.concatenate([lo, hi]))
    pts = [lim]
    up, dn = lim, lim
    for _ in range(2):
        up = np.nextafter(up, np.float32(np.inf)); dn = np.nextafter(dn, np.float32(-np.inf))
        pts += [up, dn]
    near = np.concatenate(pts).astype(np.float32)
    x = rng.uniform(-1.5, 1.5, n_random).astype(np.float32)
    x = x[~np.isin(x, near)]                                   # (a random float32 hits one of the 5 (n - 1) points about never)
    special = np.array([0.0, -0.0, np.inf, -np.inf], np.float32)
    special = special[~np.isin(special, near)]
    allx = np.concatenate([x, special, near]).astype(np.float32)
    flag = np.concatenate([np.zeros(x.size + special.size, bool), np.ones(near.size, bool)])
    return allx, flag


# ------------------------------------------------------------------ the model's own fused multiply-add
def test_fma32_is_one_rounding():
    """fma32 against exact rational arithmetic: operands of far apart exponents (the exact sum has more than 53 bits), and sums a hair below a float32
    midpoint whose float64 sum IS the midpoint (rounding twice would go to even, upwards)"""
    from fractions import Fraction
    rng = np.random.default_rng(11)
    a = rng.uniform(-2, 2, 3000).astype(np.float32); b = rng.uniform(-2, 2, 3000).astype(np.float32)
    c = (rng.uniform(-2, 2, 3000) * 2.0 ** rng.integers(-30, 36, 3000)).astype(np.float32)
    r = np.arange(1, 101)
    a = np.concatenate([a, (8 * (1 + 2.0 ** -23 * r)).astype(np.float32)]); b = np.concatenate([b, (8 * (1 - 2.0 ** -23 * r)).astype(np.float32)])
    c = np.concatenate([c, (2.0 ** 30 + 128.0 * (2 * rng.integers(0, 1 << 20, 100) + 1)).astype(np.float32)])
    got = pm.fma32(a, b, c)
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert np.any(twice[3000:] != got[3000:])                 # the second family does tell the two apart
    for k in range(a.size):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        near = np.float32(float(exact))
        cands = [near, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf))]
        dist = [abs(Fraction(float(v)) - exact) for v in cands]
        winners = [v for v, d in zip(cands, dist) if d == min(dist)]
        if len(winners) == 2:                                 # a tie: to even
            winners = [v for v in winners if (np.float32(v).view(np.uint32) & 1) == 0]
        assert got[k] == winners[0], (a[k], b[k], c[k])


# ------------------------------------------------------------------ the transmit stream
@pytest.mark.parametrize("n_psk", N_PSK)
@pytest.mark.parametrize("shape", SHAPES)
def test_model_stream_vs_reference(ref, shape, n_psk):
    """psk_modulator_u8_c | plain_interpolate_cc | apply_real_fir_cc of the reference: its T products are summed in another order, so the gate is the
    float32 dot-product bound T 2^-24 1.01 sum |x[i + t] taps[t]| against the float64 model; the float32 model is held to the same gate."""
    I, T = shape
    rng = np.random.default_rng(100 * I + T + n_psk)
    idx = rng.integers(0, n_psk, 300).astype(np.uint8)
    taps = test_taps(I, T)
    sym = pm.symbols(n_psk)
    c_ref = lib_modulate(ref, idx, n_psk)
    # the symbols of the alphabet: the library's table against the reference's own (a last bit at most); the stream is compared on the reference's symbols
    assert np.max(np.abs(c_ref - sym[idx])) <= 2.0 ** -23
    x_ref = lib_interpolate(ref, c_ref, I)
    assert bits_eq(x_ref, pm.stuffed(c_ref, I)[0])
    y_ref = lib_fir(ref, x_ref, taps)
    want, mr, mi = pm.shape64(c_ref, I, taps)
    assert y_ref.size == pm.n_outputs(idx.size, I, T) == want.size
    assert pm.within(y_ref, want, pm.dot_gate(T, mr), pm.dot_gate(T, mi))
    y32 = pm.shape32(c_ref, I, taps)
    assert pm.within(y32, want, pm.dot_gate(T, mr), pm.dot_gate(T, mi))


def test_model_phase_without_tap_is_zero():
    y = pm.shape32(np.array([1 + 1j, 2 - 1j, -1 + 3j], np.complex64), 7, np.array([0.5, -0.25, 2.0], np.float32))
    i = np.arange(y.size)
    ph = (-i) % 7
    assert np.all(y[ph >= 3] == 0) and np.all(y[ph < 3] != 0)
    assert bits_eq(y[ph >= 3], np.zeros(int((ph >= 3).sum()), np.complex64))       # + 0, not - 0


@pytest.mark.parametrize("n_psk", N_PSK)
@pytest.mark.parametrize("cuts", [(0, 1, 1, 3), ()])
@pytest.mark.parametrize("shape", SHAPES + [(3, 200)])
def test_debug_walk_equals_model(shape, cuts, n_psk):
    """the step functions the kernels run, on the CPU: bit-equal to the float32 model for every stage range, in calls of 0, 1, 1, 3, rest and in one call"""
    import csdr_amd
    I, T = shape
    rng = np.random.default_rng(7 * I + T + n_psk)
    idx = rng.integers(0, 256, 300).astype(np.uint8)           # every table entry, not only the alphabet
    taps = test_taps(I, T)
    sym = pm.symbols(n_psk)
    want = pm.shape32(sym[idx], I, taps)
    got = csdr_amd.pulsetx_debug_walk(idx, taps, n_psk, I, "mod", "shape", cuts)
    assert got.size == pm.n_outputs(300, I, T) and bits_eq(got, want)
    c = (rng.standard_normal(300) + 1j * rng.standard_normal(300)).astype(np.complex64)
    assert bits_eq(csdr_amd.pulsetx_debug_walk(c, taps, n_psk, I, "shape", "shape", cuts), pm.shape32(c, I, taps))
    assert bits_eq(csdr_amd.pulsetx_debug_walk(idx, None, n_psk, I, "mod", "mod", cuts), sym[idx])


def test_debug_walk_short_streams():
    """fewer symbols than the filter spans: no output until n I >= T, then exactly n I - T + 1"""
    import csdr_amd
    taps = test_taps(3, 20)
    for n in range(0, 12):
        idx = (np.arange(n) % 4).astype(np.uint8)
        got = csdr_amd.pulsetx_debug_walk(idx, taps, 4, 3, "mod", "shape", (1,) * n)
        assert got.size == pm.n_outputs(n, 3, 20) and bits_eq(got, pm.shape32(pm.symbols(4)[idx], 3, taps))


def test_debug_walk_argument_errors():
    import csdr_amd
    t = np.ones(3, np.float32); x = np.zeros(4, np.uint8)
    for kw in [dict(n_psk=0), dict(n_psk=257), dict(interpolation=0), dict(first="shape", last="mod")]:
        with pytest.raises(csdr_amd.CsdrAmdError):
            csdr_amd.pulsetx_debug_walk(x, t, **{**dict(n_psk=4, interpolation=2), **kw})
    with pytest.raises(csdr_amd.CsdrAmdError):
        csdr_amd.pulsetx_debug_walk(x, np.zeros(0, np.float32), 4, 2)


# ------------------------------------------------------------------ designs
@pytest.mark.parametrize("case", RRC_CASES)
def test_rrc_vs_reference(ref, case):
    """gate: 1e-6 x the largest tap (about sixteen float32 roundings); the model and the library against the reference, the library against the model to the bit"""
    import csdr_amd
    sps, T, beta = case
    special = pm.rrc_special_index(sps, beta)
    assert (special is not None and special <= T // 2) == (case in RRC_CASES[:2])
    for i in range(1, T // 2 + 1):                             # the reference's own formula is well conditioned away from its closed-form branch
        if i != special:
            assert abs(1 - (4 * beta * i / sps) ** 2) > 1e-3
    r = lib_rrc(ref, T, sps, beta)
    assert r[T] == np.float32(12345.0)
    m = pm.firdes_rrc(T, sps, beta)
    got = csdr_amd.firdes_rrc_f(T, sps, beta)
    gate = 1e-6 * float(np.max(np.abs(r[:T])))
    print("rrc sps %d T %d beta %g: max |model - reference| / max tap = %.3g, library - model bits equal: %s"
          % (sps, T, beta, float(np.max(np.abs(m.astype(np.float64) - r[:T]))) / float(np.max(np.abs(r[:T]))), bits_eq(got, m)))
    assert np.max(np.abs(m.astype(np.float64) - r[:T])) <= gate
    assert np.max(np.abs(got.astype(np.float64) - r[:T])) <= gate
    assert bits_eq(got, m)
    assert np.array_equal(got, got[::-1]) and abs(float(np.sum(got.astype(np.float64))) - 1) < 1e-5


@pytest.mark.parametrize("sps", COSINE_SPS)
def test_cosine_vs_reference(ref, sps):
    import csdr_amd
    r = lib_cosine(ref, sps)
    m = pm.firdes_cosine(sps)
    got = csdr_amd.firdes_cosine_f(sps)
    gate = 1e-6 * float(np.max(np.abs(r)))
    print("cosine sps %d: max |model - reference| / max tap = %.3g" % (sps, float(np.max(np.abs(m.astype(np.float64) - r))) / float(np.max(np.abs(r)))))
    assert got.size == 2 * sps + 1 and got[0] == 0 and got[-1] == 0
    assert np.max(np.abs(m.astype(np.float64) - r)) <= gate and np.max(np.abs(got.astype(np.float64) - r)) <= gate
    assert bits_eq(got, m)


def test_rrc_even_length():
    """the library form refuses an even length; the drop-in designs it as the reference does, without the reference's write to taps[T]"""
    import csdr_amd
    with pytest.raises(csdr_amd.CsdrAmdError):
        csdr_amd.firdes_rrc_f(64, 8, 0.35)
    with pytest.raises(csdr_amd.CsdrAmdError):
        csdr_amd.firdes_rrc_f(0, 8, 0.35)
    L = bind_modem(C.CDLL(csdr_amd.LIB_PATH))
    t = lib_rrc(L, 64, 8, 0.35, guard=4)
    assert np.all(t[64:] == np.float32(12345.0)) and np.all(np.isfinite(t[:64])) and np.all(t[:64] != np.float32(12345.0))
    assert bits_eq(t[:64], pm.firdes_rrc(64, 8, 0.35))
    odd = lib_rrc(L, 65, 8, 0.35)
    assert odd[65] == np.float32(12345.0) and bits_eq(odd[:65], csdr_amd.firdes_rrc_f(65, 8, 0.35))
    assert bits_eq(lib_cosine(L, 4), csdr_amd.firdes_cosine_f(4))
    assert [L.matched_filter_get_type_from_string(s) for s in (b"RRC", b"COSINE", b"cosine", b"")] == [0, 1, 0, 0]


def test_matched_filter_type_vs_reference(ref):
    import csdr_amd
    L = bind_modem(C.CDLL(csdr_amd.LIB_PATH))
    for s in (b"RRC", b"COSINE", b"GAUSS", b"rrc", b""):
        assert L.matched_filter_get_type_from_string(s) == ref.matched_filter_get_type_from_string(s)


# ------------------------------------------------------------------ slicer
@pytest.mark.parametrize("n_symbols", SLICER_N)
def test_slicer_model_vs_reference(ref, n_symbols):
    """the float32 model equals the compiled reference on every input more than 2 ulp from a limit; at the threshold points the reference's
    optimised float arithmetic may place a limit an ulp or two elsewhere (profiles/pulse_gates.md)"""
    x, near = slicer_points(n_symbols)
    assert near.sum() >= 5 * (n_symbols - 1) and (~near).sum() > 99000
    m = pm.slicer(x, n_symbols)
    r = lib_slicer(ref, x, n_symbols)
    assert np.array_equal(m[~near], r[~near])
    print("slicer n %d: %d of %d threshold points differ from the reference" % (n_symbols, int((m[near] != r[near]).sum()), int(near.sum())))
    # the model at the exact limits: a lower limit belongs to its symbol
    lo, hi = pm.slicer_limits(n_symbols)
    assert np.array_equal(pm.slicer(lo, n_symbols)[lo >= hi], np.arange(1, n_symbols, dtype=np.uint8)[lo >= hi])
    assert pm.slicer(np.array([np.nan, -np.inf, np.inf, 0.0, -0.0], np.float32), n_symbols).tolist()[:3] == [0, 0, n_symbols - 1]


def test_slicer_reference_leaves_nan_unwritten(ref):
    x = np.array([np.nan, 0.9], np.float32)
    assert lib_slicer(ref, x, 4, fill=77).tolist() == [77, 3]


# ------------------------------------------------------------------ packers and plain_interpolate_cc
def test_packers_and_interpolate_vs_reference(ref):
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(pm.pack_1to8(every), lib_pack_1to8(ref, every))
    alphabet = np.array([0, 1, 2, 255], np.uint8)
    groups = alphabet[(np.arange(256)[:, None] >> np.arange(7, -1, -1)) & 1]                     # the 256 zero / nonzero patterns ...
    groups = np.where(groups == 1, alphabet[1 + (np.arange(256)[:, None] + np.arange(8)) % 3], 0).astype(np.uint8)   # ... their nonzero bytes drawn from 1, 2, 255
    assert len({tuple(g != 0) for g in groups}) == 256 and set(np.unique(groups)) == {0, 1, 2, 255}
    assert np.array_equal(pm.pack_8to1(groups.ravel()), lib_pack_8to1(ref, groups))
    # not inverses of each other: LSB first out, MSB first in
    assert pm.pack_8to1(pm.pack_1to8(np.array([1], np.uint8)))[0] == 128
    rng = np.random.default_rng(2)
    c = (rng.standard_normal(37) + 1j * rng.standard_normal(37)).astype(np.complex64)
    for I in (1, 2, 7, 64):
        assert bits_eq(pm.stuffed(c, I)[0], lib_interpolate(ref, c, I))
