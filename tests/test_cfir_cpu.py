"""CPU checks of the complex-tap FIR: the float32 model (cfir_model.py) against float64 within the derived gate, other float32 orders within it, wrong
filters outside it, the reference library and its committed golden vectors within it, and the library's host side (the kernels' step functions through
csdr_amd_debug_cfir_walk, the peak design, the refusals, the drop-in symbol) against the model bit for bit."""
import ctypes as C
import os
import numpy as np
import pytest

import cfir_model as cm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def ref():
    L = cm.ref_lib()
    if L is None:
        pytest.skip("reference library not built (oracle/_ref/libcsdr_ref.so)")
    return L


def _bits(y):
    return np.ascontiguousarray(y, np.complex64).view(np.uint32)


# ---------------------------------------------------------------- the model and its gate
@pytest.mark.parametrize("T", [1, 2, 7, 101, 257])
def test_model_and_other_orders_within_gate(T):
    """cfir32, a sequential sum without fma and a pairwise sum are all within the gate of cfir64"""
    x = cm.signal(1500, T)
    h = cm.random_taps(T, 50 + T)
    y64, g = cm.cfir64(x, h), cm.cfir_gate(x, h)
    assert y64.size == 1500 - T + 1
    assert cm.within(cm.cfir32(x, h), y64, g)
    assert cm.within(cm.cfir32_other(x, h), y64, g)
    assert cm.within(cm.cfir32_other(x, h, pairwise=True), y64, g)


@pytest.mark.parametrize("T", [7, 101])
def test_gate_rejects_wrong_filters(T):
    """conjugated, reversed, re/im-swapped taps, a dropped last tap and a one-sample shift leave at least 90 % of outputs outside the gate; the
    correct filter none"""
    import csdr_amd
    x = cm.signal(4096, 3)
    h = csdr_amd.firdes_peaks_c(T, [0.1, -0.23])
    y64, g = cm.cfir64(x, h), cm.cfir_gate(x, h)
    assert cm.outside(cm.cfir32(x, h), y64, g) == 0.0
    dropped = h.copy(); dropped[-1] = 0
    bad = {
        "conjugated": cm.cfir32(x, np.conj(h)),
        "reversed": cm.cfir32(x, h[::-1].copy()),
        "re/im swapped": cm.cfir32(x, (h.imag + 1j * h.real).astype(np.complex64)),
        "dropped last tap": cm.cfir32(x, dropped),
        "shifted": np.concatenate([cm.cfir32(x, h)[1:], [0]]),
    }
    for name, y in bad.items():
        assert cm.outside(y, y64, g) >= 0.9, (name, cm.outside(y, y64, g))


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("T", [7, 31, 101])
def test_reference_within_gate(ref, T):
    """the reference's apply_fir_cc (-ffast-math, per-tap complex products) is within the gate of float64"""
    x = cm.signal(3000, 20 + T)
    h = cm.random_taps(T, T)
    y = cm.ref_apply(ref, x, h)
    assert cm.within(y, cm.cfir64(x, h), cm.cfir_gate(x, h))
    assert ref.apply_fir_cc(cm._p(x), cm._p(np.zeros(8, np.complex64)), T - 1, cm._p(h), T) == 0


def test_firdes_peaks_c_matches_reference(ref):
    """the peaks_fir_cc taps for 1, 2 and 3 peaks within a few ulp (or 1e-6 of the largest tap) of the reference's firdes_add_peak_c sequence"""
    import csdr_amd
    for T, rates in [(101, [0.1]), (31, [0.1, -0.2]), (101, [0.05, -0.23, 0.31]), (7, [-0.4, 0.25]), (256, [0.0013, 0.2, -0.2])]:
        want = cm.ref_peaks(ref, T, rates)
        got = csdr_amd.firdes_peaks_c(T, rates)
        d = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        scale = np.abs(want.view(np.float32)).max()
        assert np.all((d <= 64) | (np.abs(got.view(np.float32) - want.view(np.float32)) <= 1e-6 * scale)), (T, rates, d.max())


def _golden():
    z = np.load(cm.GOLDEN)
    return [(z["x%d" % k], z["h%d" % k], z["y%d" % k], z["rates%d" % k]) for k in range(3)]


def test_golden_vectors_pin_model():
    """the committed reference outputs (three small cases): data only, small, and the model within the gate of them"""
    assert os.path.getsize(cm.GOLDEN) < 64 * 1024
    import csdr_amd
    for x, h, y, rates in _golden():
        assert y.size == x.size - h.size + 1 and y.dtype == np.complex64
        g = cm.cfir_gate(x, h)
        y32 = cm.cfir32(x, h)
        # both are within the gate of float64, so within two gates of each other; the model against float64 is the sharper statement
        assert cm.within(y32, cm.cfir64(x, h), g) and cm.within(y, cm.cfir64(x, h), g)
        assert cm.within(y32, y.astype(np.complex128), (2 * g[0], 2 * g[1]))
        mine = csdr_amd.firdes_peaks_c(h.size, rates)
        assert np.allclose(mine, h, rtol=0, atol=1e-6 * np.abs(h.view(np.float32)).max())


def test_golden_vectors_are_the_reference(ref):
    """where the reference exists, the committed vectors are what it gives"""
    for x, h, y, rates in _golden():
        assert np.array_equal(_bits(cm.ref_peaks(ref, h.size, list(rates))), _bits(h))
        assert np.array_equal(_bits(cm.ref_apply(ref, x, h)), _bits(y))


# ---------------------------------------------------------------- the library's host side
@pytest.mark.parametrize("T", [1, 2, 7, 101, 256, 257])
def test_debug_walk_equals_model_any_cuts(T):
    """csdr_amd_debug_cfir_walk equals cfir32 bit for bit, whatever the cuts"""
    import csdr_amd
    n = 3000
    x = cm.signal(n, 70 + T)
    h = cm.random_taps(T, 7 * T)
    want = cm.cfir32(x, h)
    assert want.size == n - T + 1
    for cuts in ([], [1, 1, 1], [T - 2, 1, 1], [0, 5, 0, 700]):
        got = csdr_amd.cfir_debug_walk(h, x, cuts)
        assert np.array_equal(_bits(got), _bits(want)), (T, cuts)


def test_debug_walk_short_stream():
    """a stream shorter than the filter gives nothing; outputs begin once enough has arrived"""
    import csdr_amd
    T = 31
    x = cm.signal(200, 5)
    h = cm.random_taps(T, 6)
    assert csdr_amd.cfir_debug_walk(h, x[:T - 1]).size == 0
    assert csdr_amd.cfir_debug_walk(h, x[:T - 1], [10, 10]).size == 0
    assert np.array_equal(_bits(csdr_amd.cfir_debug_walk(h, x[:T], [10, 10, 10])), _bits(cm.cfir32(x[:T], h)))
    assert np.array_equal(_bits(csdr_amd.cfir_debug_walk(h, x, [T - 1, 1, 1])), _bits(cm.cfir32(x, h)))


def test_refusals_cpu():
    """the refusals that need no device, with their messages"""
    import csdr_amd
    L = csdr_amd.lib()
    x = np.zeros(16, np.complex64); out = np.zeros(32, np.complex64); h = np.ones(4, np.complex64)

    def err():
        return L.csdr_amd_last_error().decode()
    assert L.csdr_amd_debug_cfir_walk(cm._p(h), 0, cm._p(x), 16, None, 0, cm._p(out)) < 0 and "taps_length should be 1 .. 65536" in err()
    assert L.csdr_amd_debug_cfir_walk(cm._p(h), 65537, cm._p(x), 16, None, 0, cm._p(out)) < 0 and "taps_length should be 1 .. 65536" in err()
    assert L.csdr_amd_debug_cfir_walk(None, 4, cm._p(x), 16, None, 0, cm._p(out)) < 0 and "null taps" in err()
    assert L.csdr_amd_debug_cfir_walk(cm._p(h), 4, None, 16, None, 0, cm._p(out)) < 0 and "bad arguments" in err()
    with pytest.raises(csdr_amd.CsdrAmdError):
        csdr_amd.cfir_debug_walk(np.zeros(0, np.complex64), x)
    with pytest.raises(ValueError):
        csdr_amd.firdes_peaks_c(11, [])
    # the object and the stateless call refuse a null context before anything else
    assert not L.csdr_amd_cfir_create(None, 1, 11) and "null context" in err()
    assert L.csdr_amd_apply_fir_cc(None, None, None, 1, 0, 0, 0, None, 0, 1, 0) < 0 and "null context" in err()
    for fn, args in (("set_taps", (0, None)), ("set_peaks", (0, None, 1, 2)), ("reset", ()), ("force_generic", (1,))):
        assert getattr(L, "csdr_amd_cfir_" + fn)(None, *args) < 0 and "null object" in err(), fn
    assert L.csdr_amd_cfir_reset_channel(None, 0) < 0 and "channel out of range" in err()      # (the bank base's one check of object and channel)
    assert L.csdr_amd_cfir_process(None, None, 0, 0, None, 0, None) < 0 and "null object" in err()
    assert L.csdr_amd_cfir_max_out(None, 100) == 0 and L.csdr_amd_cfir_kernel_name(None) == b""


def test_dropin_symbol_exported_and_declared():
    """apply_fir_cc is exported by the library and declared in the drop-in header with the reference's signature"""
    import csdr_amd
    A = C.CDLL(csdr_amd.lib()._name)
    assert hasattr(A, "apply_fir_cc")
    hdr = open(os.path.join(ROOT, "include", "libcsdr_amd_compat.h")).read()
    assert "int apply_fir_cc(complexf *input, complexf *output, int input_size, complexf *taps, int taps_length);" in hdr
    pub = open(os.path.join(ROOT, "include", "csdr_amd.h")).read()
    for name in ("csdr_amd_apply_fir_cc", "csdr_amd_apply_fir_last_kernel", "csdr_amd_cfir_create", "csdr_amd_cfir_set_taps", "csdr_amd_cfir_set_peaks",
                 "csdr_amd_cfir_process", "csdr_amd_cfir_max_out", "csdr_amd_cfir_reset", "csdr_amd_cfir_reset_channel", "csdr_amd_cfir_force_generic",
                 "csdr_amd_cfir_kernel_name", "csdr_amd_cfir_destroy", "csdr_amd_debug_cfir_walk", "csdr_amd_firdes_peaks_c"):
        assert name in pub and hasattr(csdr_amd.lib(), name), name
    # a stream shorter than the filter returns 0 without touching a device
    x = np.zeros(4, np.complex64); h = np.ones(8, np.complex64)
    A.apply_fir_cc.restype = C.c_int
    A.apply_fir_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    assert A.apply_fir_cc(cm._p(x), cm._p(x), 4, cm._p(h), 8) == 0
