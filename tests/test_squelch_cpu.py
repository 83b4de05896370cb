"""CPU checks of the squelch and S-meter (no GPU): the library's power step function (csdr_amd_debug_squelch_power: the source the kernels run), the model
and the reference library against the float64 power within the derived gate (squelch_model.py), the gate's power to reject wrong formulas, the block stream
with level changes against the reference's get_power_c, the report schedule against a literal replay of the reference's counter, the drop-in prototypes
and parameter errors."""
import ctypes as C
import os
import re
import numpy as np
import pytest

import squelch_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = [64, 1000, 1024, 4096, 16384]


def DS(B):
    return [1, 3, 16, 1000, B + 5]


@pytest.fixture(scope="module")
def ref():
    L = sm.ref_lib()
    if L is None:
        pytest.skip("reference library not built")
    return L


def _inputs(B):
    """noise, a tone on a DC offset with noise 60 dB down, and a block with a 10^6 : 1 power step in its middle"""
    rng = np.random.default_rng(B)
    a = (0.3 * (rng.standard_normal(B) + 1j * rng.standard_normal(B))).astype(np.complex64)
    t = np.arange(B)
    b = (0.25 + 0.7 * np.exp(2j * np.pi * 0.013 * t) + 7e-4 * (rng.standard_normal(B) + 1j * rng.standard_normal(B))).astype(np.complex64)
    c = a.copy()
    c[B // 2:] *= 1e-3
    return [a, b, c]


@pytest.mark.parametrize("B", BS)
def test_powers_within_gate(ref, B):
    """the library's step function, the model (the same order: also bit for bit) and the reference lie within (n + 8) 2^-24 P of the float64 power"""
    import csdr_amd
    for x in _inputs(B):
        for d in DS(B):
            for v in (x, x.real.copy()):
                P = sm.power64(v, d)
                g = sm.bound(B, d, P)
                lib = csdr_amd.squelch_debug_power(v, d)
                mod = sm.power32(v, d)
                rf = sm.ref_power(ref, v, d)
                assert abs(float(rf) - P) <= g, ("reference", B, d, float(rf), P, g)
                assert abs(float(lib) - P) <= g, ("library", B, d, float(lib), P, g)
                assert abs(float(mod) - P) <= g, ("model", B, d, float(mod), P, g)
                assert lib.tobytes() == mod.tobytes(), (B, d, float(lib), float(mod))


def test_gate_rejects_wrong_formulas():
    """the divisor equal to the term count, a dropped last term and an off-by-one stride all leave the gate (unit-magnitude samples: every term is 1 / B)"""
    rng = np.random.default_rng(5)
    B = 1024
    x = np.exp(2j * np.pi * rng.uniform(0, 1, B)).astype(np.complex64)
    for d in (1, 3, 16):
        P = sm.power64(x, d)
        g = sm.bound(B, d, P)
        n = sm.n_terms(B, d)
        t = sm.terms32(x)[::d].astype(np.float64)
        assert abs(t.sum() - P) <= g
        if d > 1:
            assert abs(t.sum() * B / n - P) > g                          # divided by the number of terms
        assert abs(t[:-1].sum() - P) > g                                 # the last term dropped
        assert abs(sm.terms32(x)[::d + 1].astype(np.float64).sum() - P) > g    # stride d + 1


@pytest.mark.parametrize("B,d", [(1024, 1), (1000, 3), (4096, 16)])
def test_stream_vs_reference_two_classes(ref, B, d):
    """model and library decisions equal the reference's on blocks 6 dB apart around the level (none undecidable), with level changes that apply from
    the next block, level 0 (always open) among them; closed blocks are +0.0"""
    import csdr_amd
    rng = np.random.default_rng(B + d)
    nb = 48
    level = 1e-3 / d                                                     # (d > 1 takes 1 / d of the terms)
    x, _ = sm.two_class(rng, nb, B, 1e-3)
    changes = {9: level * 0.05, 17: 0.0, 25: level * 40, 33: level}
    ro, rp, rf = sm.ref_stream(ref, x, B, d, level, changes)
    lv = level
    for k in range(nb):                                                  # the reference alone: nothing undecidable on these vectors
        assert not sm.undecidable(B, d, sm.power64(x[k * B:(k + 1) * B], d), lv), k
        lv = changes.get(k, lv)
    mo, mp, mf = sm.stream(x, B, d, level, changes)
    lo, lp, lf = sm.stream(x, B, d, level, changes, power=lambda b, dd: csdr_amd.squelch_debug_power(b, dd))
    assert np.array_equal(mf, rf) and np.array_equal(lf, rf)
    assert mo.tobytes() == ro.tobytes() == lo.tobytes()
    assert 0 < rf.sum() < nb
    # the changes took effect one block late: everything passes under level 0, nothing under 40 x level
    assert rf[18:26].all() and not rf[26:34].any()
    closed = ro.reshape(nb, B)[rf == 0]
    assert closed.size and not closed.view(np.uint8).any()               # +0.0: all-zero bytes
    lv = level
    for k in range(nb):
        assert bool(lf[k]) == csdr_amd.squelch_gate_open(lp[k], lv) == sm.gate_open(lp[k], lv)
        lv = changes.get(k, lv)
    assert csdr_amd.squelch_gate_open(float("nan"), 0.0) and not csdr_amd.squelch_gate_open(float("nan"), 1e-9)
    assert csdr_amd.squelch_gate_open(float("inf"), 3.0)


@pytest.mark.parametrize("B,spread", [(1024, 0.01), (16384, 0.10)])
def test_stream_vs_reference_near_threshold(ref, B, spread):
    """powers uniform over level (1 +- spread): the decisions differ from the reference's only on undecidable blocks (|P - level| within the gate),
    expected share at most 1 %, cap 5 %"""
    import csdr_amd
    rng = np.random.default_rng(B)
    nb = 600 if B == 1024 else 200
    level = 1e-3
    x = sm.near_threshold(rng, nb, B, level, spread)
    P = np.array([sm.power64(x[k * B:(k + 1) * B]) for k in range(nb)])
    und = np.array([sm.undecidable(B, 1, p, level) for p in P])
    assert und.sum() <= 0.05 * nb
    _, rp, rf = sm.ref_stream(ref, x, B, 1, level)
    assert np.all(np.abs(rp.astype(np.float64) - P) <= [sm.bound(B, 1, p) for p in P])
    assert np.array_equal(rf[~und], (P >= level)[~und])                  # the reference alone, first
    _, mp, mf = sm.stream(x, B, 1, level)
    _, lp, lf = sm.stream(x, B, 1, level, power=lambda b, dd: csdr_amd.squelch_debug_power(b, dd))
    for pw, fl in ((mp, mf), (lp, lf)):
        assert np.all(np.abs(pw.astype(np.float64) - P) <= [sm.bound(B, 1, p) for p in P])
        assert np.array_equal(fl[~und], rf[~und])
    assert lp.tobytes() == mp.tobytes()
    assert 0.3 * nb < rf.sum() < 0.7 * nb


@pytest.mark.parametrize("every", [1, 2, 7, 100])
def test_report_schedule(every):
    """model and library against the literal replay of `if (report_cntr++ > report_every_nth)` over 1000 blocks"""
    import csdr_amd
    due = set(sm.report_replay(every, 1000))
    assert due and min(due) == every + 1
    for k in range(1000):
        assert sm.report_due(every, k) == (k in due) == csdr_amd.squelch_report_due(every, k), (every, k)
    assert not csdr_amd.squelch_report_due(every, -1)


def test_compat_header_prototypes():
    """get_power_c / get_power_f in the drop-in header with the reference's prototypes (libcsdr.h)"""
    txt = open(os.path.join(ROOT, "include", "libcsdr_amd_compat.h")).read()
    txt = re.sub(r"\s+", " ", txt)
    assert re.search(r"float get_power_f\( ?float ?\* ?\w+, int \w+, int \w+ ?\);", txt)
    assert re.search(r"float get_power_c\( ?complexf ?\* ?\w+, int \w+, int \w+ ?\);", txt)


def test_parameter_errors():
    """negative codes (NULL from create) with the reason in csdr_amd_last_error(); no device is touched"""
    import csdr_amd
    L = csdr_amd.lib()
    x = np.zeros(16, np.float32)
    p = x.ctypes.data_as(C.c_void_p)
    assert L.csdr_amd_debug_squelch_power(p, 0, 1, 1) < 0 and "block_size" in L.csdr_amd_last_error().decode()
    assert L.csdr_amd_debug_squelch_power(p, 8, 0, 1) < 0
    assert L.csdr_amd_debug_squelch_power(None, 8, 1, 0) < 0
    assert not L.csdr_amd_squelch_create(None, 1, 1024, 1, None, 65536)
    assert L.csdr_amd_get_power_c(None, p, 1, 1, 8, 1, 8, p) < 0
    assert L.csdr_amd_get_power_f(None, p, 1, 1, 8, 1, 8, p) < 0
    assert L.csdr_amd_squelch_process(None, p, 8, 8, p, 8, None, 0, None, None) < 0
    assert L.csdr_amd_squelch_set_level(None, 0, 1.0) < 0 and L.csdr_amd_squelch_reset(None) < 0 and L.csdr_amd_squelch_force_generic(None, 1) < 0
    assert L.csdr_amd_squelch_block_index(None, 0) < 0
