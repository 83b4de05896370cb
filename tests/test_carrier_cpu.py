"""CPU checks of carrier recovery: the float32 model (carrier_model.py) against the library's host run of the kernels' step functions
(csdr_amd_debug_carrier_walk) bit for bit, the coefficient helpers against the reference's init functions bit for bit, the model against the reference
library within the gate G, and the drop-in structs against the reference header's layout."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import carrier_model as cm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")
REF_HEADER_DIR = "/root/reference"

# The gate G per output: 4 x the largest deviation between the strict float32 model and the reference's -ffast-math build, measured on the committed inputs
# (carrier_model.COSTAS_CASES / PLL_CASES, 8192 samples each).  Measured: Costas out 1.84e-5, error 3.11e-5, dphase 2.64e-5, nco 3.37e-5 (all four in the
# plain loop at 10 dB, where noise makes the loop amplify a last-bit difference; the 20 and 30 dB cases stay below 1.8e-6); PLL dphase 0, nco 2^-24 = 5.96e-8 (one
# float ulp of a value in [0.5, 1)).  The factor 4 covers fast-math reorderings that vary with the compiler.
MEASURED = {("costas", "out"): 1.84e-5, ("costas", "error"): 3.11e-5, ("costas", "dphase"): 2.64e-5, ("costas", "nco"): 3.37e-5,
            ("pll", "dphase"): 0.0, ("pll", "nco"): 2.0 ** -24}
G = {k: 4 * v for k, v in MEASURED.items()}

CUTS = [[], [0, 1, 1, 0, 63, 64, 65, 1000, 0, 1, 4097], [1] * 40 + [0] * 3 + [333]]


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built (oracle/_ref/libcsdr_ref.so)")
    return cm.bind(C.CDLL(REF_LIB))


def _params(mode, alpha, beta, dphase_max):
    import csdr_amd
    return csdr_amd.CarrierParams(mode, alpha, beta, dphase_max, 0)


def _bits_equal(got, want, what):
    for k in want:
        d = cm.words_differing(got[k], want[k])
        assert d == 0, "%s: %s differs from the model in %d words, largest deviation %.3g" % (what, k, d, cm.maxdev(got[k], want[k]))


# ------------------------------------------------------------------ the kernels' step functions (CPU run) against the model, bit for bit
@pytest.mark.parametrize("case", range(len(cm.COSTAS_CASES)))
def test_walk_vs_model_costas(case):
    import csdr_amd
    P = _params(*cm.costas_mode_coefficients(case))
    want, wst = cm.model_costas(case)
    x = cm.costas_input(case)
    for cuts in CUTS:
        st = csdr_amd.CarrierChan()
        got = csdr_amd.carrier_debug_walk(P, x, cuts=cuts, state=st)
        _bits_equal(got, want, "costas case %d cuts %r" % (case, cuts[:4]))
        assert (st.phase, st.dphase, st.freq) == wst
    # a subset of the outputs is the same values
    got = csdr_amd.carrier_debug_walk(P, x, outputs=("dphase",))
    assert list(got) == ["dphase"] and cm.words_differing(got["dphase"], want["dphase"]) == 0


@pytest.mark.parametrize("case", range(len(cm.PLL_CASES)))
def test_walk_vs_model_pll(case):
    import csdr_amd
    P = _params(*cm.pll_mode_coefficients(case))
    want, wst = cm.model_pll(case)
    x = cm.pll_input(case)
    for cuts in CUTS:
        st = csdr_amd.CarrierChan()
        got = csdr_amd.carrier_debug_walk(P, x, outputs=("dphase", "nco"), cuts=cuts, state=st)
        _bits_equal(got, want, "pll case %d cuts %r" % (case, cuts[:4]))
        assert (st.phase, st.dphase, st.freq) == wst


def test_walk_state_carried_and_reset_to_zero():
    """a state handed in is where the walk starts; dphase_max_reset_to_zero sends a clamped dphase to 0"""
    import csdr_amd
    mode, a, b, dm = cm.costas_mode_coefficients(3)
    x = cm.costas_input(3)[:3000]
    start = (1.25, -0.01, 0.02)
    want, wst = cm.costas(x, a, b, dm, False, False, start)
    st = csdr_amd.CarrierChan(*start)
    got = csdr_amd.carrier_debug_walk(_params(mode, a, b, dm), x, cuts=[7, 0, 1], state=st)
    _bits_equal(got, want, "carried state")
    assert (st.phase, st.dphase, st.freq) == wst
    want, _ = cm.costas(x, a, b, cm.R(0.01), False, True)
    assert np.count_nonzero(want["dphase"] == 0) > 100               # the clamp is at work on this input
    P = _params(mode, a, b, 0.01); P.dphase_max_reset_to_zero = 1
    _bits_equal(csdr_amd.carrier_debug_walk(P, x), want, "reset to zero")


def test_argument_errors_cpu():
    import csdr_amd
    x = np.zeros(16, np.complex64)
    for P in [_params(4, 0.1, 0.1, 0.1), _params(-1, 0.1, 0.1, 0.1), _params(0, float("nan"), 0.1, 0.1), _params(0, 0.1, 0.1, -1.0), _params(0, 0.1, 0.1, 1e9)]:
        with pytest.raises(csdr_amd.CsdrAmdError):
            csdr_amd.carrier_debug_walk(P, x)
    with pytest.raises(csdr_amd.CsdrAmdError):                       # the PLL modes have no `out` or `error`
        csdr_amd.carrier_debug_walk(_params(2, 0.1, 0.0, 0.0), x, outputs=("error",))
    with pytest.raises(csdr_amd.CsdrAmdError):
        csdr_amd.carrier_debug_walk(_params(0, 0.1, 0.1, 0.1), x, state=csdr_amd.CarrierChan(float("inf"), 0, 0))


# ------------------------------------------------------------------ coefficients
def test_coefficient_helpers_vs_model():
    import csdr_amd
    for bw in (0.05, 0.1, 0.01, 0.003, 0.2):
        for damping in (0.707, 0.5, 1.0):
            for dd in (0, 1):
                P = csdr_amd.costas_params(bw, damping, dd)
                assert (P.mode, P.alpha, P.beta, P.dphase_max, P.dphase_max_reset_to_zero) == (dd,) + cm.costas_coefficients(bw, damping) + (0,)
            P = csdr_amd.pll_params("PI", bandwidth=bw, damping=damping)
            assert (P.mode, P.alpha, P.beta) == (cm.PLL_PI,) + cm.pll_pi_coefficients(bw, damping=damping)
    P = csdr_amd.pll_params(1, alpha=0.01)
    assert (P.mode, P.alpha, P.beta) == (cm.PLL_P, cm.R(0.01), 0.0)


def test_coefficient_helpers_vs_ref(ref):
    """bit for bit what init_bpsk_costas_loop_cc and pll_cc_init_pi_controller store"""
    import csdr_amd
    for bw in (0.05, 0.1, 0.01, 0.003, 0.2):
        for damping in (0.707, 0.5, 1.0):
            st = cm.costas_init(ref, bw, damping, 1)
            P = csdr_amd.costas_params(bw, damping, 1)
            assert (P.alpha, P.beta, P.dphase_max) == (st.alpha, st.beta, st.dphase_max), (bw, damping)
            assert (st.current_freq, st.dphase, st.nco_phase, st.dphase_max_reset_to_zero) == (0, 0, 0, 0)
            for ko, kd in ((10.0, 0.1), (1.0, 1.0), (3.0, 0.7)):
                pst = cm.PllState(); ref.pll_cc_init_pi_controller(C.byref(pst), bw, ko, kd, damping)
                P = csdr_amd.pll_params(2, bandwidth=bw, ko=ko, kd=kd, damping=damping)
                assert (P.alpha, P.beta) == (pst.alpha, pst.beta), (bw, damping, ko, kd)


# ------------------------------------------------------------------ the model against the reference library, within G
@pytest.mark.parametrize("case", range(len(cm.COSTAS_CASES)))
def test_model_vs_ref_costas(ref, case):
    bw, damping, dd, _, _ = cm.COSTAS_CASES[case]
    want, st = cm.drive_costas(ref, cm.costas_input(case), bw, damping, dd)
    got, gst = cm.model_costas(case)
    dev = {k: cm.maxdev(got[k], want[k]) for k in want}
    print("costas case %d model - reference: %s" % (case, dev))
    for k in want:
        assert dev[k] <= G["costas", k], (k, dev[k])


@pytest.mark.parametrize("case", range(len(cm.PLL_CASES)))
def test_model_vs_ref_pll(ref, case):
    kind, coef, _, _ = cm.PLL_CASES[case]
    want, st = cm.drive_pll(ref, cm.pll_input(case), kind, coef)
    got, gst = cm.model_pll(case)
    dev = {k: cm.maxdev(got[k], want[k]) for k in want}
    print("pll case %d model - reference: %s" % (case, dev))
    for k in want:
        assert dev[k] <= G["pll", k], (k, dev[k])


def test_ref_quirks_the_dropin_keeps(ref):
    """init_bpsk_costas_loop_cc never stores decision_directed; pll_cc_init_p_controller leaves iir_temp and pll_type alone; any other pll_type advances the
    phase, writes output_nco[0] and returns"""
    st = cm.CostasState(); st.decision_directed = 77
    with cm._quiet_stderr():
        ref.init_bpsk_costas_loop_cc(C.byref(st), 0, 0.707, 0.05)
    assert st.decision_directed == 77
    p = cm.PllState(); p.pll_type = 9; p.iir_temp = 3.5
    ref.pll_cc_init_p_controller(C.byref(p), 0.25)
    assert (p.pll_type, p.iir_temp, p.alpha) == (9, 3.5, 0.25)
    p.dphase = 0.5
    x = np.ones(4, np.complex64); nco = np.full(4, 9 + 9j, np.complex64); dph = np.full(4, 9, np.float32)
    ref.pll_cc(C.byref(p), cm._p(x), cm._p(dph), cm._p(nco), 4)
    assert p.output_phase == 0.5 and np.all(nco[1:] == 9 + 9j) and np.all(dph == 9)
    assert abs(nco[0] - (np.sin(0.5) + 1j * np.cos(0.5))) < 1e-6


# ------------------------------------------------------------------ the drop-in structs
_LAYOUT_SRC = r'''
#include <stdio.h>
#include <stddef.h>
#include "%s"
int main(void){
 printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\n", sizeof(bpsk_costas_loop_state_t), offsetof(bpsk_costas_loop_state_t, alpha), offsetof(bpsk_costas_loop_state_t, beta),
   offsetof(bpsk_costas_loop_state_t, decision_directed), offsetof(bpsk_costas_loop_state_t, current_freq), offsetof(bpsk_costas_loop_state_t, dphase),
   offsetof(bpsk_costas_loop_state_t, nco_phase), offsetof(bpsk_costas_loop_state_t, dphase_max), offsetof(bpsk_costas_loop_state_t, dphase_max_reset_to_zero));
 printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%d %%d\n", sizeof(pll_t), offsetof(pll_t, pll_type), offsetof(pll_t, output_phase), offsetof(pll_t, dphase),
   offsetof(pll_t, frequency), offsetof(pll_t, alpha), offsetof(pll_t, beta), offsetof(pll_t, iir_temp), sizeof(pll_type_t), (int)PLL_P_CONTROLLER, (int)PLL_PI_CONTROLLER);
 return 0; }'''


def _layout(tmp_path, include_dir, header, name, flags=()):
    src = tmp_path / (name + ".c")
    src.write_text(_LAYOUT_SRC % header)
    exe = str(tmp_path / name)
    subprocess.run(["gcc", "-std=gnu99", *flags, "-I", include_dir, str(src), "-o", exe], check=True)
    return [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]


def test_compat_struct_layout(tmp_path):
    """bpsk_costas_loop_state_t, pll_t and pll_type_t of the drop-in header: sizes and field offsets as libcsdr.h:292-308, 364-374 lays them out (and as the
    ctypes mirrors used by these tests do); against the reference header itself where it is present"""
    ours = _layout(tmp_path, os.path.join(ROOT, "include"), "libcsdr_amd_compat.h", "ours")
    assert ours == [32, 0, 4, 8, 12, 16, 20, 24, 28, 28, 0, 4, 8, 12, 16, 20, 24, 4, 1, 2]
    assert C.sizeof(cm.CostasState) == 32 and [getattr(cm.CostasState, f[0]).offset for f in cm.CostasState._fields_] == ours[1:9]
    assert C.sizeof(cm.PllState) == 28 and [getattr(cm.PllState, f[0]).offset for f in cm.PllState._fields_] == ours[10:17]
    if os.path.exists(os.path.join(REF_HEADER_DIR, "libcsdr.h")):
        assert _layout(tmp_path, REF_HEADER_DIR, "libcsdr.h", "theirs", ["-DUSE_FFTW", "-DLIBCSDR_GPL", "-I", os.path.join(ROOT, "oracle")]) == ours
