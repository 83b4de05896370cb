"""CPU checks of the transmit-side modulators: the library's host run of fmmod_fc's phase step function (csdr_amd_debug_fmmod_walk) against the float32
model (txmod_model.py) bit for bit, the models against the reference library, and the new symbols and the drop-in header."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import txmod_model as tm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")

# The gate G: 4 x the largest deviation between the strict float32 model and the reference's -ffast-math build, measured on the committed inputs.
#   fmmod_fc outputs      5.96e-8 = 2^-24 on every FM case (about 1.3 % of the words: the reference build calls cosf / sinf, the model rounds the double functions)
#   fixed_amplitude_cc    1.81e-7 at amplitude 0.7 on Gaussian input of sigma 0.5 (the reference multiplies by a reciprocal square root)
# fmmod_fc's final phase and add_dcoffset_cc are bit-equal.
MEASURED = {"fmmod": 2.0 ** -24, "fixed_amplitude": 1.81e-7}
G = {k: 4 * v for k, v in MEASURED.items()}

CUTS = [[], [0, 1, 1, 0, 63, 64, 65, 1000, 0, 1, 4097], [1] * 40 + [0] * 3 + [333]]      # the cut lists of test_carrier_cpu.py


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built (oracle/_ref/libcsdr_ref.so)")
    return tm.bind(C.CDLL(REF_LIB))


# ------------------------------------------------------------------ the phase step function (CPU run) against the model, bit for bit
@pytest.mark.parametrize("case", range(len(tm.FM_CASES)))
def test_walk_vs_model(case):
    import csdr_amd
    x = tm.fm_input(case)
    want_out, want_ph, want_last = tm.fm_model(case)
    for cuts in CUTS:
        ph, last = csdr_amd.fmmod_debug_walk(x, cuts=cuts)
        d = tm.words_differing(ph, want_ph)
        assert d == 0, "%s cuts %r: %d phases differ from the model" % (tm.FM_CASES[case], cuts[:4], d)
        assert last.view(np.uint32) == want_last.view(np.uint32)
    ph, last, out = csdr_amd.fmmod_debug_walk(x, want_out=True)
    assert tm.maxdev(out, want_out) <= G["fmmod"]


def test_cases_reach_the_wrap_edges():
    """the constant +-1 cases step by exactly +-PI and sit on the compared edges; the [-3, 3] case needs a second turn of a wrap loop"""
    assert np.any(tm.fm_model(3)[1] == tm.PI) and np.any(tm.fm_model(4)[1] == tm.R(0))
    assert np.all(tm.fm_model(4)[1] > -tm.PI) and np.all(tm.fm_model(3)[1] <= tm.PI)
    x = tm.fm_input(5).astype(np.float64) * float(tm.PI)
    assert np.abs(x).max() > 2 * np.pi + 1.0
    for c in range(len(tm.FM_CASES)):
        p = tm.fm_model(c)[1]
        assert np.all(p <= tm.PI) and np.all(p > -tm.PI)


def test_walk_state_carried():
    import csdr_amd
    x = tm.fm_input(1)[:3000]
    _, want_ph, want_last = tm.model_fmmod(x, 1.25)
    ph, last = csdr_amd.fmmod_debug_walk(x, cuts=[7, 0, 1], state=1.25)
    assert tm.words_differing(ph, want_ph) == 0 and last == want_last
    ph, last = csdr_amd.fmmod_debug_walk(x[:0], state=-0.5)
    assert ph.size == 0 and last == np.float32(-0.5)


# ------------------------------------------------------------------ the models against the reference library
@pytest.mark.parametrize("case", range(len(tm.FM_CASES)))
def test_model_vs_ref_fmmod(ref, case):
    x = tm.fm_input(case)
    want_out, want_ph, want_last = tm.fm_model(case)
    for calls in (None, [1024] * (x.size // 1024)):
        out, last = tm.lib_fmmod(ref, x, 0.0, calls)
        dev = tm.maxdev(out, want_out)
        print("%s model - reference: outputs %.3g (%d of %d words), final phase %r / %r"
              % (tm.FM_CASES[case], dev, tm.words_differing(out, want_out), 2 * x.size, float(last), float(want_last)))
        assert last.view(np.uint32) == want_last.view(np.uint32)
        assert dev <= G["fmmod"]


def test_model_vs_ref_add_dcoffset(ref):
    z = np.concatenate([tm.elementwise_input(4096, 1), np.array([0, 1, -1, 1e-30 + 3e38j, -1e-20j], np.complex64)])
    assert tm.words_differing(tm.lib_add_dcoffset(ref, z), tm.add_dcoffset(z)) == 0


def test_model_vs_ref_fixed_amplitude(ref):
    z = tm.elementwise_input(8192, 2, zeros=True)
    got, want = tm.lib_fixed_amplitude(ref, z, 0.7), tm.fixed_amplitude(z, 0.7)
    dev = tm.maxdev(got, want)
    print("fixed_amplitude_cc model - reference: %.3g" % dev)
    assert dev <= G["fixed_amplitude"]
    assert np.all(want[z == 0] == 0) and np.all(got[z == 0] == 0)
    assert np.abs(np.abs(want[z != 0]) - 0.7).max() < 1e-6


def test_samplerf_model_layout():
    b = tm.samplerf(np.array([0.5, -1.0], np.float32), 7)
    assert b.size == 32
    assert b[:8].view("<f8")[0] == 0.5 and b[8:12].view("<u4")[0] == 7 and b[12:16].view("<u4")[0] == 0 and b[16:24].view("<f8")[0] == -1.0


# ------------------------------------------------------------------ the symbols and the drop-in header
_NEW_SYMBOLS = ["csdr_amd_fmmod_fc", "csdr_amd_dsb_fc", "csdr_amd_add_dcoffset_cc", "csdr_amd_fixed_amplitude_cc", "csdr_amd_convert_f_samplerf",
                "csdr_amd_debug_fmmod_walk", "csdr_amd_txbank_create", "csdr_amd_txbank_process", "csdr_amd_txbank_set_rate", "csdr_amd_txbank_get_rate",
                "csdr_amd_txbank_reset", "csdr_amd_txbank_max_out", "csdr_amd_txbank_kernel_name", "csdr_amd_txbank_destroy",
                "fmmod_fc", "add_dcoffset_cc", "fixed_amplitude_cc"]


def test_symbols_exported():
    import csdr_amd
    out = subprocess.run(["nm", "-D", "--defined-only", csdr_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not [s for s in _NEW_SYMBOLS if s not in exported]


_CLIENT = r'''
#include "libcsdr_amd_compat.h"
/* the reference's signatures (libcsdr.h:216-218): an assignment to these pointer types fails to compile on any other */
void  (*p_dc)(complexf *, complexf *, int) = add_dcoffset_cc;
float (*p_fm)(float *, complexf *, int, float) = fmmod_fc;
void  (*p_fa)(complexf *, complexf *, int, float) = fixed_amplitude_cc;
int main(void)
{
    float x[4] = {0.1f, 0.2f, 0.3f, 0.4f}; complexf y[4], z[4];
    if (!p_dc || !p_fm || !p_fa) return 1;
    if (x[0] > 1) { float p = fmmod_fc(x, y, 4, 0.f); add_dcoffset_cc(y, z, 4); fixed_amplitude_cc(z, y, 4, p); }
    return 0;
}'''


def test_dropin_header_compiles_and_links_a_client(tmp_path):
    import csdr_amd
    src = tmp_path / "client.c"
    src.write_text(_CLIENT)
    exe = str(tmp_path / "client")
    libdir = os.path.dirname(csdr_amd.LIB_PATH)
    r = subprocess.run(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", libdir, "-lcsdr_amd",
                        "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe]).returncode == 0
