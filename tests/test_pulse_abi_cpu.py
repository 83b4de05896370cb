"""The pulse-shaped symbol modem at the boundary: libcsdr_amd.so exports the new drop-in symbols and csdr_amd_ entry points, the drop-in header declares
them with the reference's prototypes (a translation unit that assigns each one to a function pointer of the reference's type compiles without a
diagnostic), and a client that calls every one of them links against the library alone."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DROPIN = ["firdes_rrc_f", "firdes_cosine_f", "matched_filter_get_type_from_string", "apply_real_fir_cc", "plain_interpolate_cc", "generic_slicer_f_u8",
          "pack_bits_1to8_u8_u8", "pack_bits_8to1_u8_u8"]
DEVICE = ["csdr_amd_pulsetx_create", "csdr_amd_pulsetx_process", "csdr_amd_pulsetx_max_out", "csdr_amd_pulsetx_reset", "csdr_amd_pulsetx_force_generic",
          "csdr_amd_pulsetx_kernel_name", "csdr_amd_pulsetx_tile", "csdr_amd_pulsetx_destroy", "csdr_amd_debug_pulsetx_walk", "csdr_amd_generic_slicer_f_u8",
          "csdr_amd_plain_interpolate_cc", "csdr_amd_pack_bits_1to8_u8_u8", "csdr_amd_pack_bits_8to1_u8_u8", "csdr_amd_apply_real_fir_cc", "csdr_amd_firdes_rrc_f",
          "csdr_amd_firdes_cosine_f"]

# the reference's prototypes (libcsdr.h:393-410), as function pointer types, initialised from what the header under test declares
PROTOTYPES = r'''
int (*p1)(float *, int, int) = firdes_cosine_f;
int (*p2)(float *, int, int, float) = firdes_rrc_f;
matched_filter_type_t (*p3)(char *) = matched_filter_get_type_from_string;
int (*p4)(complexf *, complexf *, int, float *, int) = apply_real_fir_cc;
void (*p5)(float *, unsigned char *, int, int) = generic_slicer_f_u8;
void (*p6)(complexf *, complexf *, int, int) = plain_interpolate_cc;
void (*p7)(unsigned char *, unsigned char *, int) = pack_bits_1to8_u8_u8;
unsigned char (*p8)(unsigned char *) = pack_bits_8to1_u8_u8;
int main(void) { matched_filter_type_t d = MATCHED_FILTER_DEFAULT; return (d == MATCHED_FILTER_RRC && MATCHED_FILTER_COSINE == 1 && p1 && p2 && p3 && p4 && p5 && p6 && p7 && p8) ? 0 : 1; }
'''


@pytest.fixture(scope="module")
def libpath():
    import csdr_amd
    if not os.path.exists(csdr_amd.LIB_PATH):
        csdr_amd.build()
    return csdr_amd.LIB_PATH


def test_new_symbols_are_exported(libpath):
    out = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    missing = sorted(set(DROPIN + DEVICE) - exported)
    assert not missing, missing


def test_headers_declare_them():
    for header, names in (("libcsdr_amd_compat.h", DROPIN), ("csdr_amd.h", DEVICE)):
        txt = open(os.path.join(ROOT, "include", header)).read()
        for n in names:
            assert n + "(" in txt, (header, n)


@pytest.mark.parametrize("header", ["libcsdr_amd_compat.h", "libcsdr.h"])
def test_prototypes_and_link(libpath, tmp_path, header):
    """against the drop-in header, and (where the reference's sources are present) against the reference's own header: the same client, linked against
    the library alone"""
    inc = ["-I", os.path.join(ROOT, "include")]
    if header == "libcsdr.h":
        ref = "/root/reference"
        if not os.path.exists(os.path.join(ref, header)):
            pytest.skip("reference headers not present on this host")
        inc = ["-DUSE_FFTW", "-DLIBCSDR_GPL", "-I", ref, "-I", os.path.join(ROOT, "oracle")]
    src = tmp_path / "c.c"
    src.write_text('#include "%s"\n%s' % (header, PROTOTYPES))
    exe = str(tmp_path / "c")
    r = subprocess.run(["gcc", "-std=gnu99", "-Wall", "-Werror", "-Wno-unused-variable"] + inc + [str(src), "-L", os.path.dirname(libpath), "-l:libcsdr_amd.so",
                        "-Wl,-rpath," + os.path.dirname(libpath), "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
