"""CPU checks of the noise sources and the AWGN channel: the host build of csdr_amd/csrc/noise_dev.hpp (the csdr_amd_debug_* entries and the drop-ins)
against the numpy model (tests/noise_model.py), the golden vectors of the reference binary and, where oracle/_ref is built, the reference itself."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import csdr_amd
import noise_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")
REF_CSDR = os.path.join(ROOT, "oracle", "_ref", "csdr")
GOLDEN = os.path.join(ROOT, "tests", "golden", "awgn_ref_vectors.npz")
INT_MAX, INT_MIN = 0x7fffffff, 0x80000000
u32, f32, c64 = np.uint32, np.float32, np.complex64


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(u32)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(csdr_amd.LIB_PATH):
        csdr_amd.build()
    return csdr_amd.lib()


@pytest.fixture(scope="module")
def reflib():
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built (oracle/_ref/libcsdr_ref.so)")
    R = C.CDLL(REF_LIB)
    R.get_random_gaussian_samples_c.restype = None; R.get_random_gaussian_samples_c.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    R.get_random_samples_f.restype = None; R.get_random_samples_f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    R.total_logpower_cf.restype = C.c_float; R.total_logpower_cf.argtypes = [C.c_void_p, C.c_int]
    R.normalized_timing_variance_u32_f.restype = C.c_float; R.normalized_timing_variance_u32_f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    return R


libc = C.CDLL(None)
libc.fopen.restype = C.c_void_p; libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
libc.fclose.argtypes = [C.c_void_p]


def from_file(fn, words, n, dtype, tmp_path):
    """fn(output, n, FILE *) of a library that reads its words from a file of `words`"""
    path = str(tmp_path / "words.bin")
    np.ascontiguousarray(words, u32).tofile(path)
    f = libc.fopen(path.encode(), b"r")
    assert f
    out = np.zeros(n, dtype)
    fn(out.ctypes.data_as(C.c_void_p), n, C.c_void_p(f))
    libc.fclose(C.c_void_p(f))
    return out


# ---------------------------------------------------------------- Philox and determinism
KATS = [([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
        ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
        ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KATS)
def test_philox_known_answers(L, ctr, key, want):
    want = [int(w, 16) for w in want.split()]
    assert list(csdr_amd.philox4x32_10(ctr, key)) == want
    assert list(nm.philox4x32_10(np.array(ctr, u32), np.array(key, u32))) == want


def test_block_layout_is_the_documented_one(L):
    """block(kind, s, j) = philox((j lo, j hi, s, kind), (seed lo, seed hi)); Gaussian sample i: words 2 (i & 1), 2 (i & 1) + 1 of block(0, s, i >> 1); uniform k:
    word k & 3 of block(1, s, k >> 2)"""
    seed, s = 0x0123456789abcdef, 77
    for i in (0, 1, 6, 7, (1 << 33) + 1):
        b = csdr_amd.philox4x32_10([(i >> 1) & 0xffffffff, (i >> 1) >> 32, s, 0], [seed & 0xffffffff, seed >> 32])
        want = csdr_amd.noise_from_words("gaussian", b[2 * (i & 1):2 * (i & 1) + 2])
        assert np.array_equal(bits(csdr_amd.noise_debug_walk("gaussian", seed, s, i, 1)), bits(want))
    for k in (0, 1, 2, 3, 4, 9, (1 << 34) + 3):
        b = csdr_amd.philox4x32_10([(k >> 2) & 0xffffffff, (k >> 2) >> 32, s, 1], [seed & 0xffffffff, seed >> 32])
        assert np.array_equal(bits(csdr_amd.noise_debug_walk("uniform", seed, s, k, 1)), bits(csdr_amd.noise_from_words("uniform", b[k & 3:(k & 3) + 1])))


@pytest.mark.parametrize("kind", ["gaussian", "uniform"])
def test_walk_does_not_depend_on_the_cuts(L, kind):
    n = 1000
    whole = csdr_amd.noise_debug_walk(kind, 5, 2, 3, n)
    for cuts in ([0], [1], [3], [0, 1, 3, 7, 0, 1], [333, 1, 1, 111], [n], [n + 5]):
        assert np.array_equal(bits(csdr_amd.noise_debug_walk(kind, 5, 2, 3, n, cuts=cuts)), bits(whole)), cuts
    x = (np.arange(n) * 0.001 + 0.5j).astype(c64)
    mixed = csdr_amd.noise_debug_walk(kind, 5, 2, 3, x=x, snr_db=3.0) if kind == "gaussian" else None
    if mixed is not None:
        for cuts in ([0], [1], [3, 5], [999]):
            assert np.array_equal(bits(csdr_amd.noise_debug_walk(kind, 5, 2, 3, x=x, snr_db=3.0, cuts=cuts)), bits(mixed)), cuts
        assert np.array_equal(bits(mixed), bits(csdr_amd.awgn_debug_mix(x, whole, 3.0)))


@pytest.mark.parametrize("kind", ["gaussian", "uniform"])
@pytest.mark.parametrize("pos", [0, 1, 2, 3, 5, (1 << 33) + 1])
def test_walk_does_not_depend_on_the_start(L, kind, pos):
    """sample i is the same whatever position the walk started from: a walk from pos against the tail of one that starts 1, 2, 3 and 5 samples earlier, and
    against the transform of the model's words for those indexes"""
    n = 70
    got = csdr_amd.noise_debug_walk(kind, 9, 4, pos, n)
    for back in (1, 2, 3, 5):
        if pos >= back:
            assert np.array_equal(bits(csdr_amd.noise_debug_walk(kind, 9, 4, pos - back, n + back)[back:]), bits(got)), back
    words = nm.gaussian_words(9, 4, pos, n) if kind == "gaussian" else nm.uniform_words(9, 4, pos, n)
    assert np.array_equal(bits(csdr_amd.noise_from_words(kind, words)), bits(got))


def test_uniform_is_bit_equal_to_the_model(L):
    for seed, s, pos in ((0, 0, 0), (7, 3, 1), (1 << 63, 0xffffffff, (1 << 33) + 1)):
        got = csdr_amd.noise_debug_walk("uniform", seed, s, pos, 4099)
        assert np.array_equal(bits(got), bits(nm.uniform(seed, s, pos, 4099)))
        assert got.min() >= -1 and got.max() <= 1
    edge = csdr_amd.noise_from_words("uniform", [INT_MAX, INT_MIN, 0, 1, 0xffffffff])
    assert np.array_equal(bits(edge), bits(np.array([1.0, -1.0, 0.0, 2.0 ** -31, -2.0 ** -31], f32)))


def test_streams_and_seeds_differ(L):
    a = csdr_amd.noise_debug_walk("gaussian", 1, 0, 0, 64)
    assert not np.array_equal(a, csdr_amd.noise_debug_walk("gaussian", 1, 1, 0, 64))
    assert not np.array_equal(a, csdr_amd.noise_debug_walk("gaussian", 2, 0, 0, 64))
    assert not np.array_equal(a, csdr_amd.noise_debug_walk("gaussian", 1 + (1 << 32), 0, 0, 64))


# ---------------------------------------------------------------- the Gaussian transform against the float64 model
def test_forced_words(L):
    """w0 = INT_MAX: u_0 == 1.0f and the sample is exactly 0; w0 = INT_MIN: u_0 = 1e-8 and |sample| = 6.0697083, the largest there is; 0: the model's value"""
    w = np.array([INT_MAX, 12345, INT_MAX, INT_MIN, INT_MIN, INT_MAX, INT_MIN, INT_MIN, INT_MIN, 0, 0, 0, 0, INT_MAX, 0, INT_MIN], u32)
    got = csdr_amd.noise_from_words("gaussian", w)
    want = nm.gaussian_from_words(w)
    assert got[0] == 0 and got[1] == 0
    # u_1 = 1.0f (INT_MAX): angle 2 pi, (r, 0); u_1 = 1e-8 (INT_MIN): angle 6.3e-8; u_1 = 0.5 (0): angle pi, (-r, 0)
    assert got[2].real == f32(6.0697083) and got[2].imag == 0
    assert got[3].real == f32(6.0697083) and abs(got[3].imag - 6.0697083 * 2 * np.pi * 1.0000000050247593e-08) < 1e-12
    assert got[4].real == f32(-6.0697083) and got[4].imag == 0
    assert np.abs(got - want).max() < 1e-6
    assert np.abs(got).max() <= f32(6.0697083)
    r0 = np.sqrt(-2 * np.log(0.5))
    assert abs(got[5].real + r0) < 2e-7 and got[5].imag == 0 and abs(got[6].real - r0) < 2e-7 and abs(got[7].real - r0) < 2e-7


N_ACC = 1 << 18


@pytest.fixture(scope="module")
def acc_words():
    return nm.gaussian_words(2024, 1, 0, N_ACC)


def err_figures(got, want):
    d = got.astype(np.complex128) - want
    return max(np.abs(d.real).max(), np.abs(d.imag).max()), np.sqrt(np.mean(np.abs(d) ** 2) / np.mean(np.abs(want) ** 2))


def test_gaussian_against_the_float64_model(L, acc_words):
    """The project's float gate: relative RMS <= 1e-5 (measured 4.5e-8, max abs 6.4e-7, 62 % of the values bit-equal to the rounded model: DESIGN 4s)"""
    got = csdr_amd.noise_from_words("gaussian", acc_words)
    mx, rr = err_figures(got, nm.gaussian_from_words(acc_words))
    eq = np.mean(bits(got) == bits(nm.gaussian_from_words(acc_words).astype(c64)))
    print("hook vs float64 model on %d samples: max abs %.3g, relative RMS %.3g, bit-equal %.1f %%" % (N_ACC, mx, rr, 100 * eq))
    assert rr <= 1e-5
    assert np.array_equal(bits(got), bits(csdr_amd.noise_debug_walk("gaussian", 2024, 1, 0, N_ACC)))


def test_gaussian_max_error_within_four_times_the_references(L, reflib, acc_words, tmp_path):
    """max abs against the float64 model within 4 x what the compiled reference (-ffast-math) shows against the same model on the same words"""
    want = nm.gaussian_from_words(acc_words)
    ref = from_file(reflib.get_random_gaussian_samples_c, acc_words, N_ACC, c64, tmp_path)
    ref_mx, ref_rr = err_figures(ref, want)
    mx, rr = err_figures(csdr_amd.noise_from_words("gaussian", acc_words), want)
    print("reference vs model: max abs %.3g, relative RMS %.3g; hook vs model: max abs %.3g, relative RMS %.3g" % (ref_mx, ref_rr, mx, rr))
    assert ref_mx < 1e-5                          # (a sane reference build: 1.55e-6 measured)
    assert mx <= 4 * ref_mx


def test_random_sample_drop_ins_read_their_words_from_the_file(L, acc_words, tmp_path):
    """get_random_samples_f / get_random_gaussian_samples_c of the library are functions of the words in their FILE *"""
    D = C.CDLL(csdr_amd.LIB_PATH)
    for fn in (D.get_random_samples_f, D.get_random_gaussian_samples_c):
        fn.restype = None; fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    w = acc_words[:8192]
    assert np.array_equal(bits(from_file(D.get_random_gaussian_samples_c, w, 4096, c64, tmp_path)), bits(csdr_amd.noise_from_words("gaussian", w)))
    assert np.array_equal(bits(from_file(D.get_random_samples_f, w, 8192, f32, tmp_path)), bits(nm.uniform_from_words(w)))
    D.init_get_random_samples_f.restype = C.c_void_p; D.deinit_get_random_samples_f.argtypes = [C.c_void_p]
    f = D.init_get_random_samples_f()
    assert f
    out = np.zeros(16, f32)
    D.get_random_samples_f(out.ctypes.data_as(C.c_void_p), 16, C.c_void_p(f))
    assert D.deinit_get_random_samples_f(C.c_void_p(f)) == 0 and np.abs(out).max() <= 1 and np.unique(out).size > 1
    a = np.arange(7, dtype=f32); b = np.full(7, 0.1, f32); o = np.zeros(7, f32)
    D.add_ff.restype = C.c_void_p; D.add_ff.argtypes = [C.c_void_p] * 3 + [C.c_int]
    assert D.add_ff(a.ctypes.data, b.ctypes.data, o.ctypes.data, 7) == o.ctypes.data and np.array_equal(o, a + b)


def test_uniform_drop_in_is_bit_equal_to_the_reference(L, reflib, acc_words, tmp_path):
    ref = from_file(reflib.get_random_samples_f, acc_words, acc_words.size, f32, tmp_path)
    assert np.array_equal(bits(ref), bits(nm.uniform_from_words(acc_words)))


# ---------------------------------------------------------------- awgn_cc --awgnfile
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_gains_are_the_models(L):
    for snr in (6.0, -3.5, 40.0, 0.0, -10.0, 17.25, 100.0, -100.0):
        a, g = csdr_amd.awgn_gains(snr)
        ma, mg = nm.awgn_gains(snr)
        assert bits(f32(a)) == bits(f32(ma)) and bits(f32(g)) == bits(f32(mg)), snr


@pytest.mark.parametrize("k", [0, 1, 2])
def test_awgnfile_model_and_host_formula_against_the_golden_bytes(L, golden, k):
    """The reference binary's bytes (tests/golden/make_awgn_golden.py): 4 blocks of 1024 at 6, -3.5 and 40 dB, noise blocks 0, 1, 2, 0 of a file of 3 blocks + 100
    floats.  The model and the host run of the flat awgn_cc give them to the bit.  (The binary's fifth block is the stale one it emits after its input ends.)"""
    x, nf, snr, B = golden["x"], golden["noise_file"].view(c64), float(golden["snr_db"][k]), int(golden["bufsize"])
    y = golden["y%d" % k]
    assert x.size == 4 * B and nf.size == 3 * B + 50 and y.size == 5 * B
    want = y[:4 * B]
    assert np.array_equal(bits(nm.awgn_cc_file(x, snr, nf, B)), bits(want))
    noise = nm.awgnfile_noise(nf, B, 4)
    assert np.array_equal(noise[3 * B:], nf[:B])
    assert np.array_equal(bits(csdr_amd.awgn_debug_mix(x, noise, snr)), bits(want))


@pytest.mark.parametrize("snr", [6.0, -3.5, 40.0])
def test_awgnfile_against_the_reference_binary(L, golden, snr):
    if not os.path.exists(REF_CSDR):
        pytest.skip("reference binary not built (oracle/_ref/csdr)")
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_awgn_golden as mk
    rng = np.random.default_rng(int(snr * 10) + 100)
    B, nb = 1024, 5
    x = (rng.uniform(-1, 1, nb * B) + 1j * rng.uniform(-1, 1, nb * B)).astype(c64)
    nf = nm.gaussian(int(snr * 10) + 200, 3, 17, 3 * B + 50).astype(c64)
    y = mk.ref_awgn_file(x, snr, nf.view(f32), B)
    want = y[:nb * B]
    assert np.array_equal(bits(nm.awgn_cc_file(x, snr, nf, B)), bits(want))
    assert np.array_equal(bits(csdr_amd.awgn_debug_mix(x, nm.awgnfile_noise(nf, B, nb), snr)), bits(want))


# ---------------------------------------------------------------- measurements
def timing_rows():
    rng = np.random.default_rng(77)
    rows = []
    for n, sps, off in ((300, 8, 3), (257, 256, 85), (64, 5, 0), (2, 8, 1), (100, 7, 6)):
        idx = (off + sps * np.arange(n) + rng.integers(-sps // 2, sps // 2 + 1, n)).astype(np.int64)
        idx[0] = max(idx[0], 0)
        rows.append((idx.astype(u32), sps, off))
    rows.append((np.array([1, 0xfffffff0, 5, 2 ** 31], u32), 8, 3))      # below the offset (the unsigned difference wraps) and beyond 2^31
    return rows


def test_timing_variance_drop_in_is_the_model(L):
    D = C.CDLL(csdr_amd.LIB_PATH)
    D.normalized_timing_variance_u32_f.restype = C.c_float; D.normalized_timing_variance_u32_f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    for idx, sps, off in timing_rows():
        want = nm.normalized_timing_variance_u32_f(idx, sps, off)
        got = f32(D.normalized_timing_variance_u32_f(idx.ctypes.data, None, idx.size, sps, off, 0))
        assert bits(got) == bits(want) and bits(csdr_amd.debug_timing_variance(idx, sps, off)) == bits(want), (sps, off)
    one = np.array([11], u32)
    assert np.isnan(csdr_amd.debug_timing_variance(one, 8, 3)) and np.isnan(nm.normalized_timing_variance_u32_f(one, 8, 3))       # 0 / 0, as the reference
    assert csdr_amd.debug_timing_variance(np.zeros(0, u32), 8, 3) == 0


def test_measurement_drop_ins_against_the_reference_library(L, reflib):
    """The reference is built with -ffast-math, which may reorder its sums, so it is held to what any float32 order of the same sums can differ by:
    total_logpower_cf: the sum of n non-negative terms, (n + 8) 2^-24 relative, times 10 / ln 10 for the dB; normalized_timing_variance_u32_f: 2 roundings per
    step of the running mean and 3 per term of the sum, all terms non-negative, (5 n + 8) 2^-24 relative to result + mean^2."""
    D = C.CDLL(csdr_amd.LIB_PATH)
    D.total_logpower_cf.restype = C.c_float; D.total_logpower_cf.argtypes = [C.c_void_p, C.c_int]
    rng = np.random.default_rng(5)
    for n in (1, 7, 1000, 4096):
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(c64) * f32(0.3)
        got, want = D.total_logpower_cf(x.ctypes.data, n), reflib.total_logpower_cf(x.ctypes.data, n)
        print("total_logpower_cf n %d: ours %.7f, reference %.7f, float64 %.7f" % (n, got, want, nm.total_logpower_cf(x)))
        assert abs(got - want) <= 10 / np.log(10) * (n + 8) * 2.0 ** -24 + 4 * np.spacing(f32(abs(want)))
    for idx, sps, off in timing_rows():
        n = idx.size
        tmp = np.zeros(n, f32)
        want = reflib.normalized_timing_variance_u32_f(idx.ctypes.data, tmp.ctypes.data, n, sps, off, 0)
        got = float(csdr_amd.debug_timing_variance(idx, sps, off))
        mean = float(np.mean(tmp))
        print("timing variance n %d sps %d: ours %.8g, reference %.8g" % (n, sps, got, want))
        assert abs(got - want) <= (5 * n + 8) * 2.0 ** -24 * (abs(want) + mean * mean), (sps, off)


# ---------------------------------------------------------------- moments
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_moments_of_a_million_samples(L, seed):
    """|mean| < 5 / sqrt(n) on each part and |var - v0| < 5 sqrt(2 / n) v0, v0 the variance of the transform's own distribution (noise_model.V0).  Conditions
    on fixed seeds: the float64 model passes for these three (checked here as well)."""
    n = 1 << 20
    got = csdr_amd.noise_debug_walk("gaussian", seed, 0, 0, n).astype(np.complex128)
    for g in (got, nm.gaussian(seed, 0, 0, n)):
        for part in (g.real, g.imag):
            assert abs(part.mean()) < 5 / np.sqrt(n)
            assert abs(part.var() - nm.V0) < 5 * np.sqrt(2 / n) * nm.V0
    assert abs(np.mean(got.real * got.imag)) < 5 / np.sqrt(n)
