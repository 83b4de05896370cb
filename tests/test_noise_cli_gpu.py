"""`csdr awgn_cc`, `csdr gaussian_noise_c`, `csdr uniform_noise_f` and `csdr normalized_timing_variance_u32_f` on the GPU, through real pipes: the
--awgnfile path against the reference binary's golden bytes, the seeded sources against the CPU walk, `csdr chain` against the pipeline of processes."""
import os
import subprocess

import numpy as np
import pytest

import noise_model as nm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "csdr_amd", "csdr")
GOLDEN = os.path.join(ROOT, "tests", "golden", "awgn_ref_vectors.npz")
c64, f32, u32 = np.complex64, np.float32, np.uint32


def run(args, data, block=8192, bufsize=None, shell=False):
    assert os.path.exists(CLI), "csdr_amd/csdr not built (make -C csdr_amd/csrc)"
    env = dict(os.environ, CSDR_AMD_BLOCK=str(block))
    if bufsize:
        env["CSDR_FIXED_BUFSIZE"] = str(bufsize)
    cmd = args if shell else [CLI] + [str(a) for a in args]
    p = subprocess.run(cmd, input=np.ascontiguousarray(data).tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120, shell=shell)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout, p.stderr.decode()


@pytest.mark.parametrize("k", [0, 1, 2])
def test_awgnfile_against_the_golden_bytes(tmp_path, k):
    """csdr awgn_cc <snr> --awgnfile F with 1024-sample buffers: the reference binary's first four blocks to the bit (its fifth is the stale block it emits
    after its input has ended, which the flat stages here do not), whatever the pass size"""
    g = np.load(GOLDEN)
    f = str(tmp_path / "noise.bin")
    g["noise_file"].tofile(f)
    snr, B = float(g["snr_db"][k]), int(g["bufsize"])
    want = g["y%d" % k][:4 * B].tobytes()
    for block in (1024, 2048, 8192):
        out, err = run(["awgn_cc", snr, "--awgnfile", f], g["x"], block=block, bufsize=B)
        assert out == want, block
    assert "a_signal = " in err
    out, err = run(["awgn_cc", snr, "--awgnfile", f, "--snrshow"], g["x"], bufsize=B)
    assert out == want
    shown = [float(l.split("SNR = ")[1].split()[0]) for l in err.splitlines() if "SNR = " in l]
    a, gn = nm.awgn_gains(snr)
    noise = nm.awgnfile_noise(g["noise_file"].view(c64), B, 4)
    assert len(shown) == 4
    for b in range(4):
        sl = slice(b * B, (b + 1) * B)
        want_snr = nm.total_logpower_cf(g["x"][sl] * np.float64(a)) - nm.total_logpower_cf(noise[sl] * np.float64(gn))
        assert abs(shown[b] - want_snr) < 1e-3, (b, shown[b], want_snr)


def test_seeded_sources_against_the_walk():
    import csdr_amd
    n = 100000
    out, _ = run("%s gaussian_noise_c --seed 7 | head -c %d" % (CLI, 8 * n), b"", shell=True)
    assert out == csdr_amd.noise_debug_walk("gaussian", 7, 0, 0, n).tobytes()
    out, _ = run("%s uniform_noise_f --seed 0x1234567887654321 | head -c %d" % (CLI, 4 * n), b"", shell=True)
    assert out == csdr_amd.noise_debug_walk("uniform", 0x1234567887654321, 0, 0, n).tobytes()
    a, _ = run("%s gaussian_noise_c | head -c 4096" % CLI, b"", shell=True)                 # without --seed: eight bytes of /dev/urandom
    b, _ = run("%s gaussian_noise_c | head -c 4096" % CLI, b"", shell=True)
    assert len(a) == 4096 and a != b


def test_seeded_awgn_and_chain():
    """awgn_cc <snr> --seed S is the CPU walk of stream 0 whatever the pass size, and `csdr chain` with it between two stages equals the three processes"""
    import csdr_amd
    rng = np.random.default_rng(9)
    x = (rng.uniform(-1, 1, 30011) + 1j * rng.uniform(-1, 1, 30011)).astype(c64)
    want = csdr_amd.noise_debug_walk("gaussian", 1, 0, 0, x=x, snr_db=10.0).tobytes()
    for block in (1024, 8192, 65536):
        assert run(["awgn_cc", 10, "--seed", 1], x, block=block)[0] == want, block
    out, err = run(["awgn_cc", 10, "--seed", 1, "--snrshow"], x)
    assert out == want and err.count("SNR = ") == 30011 // 1024 + 1
    chain, _ = run(["chain", "shift_addition_cc 0.1 | awgn_cc 10 --seed 1 | realpart_cf"], x)
    pipe, _ = run("%s shift_addition_cc 0.1 | %s awgn_cc 10 --seed 1 | %s realpart_cf" % (CLI, CLI, CLI), x, shell=True)
    assert len(chain) == 4 * x.size and chain == pipe


def test_timing_variance_stage():
    rng = np.random.default_rng(4)
    sps, off, B = 8, 3, 1024
    idx = (off + sps * np.arange(3 * B + 100) + rng.integers(-4, 5, 3 * B + 100)).astype(u32)
    out, err = run(["normalized_timing_variance_u32_f", sps, off], idx, bufsize=B)
    got = np.frombuffer(out, f32)
    want = [nm.normalized_timing_variance_u32_f(idx[k * B:(k + 1) * B], sps, off) for k in range(4)]
    assert got.size == 4 and np.array_equal(got.view(u32), np.array(want, f32).view(u32))
    assert err.count("normalized variance = ") == 4
