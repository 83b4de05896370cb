"""Writes tests/golden/awgn_ref_vectors.npz: the unmodified reference binary's `csdr awgn_cc <snr_db> --awgnfile F` with 1024-sample blocks
(CSDR_FIXED_BUFSIZE) at 6, -3.5 and 40 dB on a 4-block signal and a noise file of 3 blocks + 100 floats (so the blocks cycle 0, 1, 2, 0 and the
partial tail is never used).  The binary's whole output is kept: 4 blocks, then the one stale block it emits after the end of its input.  Data only.
Run from the repository root where oracle/_ref/csdr exists:
    python tests/golden/make_awgn_golden.py"""
import os
import subprocess
import sys
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import noise_model as nm  # noqa: E402

GOLDEN = os.path.join(HERE, "awgn_ref_vectors.npz")
REF_CSDR = os.path.join(ROOT, "oracle", "_ref", "csdr")
BUFSIZE, BLOCKS, SNRS = 1024, 4, (6.0, -3.5, 40.0)


def ref_awgn_file(x, snr_db, noise_file, bufsize=BUFSIZE):
    """the reference binary's output bytes as complex64"""
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "noise.bin")
        np.ascontiguousarray(noise_file, np.float32).tofile(f)
        r = subprocess.run([REF_CSDR, "awgn_cc", repr(float(snr_db)), "--awgnfile", f], input=np.ascontiguousarray(x, np.complex64).tobytes(),
                           capture_output=True, env=dict(os.environ, CSDR_FIXED_BUFSIZE=str(bufsize)), check=True)
    return np.frombuffer(r.stdout, np.complex64).copy()


def main():
    if not os.path.exists(REF_CSDR):
        raise SystemExit("oracle/_ref/csdr is not built")
    rng = np.random.default_rng(4242)
    n = BUFSIZE * BLOCKS
    x = (0.6 * np.exp(2j * np.pi * 0.01 * np.arange(n)) + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    noise = nm.gaussian(99, 0, 0, 3 * BUFSIZE + 50).astype(np.complex64).view(np.float32)          # 3 blocks + 100 floats
    out = {"x": x, "noise_file": noise, "snr_db": np.asarray(SNRS, np.float32), "bufsize": np.int32(BUFSIZE)}
    for k, snr in enumerate(SNRS):
        out["y%d" % k] = ref_awgn_file(x, snr, noise)
    np.savez_compressed(GOLDEN, **out)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes", [out["y%d" % k].size for k in range(len(SNRS))])


if __name__ == "__main__":
    main()
