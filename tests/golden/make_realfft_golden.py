"""Writes tests/golden/realfft_ref_vectors.npz: the unmodified reference binary's `csdr fft_fc 32 E` output for E = 20 (overlapped frames), 64 (E = 2M) and
100 (E > 2M: the skip that counts complexf-sized items on a float stream), eight spectra each, with the input streams.  The reference repeats its last
spectrum at end of stream; that one is cut off.  Data only.  Run from the repository root where oracle/_ref/csdr exists:
    python tests/golden/make_realfft_golden.py"""
import os
import subprocess
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import realfft_model as rm  # noqa: E402

REF_CSDR = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "csdr")
GOLDEN = os.path.join(HERE, "realfft_ref_vectors.npz")
M, FRAMES, EVERY = 32, 8, (20, 64, 100)


def main():
    if not os.path.exists(REF_CSDR):
        raise SystemExit("oracle/_ref/csdr is not built")
    out = {}
    for every in EVERY:
        rng = np.random.default_rng(3200 + every)
        n = rm.n_for_rows(M, every, 1, FRAMES)
        t = np.arange(n)
        x = (0.5 * np.cos(2 * np.pi * 0.0731 * t) + 0.1 * rng.standard_normal(n)).astype(np.float32)
        y = np.frombuffer(subprocess.run([REF_CSDR, "fft_fc", str(M), str(every)], input=x.tobytes(), capture_output=True, timeout=60).stdout, np.complex64)
        assert y.size >= FRAMES * M, (every, y.size)
        out["x%d" % every], out["y%d" % every] = x, y[:FRAMES * M].reshape(FRAMES, M).copy()
    np.savez(GOLDEN, **out)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
