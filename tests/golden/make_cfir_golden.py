"""Writes tests/golden/cfir_ref_vectors.npz: the unmodified reference library's apply_fir_cc on three small cases (inputs, taps from its own
firdes_add_peak_c sequence, outputs).  Data only.  Run from the repository root where oracle/_ref/libcsdr_ref.so exists:
    python tests/golden/make_cfir_golden.py"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cfir_model as cm  # noqa: E402

CASES = [(7, 300, [0.1]), (31, 400, [0.1, -0.2]), (101, 500, [0.05, -0.23, 0.31])]      # (taps_length, samples, peak rates)


def main():
    L = cm.ref_lib()
    if L is None:
        raise SystemExit("oracle/_ref/libcsdr_ref.so is not built")
    out = {}
    for k, (T, n, rates) in enumerate(CASES):
        x = cm.signal(n, 900 + k)
        h = cm.ref_peaks(L, T, rates)
        out["x%d" % k], out["h%d" % k], out["y%d" % k] = x, h, cm.ref_apply(L, x, h)
        out["rates%d" % k] = np.asarray(rates, np.float32)
    np.savez(cm.GOLDEN, **out)
    print(cm.GOLDEN, os.path.getsize(cm.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
