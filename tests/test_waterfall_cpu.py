"""CPU checks of the waterfall path (waterfall.hip): the one-pass kernel's stages run on the CPU (csdr_amd_debug_waterfall_row) against the float64 model of
`[convert_u8_f |] fft_cc | logaveragepower_cf | fft_exchange_sides_ff`, and the model's own half order, add_db' and framing against the reference binary."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import waterfall_model as wm

HERE = os.path.dirname(os.path.abspath(__file__))
REF_CSDR = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "csdr")


def _stream(rng, in_format, n):
    if in_format == "u8":
        return rng.integers(0, 256, 2 * n, dtype=np.uint8)
    t = np.arange(n)
    x = 0.5 * np.exp(2j * np.pi * 0.0731 * t) + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


@pytest.mark.parametrize("fft", [1024, 2048, 4096, 8192])
@pytest.mark.parametrize("in_format", ["cf32", "u8"])
@pytest.mark.parametrize("every_kind,avg", [("below", 7), ("equal", 1), ("above", 7), ("below", 93)])
def test_onepass_row_stages_on_cpu(fft, in_format, every_kind, avg):
    """The CPU run of the one-pass kernel's stages (index maps, LDS exchanges, power tree of the twiddles, accumulation order) for the first row of a
    fresh stream: linear averaged power within 2e-6 relative RMS of the float64 model, dB row in the same (exchanged) order."""
    import csdr_amd
    import oracle
    if avg == 93 and fft > 2048:
        pytest.skip("avg 93 is covered at the small sizes (CPU time)")
    every = {"below": fft * 7 // 10, "equal": fft, "above": fft + 613}[every_kind]
    L = csdr_amd.lib()
    f = L.csdr_amd_debug_waterfall_row
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]; f.restype = C.c_int
    rng = np.random.default_rng(fft + avg + len(every_kind))
    off = every - fft if every < fft else 0
    n = (avg - 1) * every + off + fft
    x = _stream(rng, in_format, n)
    db = np.zeros(fft, np.float32); pw = np.zeros(fft, np.float32)
    fmt = 1 if in_format == "u8" else 0
    assert f(fft, every, 2, avg, -70.0, fmt, x.ctypes.data, n, db.ctypes.data, pw.ctypes.data) == 0
    want_p, want_db = wm.rows(x, in_format, fft, every, oracle.port().precalculate_window(fft, "HAMMING"), avg, -70.0)
    assert want_p.shape[0] == 1
    assert wm.relrms(pw, want_p[0]) <= 2e-6
    assert wm.db_gate(db, want_db[0]) <= 0.01
    assert f(fft, every, 2, avg, -70.0, fmt, x.ctypes.data, n - 1, db.ctypes.data, pw.ctypes.data) != 0     # the row's last frame is incomplete
    assert f(512, every, 2, avg, -70.0, fmt, x.ctypes.data, n, db.ctypes.data, pw.ctypes.data) != 0         # not a one-pass size


def _ref(args, data):
    r = subprocess.run([REF_CSDR] + args, input=data, capture_output=True, timeout=60)
    return r.stdout


@pytest.mark.skipif(not os.path.exists(REF_CSDR), reason="reference binary oracle/_ref/csdr not built")
def test_model_stages_match_reference_binary():
    """Pin the model's logaveragepower_cf (add_db', row framing: avg spectra per row, no swap) and fft_exchange_sides_ff (second half first) to the
    reference binary on random spectra.  The swap must be byte-identical, the log values within 4 ulp.  The reference emits a stale row at EOF
    (its fread at end of stream leaves the last buffer in place): only complete rows are compared."""
    rng = np.random.default_rng(5)
    fft, avg, rows = 1024, 5, 6
    spec = (rng.standard_normal((rows * avg, fft)) + 1j * rng.standard_normal((rows * avg, fft))).astype(np.complex64)
    got = np.frombuffer(_ref(["logaveragepower_cf", "-20", str(fft), str(avg)], spec.tobytes()), np.float32)
    assert got.size >= rows * fft
    got = got[:rows * fft].reshape(rows, fft)
    p = (spec.real.astype(np.float32) ** 2 + spec.imag.astype(np.float32) ** 2).reshape(rows, avg, fft)
    acc = np.zeros((rows, fft), np.float32)
    for k in range(avg):
        acc = (acc + p[:, k]).astype(np.float32)                                 # accumulate_power_cf, frame by frame in float
    want = (np.float32(10) * np.log10(acc.astype(np.float64)).astype(np.float32) + wm.add_db_eff(-20, avg)).astype(np.float32)
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulp.max() <= 4
    rowsf = rng.standard_normal((rows, fft)).astype(np.float32)
    sw = np.frombuffer(_ref(["fft_exchange_sides_ff", str(fft)], rowsf.tobytes()), np.float32)
    assert sw.size >= rows * fft
    assert np.array_equal(sw[:rows * fft].reshape(rows, fft).view(np.uint32), np.roll(rowsf, fft // 2, axis=1).view(np.uint32))
