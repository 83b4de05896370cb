"""CPU checks of the real-input spectrum path (waterfall.hip, CSDR_AMD_WF_IN_F32 / _S16): the float64 model of `[convert_s16_f |] fft_fc | logaveragepower_cf`
against the reference binary's recorded output (and the binary itself where built), the one-pass kernel's stages run on the CPU
(csdr_amd_debug_waterfall_row_at: packed load, the M-point passes, the untangling exchange) against the model, and the schedule's formulas."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import realfft_model as rm

HERE = os.path.dirname(os.path.abspath(__file__))
REF_CSDR = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "csdr")
GOLDEN = os.path.join(HERE, "golden", "realfft_ref_vectors.npz")
FORMATS = {"f32": 2, "s16": 3}                                   # CSDR_AMD_WF_IN_F32 / _S16


def _stream(rng, in_format, n, tone=0.0731):
    """a tone plus noise at -34 dB"""
    t = np.arange(n)
    x = 0.5 * np.cos(2 * np.pi * tone * t) + 0.01 * rng.standard_normal(n)
    return x.astype(np.float32) if in_format == "f32" else np.round(x * 32767).astype(np.int16)


def _window(n):
    import oracle
    return oracle.port().precalculate_window(n, "HAMMING")


def _relerr(got, want):
    return float(np.sqrt(np.mean(np.abs(got - want) ** 2) / np.mean(np.abs(want) ** 2)))


@pytest.mark.parametrize("every", [20, 64, 100])
def test_model_against_recorded_reference(every):
    """the reference binary's `fft_fc 32 E`, recorded by tests/golden/make_realfft_golden.py: E below, equal to and above 2M (the last pins P = 2E - 2M)"""
    g = np.load(GOLDEN)
    x, want = g["x%d" % every], g["y%d" % every]
    got = rm.spectra(x, "f32", 32, every, _window(64))
    assert got.shape == want.shape == (8, 32)
    for f in range(8):
        assert _relerr(got[f], want[f]) <= 1e-6, f


@pytest.mark.skipif(not os.path.exists(REF_CSDR), reason="reference binary oracle/_ref/csdr not built")
@pytest.mark.parametrize("m,every", [(32, 20), (32, 64), (32, 100), (512, 300)])
def test_model_against_reference_binary(m, every):
    """the model's frames are a prefix of the reference's (which repeats its last frame at end of stream) at <= 1e-6 relative RMS per frame"""
    rng = np.random.default_rng(m + every)
    x = _stream(rng, "f32", rm.n_for_rows(m, every, 1, 9) + every // 3)
    ref = np.frombuffer(subprocess.run([REF_CSDR, "fft_fc", str(m), str(every)], input=x.tobytes(), capture_output=True, timeout=60).stdout, np.complex64)
    got = rm.spectra(x, "f32", m, every, _window(2 * m))
    assert got.shape[0] >= 9 and got.shape[0] <= ref.size // m <= got.shape[0] + 1
    ref = ref[:got.size].reshape(got.shape)
    for f in range(got.shape[0]):
        assert _relerr(got[f], ref[f]) <= 1e-6, f


def _debug_row():
    import csdr_amd
    f = csdr_amd.lib().csdr_amd_debug_waterfall_row_at
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]; f.restype = C.c_int
    return f


@pytest.mark.parametrize("m", [1024, 2048, 4096, 8192])
@pytest.mark.parametrize("in_format", ["f32", "s16"])
@pytest.mark.parametrize("every_kind,avg", [("below", 7), ("equal", 7), ("above", 7), ("below", 93)])
def test_onepass_real_row_stages_on_cpu(m, in_format, every_kind, avg):
    """The CPU run of the real one-pass form's stages for the first rows of a stream, at the waterfall's two gates: per-row relative RMS of the power
    <= 1e-5 against the float64 model, dB within 0.01 over the bins within 60 dB of the row's peak."""
    every = {"below": (2 * m * 7 // 10) | 1, "equal": 2 * m, "above": 2 * m + 613}[every_kind]
    rows = 1 if avg == 93 else 3
    f = _debug_row()
    rng = np.random.default_rng(m + avg + len(every_kind))
    n = rm.n_for_rows(m, every, avg, rows)
    x = _stream(rng, in_format, n)
    want_p, want_db = rm.rows(x, in_format, m, every, _window(2 * m), avg, -70.0)
    assert want_p.shape == (rows, m)
    db = np.zeros(m, np.float32); pw = np.zeros(m, np.float32)
    for r in range(rows):
        assert f(m, every, 2, avg, -70.0, FORMATS[in_format], x.ctypes.data, n, r, db.ctypes.data, pw.ctypes.data) == 0
        assert rm.relrms(pw, want_p[r]) <= 1e-5, r
        assert rm.db_gate(db, want_db[r]) <= 0.01, r
    assert f(m, every, 2, avg, -70.0, FORMATS[in_format], x.ctypes.data, n - 1, rows - 1, db.ctypes.data, pw.ctypes.data) != 0   # the last frame is incomplete
    assert f(512, every, 2, avg, -70.0, FORMATS[in_format], x.ctypes.data, n, 0, db.ctypes.data, pw.ctypes.data) != 0            # not a one-pass size


def test_schedule_formulas():
    """frame counts of both schedules, counted by stepping through the stream as the reference's loop does, and the row widths"""
    for m, every in [(32, 1), (32, 20), (32, 63), (32, 64), (32, 65), (32, 100), (32, 200), (512, 300), (1024, 2661)]:
        n = 2 * m
        assert rm.schedule(m, every) == ((n, every, every - n) if every <= n else (n, 2 * every - n, 0))
        for total in (0, 1, n - 1, n, n + 1, every, 3 * every + 5, 10 * every + n, 10 * (2 * every - n) + n - 1 if every > n else 7 * every - 1):
            if every <= n:
                count = total // every                                   # one frame per E new samples, the first after E samples
            else:
                count, at = 0, 0
                while at + n <= total:                                   # 2M floats read, then 2 (E - 2M) floats skipped
                    count += 1; at += n + 2 * (every - n)
            assert rm.n_frames(total, m, every) == count, (m, every, total)
        for rows, avg in ((1, 1), (3, 7)):
            need = rm.n_for_rows(m, every, avg, rows)
            assert rm.n_frames(need, m, every) == rows * avg and rm.n_frames(need - 1, m, every) == rows * avg - 1
    assert rm.row_width(1024, "db") == 1024 and rm.row_width(1024, "adpcm") == 517 and rm.row_width(32, "adpcm") == 21
