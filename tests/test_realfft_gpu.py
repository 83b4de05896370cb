"""The real-input spectrum path on the MI355X (waterfall.hip with CSDR_AMD_WF_IN_F32 / _S16, fft_fc, fft_one_side_ff): the one-pass real form and the generic
composition against the float64 model, the bins where the untangle can go wrong, call splits, batches, the compressed rows, the stand-alone stages and
the CLI through real pipes, and that the complex objects are untouched.

The float gates are the waterfall's (tests/test_waterfall_gpu.py): per-row relative RMS of the power <= 1e-5 against the float64 model, and dB within
0.01 over the bins within 60 dB of each row's peak."""
import os
import subprocess
import numpy as np
import pytest

import realfft_model as rm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
REF_CSDR = os.path.join(ROOT, "oracle", "_ref", "csdr")
need_ref = pytest.mark.skipif(not os.path.exists(REF_CSDR), reason="reference binary oracle/_ref/csdr not built")


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _quantise(x, in_format):
    return np.asarray(x, np.float64).astype(np.float32) if in_format == "f32" else np.round(np.asarray(x) * 32767).astype(np.int16)


def _stream(rng, in_format, n, tone=0.0731):
    """a tone plus noise at -34 dB"""
    return _quantise(0.5 * np.cos(2 * np.pi * tone * np.arange(n)) + 0.01 * rng.standard_normal(n), in_format)


def _check_rows(db, x, in_format, m, every, avg, add_db, window_table):
    want_p, want_db = rm.rows(x, in_format, m, every, window_table, avg, add_db)
    assert db.shape == want_db.shape, (db.shape, want_db.shape)
    got_p = 10.0 ** ((db.astype(np.float64) - float(rm.add_db_eff(add_db, avg))) / 10)
    for r in range(db.shape[0]):
        assert rm.relrms(got_p[r], want_p[r]) <= 1e-5, r
    assert rm.db_gate(db, want_db) <= 0.01


# ---- 1. the one-pass real form against the model
@pytest.mark.parametrize("m", [1024, 2048, 4096, 8192])
@pytest.mark.parametrize("in_format", ["f32", "s16"])
@pytest.mark.parametrize("every_kind,avg", [("below", 7), ("equal", 7), ("above", 7), ("below", 93)])
def test_onepass_real_against_model(ctx, port, m, in_format, every_kind, avg):
    every = {"below": (2 * m * 7 // 10) | 1, "equal": 2 * m, "above": 2 * m + 613}[every_kind]
    rows = 1 if avg == 93 else 3
    rng = np.random.default_rng(m + avg)
    n = rm.n_for_rows(m, every, avg, rows) + every // 2
    x = _stream(rng, in_format, n)
    w = ctx.waterfall(m, every, avg, -70.0, in_format=in_format, out_format="db", n_streams=1, max_samples_per_call=n)
    db = w.process(x[None])[0]
    assert w.kernel_name() == "k_wf_onepass_real (%s)" % in_format
    w.close()
    assert db.shape == (rows, m)
    _check_rows(db, x, in_format, m, every, avg, -70.0, port.precalculate_window(2 * m, "HAMMING"))


# ---- 2. the bins where the untangle can go wrong (M = 1024, avg 1)
def _one_row(ctx, x, in_format, m=1024):
    w = ctx.waterfall(m, 2 * m, 1, 0.0, in_format=in_format, out_format="db", n_streams=1, max_samples_per_call=x.size)
    db = w.process(x[None])[0]
    assert w.kernel_name().startswith("k_wf_onepass_real")
    w.close()
    return db


@pytest.mark.parametrize("in_format", ["f32", "s16"])
def test_untangle_dc_and_top_bins(ctx, port, in_format):
    """a DC offset (bin 0 is its own partner) plus a tone just below Nyquist (the top bins pair with bins 1, 2, ...)"""
    m = 1024
    x = _quantise(0.25 + 0.5 * np.cos(2 * np.pi * 0.4993 * np.arange(2 * m)), in_format)
    db = _one_row(ctx, x, in_format)
    _check_rows(db, x, in_format, m, 2 * m, 1, 0.0, port.precalculate_window(2 * m, "HAMMING"))
    floor = db[0, 8:m - 64].max()
    assert db[0, 0] > floor + 30 and db[0, m - 3:].max() > floor + 30         # (both stand out: the input exercises the bins it is meant to)


@pytest.mark.parametrize("in_format", ["f32", "s16"])
@pytest.mark.parametrize("index", [777, 1, 2047])
def test_untangle_impulse_is_flat(ctx, port, in_format, index):
    """a unit impulse at an odd sample index lives in the imaginary half of one packed point: |X[k]| = w[index] x[index] in every bin"""
    m = 1024
    x = np.zeros(2 * m); x[index] = 1.0
    x = _quantise(x, in_format)
    db = _one_row(ctx, x, in_format)[0].astype(np.float64)
    want = float(port.precalculate_window(2 * m, "HAMMING")[index]) * rm.samples(x, in_format)[index]
    assert np.abs(10.0 ** (db / 20) / want - 1).max() <= 1e-5


@pytest.mark.parametrize("in_format", ["f32", "s16"])
def test_untangle_self_partner_bin(ctx, port, in_format):
    """a tone exactly on bin M/2, the other bin that is its own partner"""
    m = 1024
    x = _quantise(0.5 * np.cos(2 * np.pi * 0.25 * np.arange(2 * m) + 0.3), in_format)
    db = _one_row(ctx, x, in_format)
    assert db[0].argmax() == m // 2
    _check_rows(db, x, in_format, m, 2 * m, 1, 0.0, port.precalculate_window(2 * m, "HAMMING"))


# ---- 3. the generic path
@pytest.mark.parametrize("m", [256, 16384, 1024])
@pytest.mark.parametrize("in_format", ["f32", "s16"])
def test_generic_real_against_model(ctx, port, m, in_format):
    """M 256 / 16384 have no one-pass form; 1024 is forced onto the generic path.  Two streams with different data."""
    every, avg, rows = (2 * m * 7 // 10) | 1, 7, 3
    rng = np.random.default_rng(m)
    n = rm.n_for_rows(m, every, avg, rows)
    X = np.stack([_stream(rng, in_format, n), _stream(rng, in_format, n, tone=0.2113)])
    w = ctx.waterfall(m, every, avg, 3.0, in_format=in_format, out_format="db", n_streams=2, max_samples_per_call=n)
    if m == 1024:
        w.force_generic()
    db = w.process(X)
    assert w.kernel_name().startswith("k_wf_post (generic real")
    w.close()
    for s in range(2):
        _check_rows(db[s], X[s], in_format, m, every, avg, 3.0, port.precalculate_window(2 * m, "HAMMING"))


# ---- 4. call splits
@pytest.mark.parametrize("m,every,generic", [(1024, 1433, False), (1024, 2661, False), (2048, 4096, False), (256, 301, True), (256, 700, True), (1024, 1433, True)])
@pytest.mark.parametrize("in_format", ["f32", "s16"])
def test_real_call_splits_bit_identical(ctx, m, every, generic, in_format):
    """calls that end mid-frame, mid-skip (E > 2M) and mid-row, 1-sample and odd-length calls: the same rows, bit for bit, on both paths"""
    avg = 5
    rng = np.random.default_rng(every)
    n = rm.n_for_rows(m, every, avg, 4) + every + 17
    x = _stream(rng, in_format, n)
    outs = []
    splits = [[n], [every // 3, every // 3, 5, 2 * m + 7, every * avg + 1, n], [n // 7] * 7 + [n], [1, 1, 3, every - 1, 2 * every - 2 * m + 1 if every > 2 * m else 77, n]]
    for sp in splits:
        calls, left = [], n
        for k in sp:
            k = min(k, left)
            if k:
                calls.append(k); left -= k
        w = ctx.waterfall(m, every, avg, 0.0, in_format=in_format, out_format="db", n_streams=1, max_samples_per_call=n)
        if generic:
            w.force_generic()
        outs.append(w.process(x[None], calls)[0])
        assert w.kernel_name().startswith("k_wf_post" if generic else "k_wf_onepass_real")
        w.close()
    assert outs[0].shape == (4, m)
    for o in outs[1:]:
        assert np.array_equal(o.view(np.uint32), outs[0].view(np.uint32))


# ---- 5. batches
@pytest.mark.parametrize("in_format,out_format", [("f32", "db"), ("s16", "adpcm"), ("f32", "adpcm"), ("s16", "db")])
@pytest.mark.parametrize("m", [2048, 512])
def test_real_batch_rows_equal_single_streams(ctx, m, in_format, out_format):
    """five distinct streams (in_pitch > n_in, an odd pitch) in one object: each stream's rows are the bytes of that stream processed alone"""
    every, avg, S = 2867 if m == 2048 else 1100, 3, 5
    rng = np.random.default_rng(m + S)
    n = rm.n_for_rows(m, every, avg, 3)
    pitch = (n + 333) | 1
    X = np.stack([_stream(rng, in_format, pitch, tone=0.01 + 0.07 * s) for s in range(S)])
    w = ctx.waterfall(m, every, avg, -10.0, in_format=in_format, out_format=out_format, n_streams=S, max_samples_per_call=n)
    assert w.row_bytes == rm.row_width(m, out_format) * (4 if out_format == "db" else 1)
    di = ctx.upload(X)
    opitch = 4 * w.row_bytes + 64
    do = ctx.alloc(opitch * S)
    r = w.process_dev(di.ptr, n, pitch, do.ptr, opitch)
    assert r == 3
    Y = ctx.download(do, np.uint8, opitch * S).reshape(S, opitch)[:, :r * w.row_bytes]
    w.close()
    for s in range(S):
        w1 = ctx.waterfall(m, every, avg, -10.0, in_format=in_format, out_format=out_format, n_streams=1, max_samples_per_call=n)
        one = w1.process(X[s:s + 1, :n])[0]
        w1.close()
        assert np.array_equal(one.ravel().view(np.uint8), Y[s]), s


# ---- 6. compressed rows
@pytest.mark.parametrize("m", [4096, 256, 8192])
@pytest.mark.parametrize("in_format", ["f32", "s16"])
def test_real_adpcm_rows_equal_compressed_db_rows(ctx, m, in_format):
    """(8192: the one-pass form whose rows are compressed in a pass of their own)"""
    every, avg = (2 * m * 7 // 10) | 1, 4
    rng = np.random.default_rng(m + 1)
    n = rm.n_for_rows(m, every, avg, 3)
    x = _stream(rng, in_format, n)
    wd = ctx.waterfall(m, every, avg, -20.0, in_format=in_format, out_format="db", n_streams=1, max_samples_per_call=n)
    wa = ctx.waterfall(m, every, avg, -20.0, in_format=in_format, out_format="adpcm", n_streams=1, max_samples_per_call=n)
    db = wd.process(x[None])[0]; ad = wa.process(x[None])[0]
    assert wd.kernel_name() == wa.kernel_name()
    wd.close(); wa.close()
    assert ad.shape == (3, (m + 10) // 2)
    want = ctx.compress_fft_adpcm_f_u8(db.ravel(), m)
    assert np.array_equal(ad.ravel(), np.asarray(want).ravel())


# ---- 7. the stand-alone stages
def _relerr(got, want):
    return float(np.sqrt(np.mean(np.abs(got - want) ** 2) / np.mean(np.abs(want) ** 2)))


FFT_FC_CASES = [(64, 20), (64, 64), (64, 128), (64, 200), (4096, 3000)]


@pytest.mark.parametrize("m,every", FFT_FC_CASES)
@pytest.mark.parametrize("calls", [1, 7])
def test_fft_fc_against_model(ctx, port, m, every, calls):
    rng = np.random.default_rng(m + every)
    x = _stream(rng, "f32", rm.n_for_rows(m, every, 1, 9) + every // 3)
    got = ctx.fft_fc(x, m, every, calls=calls)
    want = rm.spectra(x, "f32", m, every, port.precalculate_window(2 * m, "HAMMING"))
    assert got.shape == want.shape and got.shape[0] >= 9
    for f in range(got.shape[0]):
        assert _relerr(got[f], want[f]) <= 1e-5, f


@need_ref
@pytest.mark.parametrize("m,every", FFT_FC_CASES)
def test_fft_fc_against_reference_binary(ctx, m, every):
    rng = np.random.default_rng(m + every)
    x = _stream(rng, "f32", rm.n_for_rows(m, every, 1, 9) + every // 3)
    got = ctx.fft_fc(x, m, every)
    ref = np.frombuffer(subprocess.run([REF_CSDR, "fft_fc", str(m), str(every)], input=x.tobytes(), capture_output=True, timeout=120).stdout, np.complex64)
    assert got.shape[0] <= ref.size // m <= got.shape[0] + 1                   # (the reference repeats its last spectrum at end of stream)
    ref = ref[:got.size].reshape(got.shape)
    for f in range(got.shape[0]):
        assert _relerr(got[f], ref[f]) <= 1e-5, f


def test_fft_one_side_ff_bit_exact(ctx):
    rng = np.random.default_rng(21)
    for fft, rows in ((2048, 5), (6, 3), (2, 4)):
        r = rng.standard_normal((rows, fft)).astype(np.float32)
        got = ctx.fft_one_side_ff(r, fft)
        assert got.shape == (rows, fft // 2) and np.array_equal(got.view(np.uint32), r[:, :fft // 2].view(np.uint32))


# ---- 8. the CLI through real pipes
def _run(cmd, data):
    r = subprocess.run(cmd, input=data, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


def _pipe(stages, data):
    r = subprocess.run(["bash", "-c", "set -o pipefail; " + " | ".join("%s %s" % (CSDR, s) for s in stages)], input=data, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


def _ulp(a, b):
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


@need_ref
@pytest.mark.parametrize("m,every", [(64, 20), (64, 200), (4096, 3000)])
def test_cli_fft_fc_against_reference(m, every):
    rng = np.random.default_rng(m + every + 1)
    x = _stream(rng, "f32", rm.n_for_rows(m, every, 1, 12) + every // 3)
    ours = np.frombuffer(_run([CSDR, "fft_fc", str(m), str(every)], x.tobytes()), np.complex64)
    ref = np.frombuffer(subprocess.run([REF_CSDR, "fft_fc", str(m), str(every)], input=x.tobytes(), capture_output=True, timeout=120).stdout, np.complex64)
    k = rm.n_frames(x.size, m, every)
    assert ours.size == k * m and k <= ref.size // m <= k + 1                  # ours: the complete frames; the reference adds its stale last frame
    ours = ours.reshape(k, m); ref = ref[:k * m].reshape(k, m)
    for f in range(k):
        assert _relerr(ours[f], ref[f]) <= 1e-5, f


def test_cli_fft_one_side_ff_byte_exact():
    rng = np.random.default_rng(22)
    r = rng.standard_normal((7, 512)).astype(np.float32)
    assert _run([CSDR, "fft_one_side_ff", "512"], r.tobytes()) == r[:, :256].tobytes()


@pytest.mark.parametrize("every", [301, 700])
def test_cli_waterfall_ff_equals_stages(every):
    """`csdr waterfall_ff` against `csdr fft_fc | csdr logaveragepower_cf` on the same stream at <= 4 ulp per value, at a size of the generic form: both then
    run the same hipFFT plan and the same untangle, which a 4 ulp gate on dB values asks for (the one-pass transform differs from hipFFT's in the last
    bits, far inside the float gates and far outside 4 ulp in the weak bins); and the compressed rows are the bytes of compressing those rows."""
    m, avg, rows = 256, 4, 6
    rng = np.random.default_rng(every)
    x = _stream(rng, "f32", rm.n_for_rows(m, every, avg, rows) + every // 2).tobytes()
    fused = _run([CSDR, "waterfall_ff", str(m), str(every), "HAMMING", "-30", str(avg), "db"], x)
    split = _pipe(["fft_fc %d %d" % (m, every), "logaveragepower_cf -30 %d %d" % (m, avg)], x)
    a = np.frombuffer(fused, np.float32); b = np.frombuffer(split, np.float32)
    assert a.size == rows * m and b.size == a.size
    assert _ulp(a, b).max() <= 4
    packed = _run([CSDR, "waterfall_ff", str(m), str(every), "HAMMING", "-30", str(avg), "adpcm"], x)
    assert packed == _run([CSDR, "compress_fft_adpcm_f_u8", str(m)], fused) and len(packed) == rows * ((m + 10) // 2)


@pytest.mark.parametrize("cmd,in_format", [("waterfall_ff", "f32"), ("waterfall_s16", "s16")])
def test_cli_waterfall_real_onepass_against_model(port, cmd, in_format):
    """the fused commands at a one-pass size, at the float gates"""
    m, every, avg, rows = 1024, 1433, 4, 3
    rng = np.random.default_rng(23)
    x = _stream(rng, in_format, rm.n_for_rows(m, every, avg, rows) + 100)
    db = np.frombuffer(_run([CSDR, cmd, str(m), str(every), "HAMMING", "-30", str(avg), "db"], x.tobytes()), np.float32).reshape(-1, m)
    _check_rows(db, x, in_format, m, every, avg, -30.0, port.precalculate_window(2 * m, "HAMMING"))


# ---- 9. nothing existing moved
def test_complex_objects_unchanged_beside_a_real_one(ctx):
    """a cf32 and a u8 object give the same bytes before and after a real object has been created and run: the objects share no state"""
    rng = np.random.default_rng(24)
    fft, every, avg = 1024, 717, 3
    n = (3 * avg - 1) * every + every
    z = (0.5 * np.exp(2j * np.pi * 0.0731 * np.arange(n)) + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    u8 = rng.integers(0, 256, 2 * n, dtype=np.uint8)

    def run(fmt, x, generic):
        w = ctx.waterfall(fft, every, avg, -5.0, in_format=fmt, out_format="db", n_streams=1, max_samples_per_call=x.size)
        if generic:
            w.force_generic()
        y = w.process(x[None])[0]
        w.close()
        return y

    before = [run(f, x, g) for f, x in (("cf32", z), ("u8", u8)) for g in (False, True)]
    xr = _stream(rng, "f32", 4 * n)
    for g in (False, True):
        assert run("f32", xr, g).shape[1] == fft and run("s16", _quantise(xr, "s16"), g).shape[1] == fft
    after = [run(f, x, g) for f, x in (("cf32", z), ("u8", u8)) for g in (False, True)]
    for a, b in zip(before, after):
        assert a.shape[0] == 3 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
