"""The waterfall path on the MI355X (waterfall.hip): the one-pass kernel and the generic composition against the float64 model, call splits, batches,
the compressed rows, the stand-alone stages and the CLI against the reference binary, and the drop-in accumulate_power_cf / log_ff."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import waterfall_model as wm

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


def _stream(rng, in_format, n, tone=0.0731):
    if in_format == "u8":
        t = np.arange(n)
        z = 0.6 * np.exp(2j * np.pi * tone * t) + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        iq = np.empty(2 * n); iq[0::2] = z.real; iq[1::2] = z.imag
        return np.clip(np.round(127.5 * (iq + 1)), 0, 255).astype(np.uint8)
    t = np.arange(n)
    x = 0.5 * np.exp(2j * np.pi * tone * t) + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def _n_for_rows(fft, every, avg, rows):
    off = every - fft if every < fft else 0
    return (rows * avg - 1) * every + off + fft


def _check_rows(db, x, in_format, fft, every, avg, add_db, window_table):
    want_p, want_db = wm.rows(x, in_format, fft, every, window_table, avg, add_db)
    assert db.shape == want_db.shape, (db.shape, want_db.shape)
    got_p = 10.0 ** ((db.astype(np.float64) - float(wm.add_db_eff(add_db, avg))) / 10)
    for r in range(db.shape[0]):
        assert wm.relrms(got_p[r], want_p[r]) <= 1e-5, r
    assert wm.db_gate(db, want_db) <= 0.01


@pytest.mark.parametrize("fft", [1024, 2048, 4096, 8192])
@pytest.mark.parametrize("in_format", ["cf32", "u8"])
@pytest.mark.parametrize("every_kind,avg", [("below", 7), ("equal", 1), ("above", 7), ("below", 93)])
def test_onepass_against_model(ctx, port, fft, in_format, every_kind, avg):
    every = {"below": fft * 7 // 10, "equal": fft, "above": fft + 613}[every_kind]
    rows = 1 if avg == 93 else 3
    rng = np.random.default_rng(fft + avg)
    n = _n_for_rows(fft, every, avg, rows) + every // 2
    x = _stream(rng, in_format, n)
    w = ctx.waterfall(fft, every, avg, -70.0, in_format=in_format, out_format="db", n_streams=1, max_samples_per_call=n)
    db = w.process(x[None])[0]
    assert w.kernel_name().startswith("k_wf_onepass")
    _check_rows(db, x, in_format, fft, every, avg, -70.0, port.precalculate_window(fft, "HAMMING"))
    w.close()


@pytest.mark.parametrize("fft", [256, 16384, 1024])
@pytest.mark.parametrize("in_format", ["cf32", "u8"])
def test_generic_against_model(ctx, port, fft, in_format):
    """fft 256 / 16384 have no one-pass form; 1024 is forced onto the generic path (the A/B of bench_waterfall.py --generic)"""
    every, avg, rows = fft * 7 // 10, 7, 3
    rng = np.random.default_rng(fft)
    n = _n_for_rows(fft, every, avg, rows)
    x = _stream(rng, in_format, n)
    w = ctx.waterfall(fft, every, avg, 3.0, in_format=in_format, out_format="db", n_streams=2, max_samples_per_call=n)
    if fft == 1024:
        w.force_generic()
    db = w.process(np.stack([x, x]))
    assert w.kernel_name().startswith("k_wf_post")
    _check_rows(db[0], x, in_format, fft, every, avg, 3.0, port.precalculate_window(fft, "HAMMING"))
    assert np.array_equal(db[0].view(np.uint32), db[1].view(np.uint32))
    w.close()


@pytest.mark.parametrize("fft,every,generic", [(4096, 2867, False), (2048, 2500, False), (1024, 1024, False), (512, 300, True), (4096, 2867, True)])
def test_call_splits_bit_identical(ctx, fft, every, generic):
    """calls that end mid-frame, mid-skip (every > fft) and mid-row, and calls shorter than every_n: the same rows, bit for bit, on both paths (the
    generic path runs one fixed-batch hipFFT plan whatever the call size)"""
    avg = 5
    rng = np.random.default_rng(every)
    n = _n_for_rows(fft, every, avg, 4) + 3 * every + 17
    x = _stream(rng, "u8", n)
    outs = []
    splits = [[n], [every // 3, every // 3, 5, fft + 7, every * avg + 1, n], [n // 7] * 7 + [n], [1, 2, 3, every - 1, n]]
    for sp in splits:
        calls, left = [], n
        for k in sp:
            k = min(k, left)
            if k:
                calls.append(k); left -= k
        w = ctx.waterfall(fft, every, avg, 0.0, in_format="u8", out_format="db", n_streams=1, max_samples_per_call=n)
        if generic:
            w.force_generic()
        outs.append(w.process(x[None], calls)[0])
        w.close()
    assert outs[0].shape[0] == 4
    for o in outs[1:]:
        assert np.array_equal(o.view(np.uint32), outs[0].view(np.uint32))


def test_batch_rows_equal_single_streams(ctx):
    """64 distinct streams with in_pitch > n_in: each stream's rows are bit-identical to that stream processed alone"""
    fft, every, avg, S = 4096, 2867, 3, 64
    rng = np.random.default_rng(64)
    n = _n_for_rows(fft, every, avg, 3)
    pitch = n + 333
    X = np.stack([_stream(rng, "u8", pitch, tone=0.01 + 0.007 * s) for s in range(S)])
    import csdr_amd
    w = ctx.waterfall(fft, every, avg, 0.0, in_format="u8", out_format="adpcm", n_streams=S, max_samples_per_call=n)
    di = ctx.upload(X)
    opitch = 6 * w.row_bytes + 64
    do = ctx.alloc(opitch * S)
    r = w.process_dev(di.ptr, n, pitch, do.ptr, opitch)
    assert r == 3
    Y = ctx.download(do, np.uint8, opitch * S).reshape(S, opitch)[:, :r * w.row_bytes]
    w.close()
    for s in range(0, S, 9):
        w1 = ctx.waterfall(fft, every, avg, 0.0, in_format="u8", out_format="adpcm", n_streams=1, max_samples_per_call=n)
        one = w1.process(X[s:s + 1, :2 * n])[0].ravel()
        w1.close()
        assert np.array_equal(one, Y[s]), s
    assert isinstance(csdr_amd.Waterfall, type)


@pytest.mark.parametrize("fft", [4096, 256])
def test_adpcm_rows_equal_compressed_db_rows(ctx, fft):
    every, avg = fft * 7 // 10, 4
    rng = np.random.default_rng(fft + 1)
    n = _n_for_rows(fft, every, avg, 3)
    x = _stream(rng, "u8", n)
    wd = ctx.waterfall(fft, every, avg, -20.0, in_format="u8", out_format="db", n_streams=1, max_samples_per_call=n)
    wa = ctx.waterfall(fft, every, avg, -20.0, in_format="u8", out_format="adpcm", n_streams=1, max_samples_per_call=n)
    db = wd.process(x[None])[0]; ad = wa.process(x[None])[0]
    assert wd.kernel_name() == wa.kernel_name()
    want = ctx.compress_fft_adpcm_f_u8(db.ravel(), fft)
    assert np.array_equal(ad.ravel(), np.asarray(want).ravel())
    wd.close(); wa.close()


def _ref(args, data):
    return subprocess.run([REF_CSDR] + args, input=data, capture_output=True, timeout=120).stdout


def _ulp(a, b):
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


@need_ref
def test_standalone_stages_against_reference(ctx):
    rng = np.random.default_rng(9)
    fft, avg, rows = 2048, 6, 5
    spec = (rng.standard_normal((rows * avg, fft)) + 1j * rng.standard_normal((rows * avg, fft))).astype(np.complex64)
    got = ctx.logaveragepower_cf(spec, fft, avg, -12.5)
    ref = np.frombuffer(_ref(["logaveragepower_cf", "-12.5", str(fft), str(avg)], spec.tobytes()), np.float32)[:rows * fft].reshape(rows, fft)
    assert _ulp(got, ref).max() <= 4
    r = rng.standard_normal((rows, fft)).astype(np.float32)
    sw = ctx.fft_exchange_sides_ff(r, fft)
    refsw = np.frombuffer(_ref(["fft_exchange_sides_ff", str(fft)], r.tobytes()), np.float32)[:rows * fft].reshape(rows, fft)
    assert np.array_equal(sw.view(np.uint32), refsw.view(np.uint32))


def _run(cmd, data, env=None):
    e = dict(os.environ); e.update(env or {})
    r = subprocess.run(cmd, input=data, capture_output=True, timeout=120, env=e)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr.decode()


@need_ref
def test_cli_stages_against_reference():
    rng = np.random.default_rng(10)
    fft, avg, rows = 1024, 4, 6
    spec = (rng.standard_normal((rows * avg, fft)) + 1j * rng.standard_normal((rows * avg, fft))).astype(np.complex64)
    ours, _ = _run([CSDR, "logaveragepower_cf", "-30", str(fft), str(avg)], spec.tobytes())
    ref = _ref(["logaveragepower_cf", "-30", str(fft), str(avg)], spec.tobytes())
    a = np.frombuffer(ours, np.float32); b = np.frombuffer(ref, np.float32)[:a.size]
    assert a.size == rows * fft and _ulp(a, b).max() <= 4
    r = rng.standard_normal(rows * fft).astype(np.float32)
    ours, _ = _run([CSDR, "fft_exchange_sides_ff", str(fft)], r.tobytes())
    ref = _ref(["fft_exchange_sides_ff", str(fft)], r.tobytes())
    assert ours == ref[:len(ours)] and len(ours) == r.nbytes


@need_ref
def test_cli_chain_fused_pattern():
    """the five-stage u8 pattern in `csdr chain` is recognised and equals the stages as separate processes and the reference pipeline (ADPCM codes: < 2 % differ)"""
    fft, every, avg = 2048, 1434, 10
    rng = np.random.default_rng(11)
    n = _n_for_rows(fft, every, avg, 6)
    x = _stream(rng, "u8", n).tobytes()
    stages = ["convert_u8_f", "fft_cc %d %d" % (fft, every), "logaveragepower_cf -70 %d %d" % (fft, avg), "fft_exchange_sides_ff %d" % fft,
              "compress_fft_adpcm_f_u8 %d" % fft]
    fused, err = _run([CSDR, "chain", " | ".join(stages)], x)
    assert "waterfall pattern recognised" in err
    sh = " | ".join("%s %s" % (CSDR, s) for s in stages)
    split = subprocess.run(["bash", "-c", sh], input=x, capture_output=True, timeout=300).stdout
    ref = subprocess.run(["bash", "-c", " | ".join("%s %s" % (REF_CSDR, s) for s in stages)], input=x, capture_output=True, timeout=300).stdout
    rb = (fft + 10) // 2
    assert len(fused) == 6 * rb
    for other in (split, ref):
        m = min(len(fused), len(other)) // rb * rb
        assert m >= 5 * rb
        a = np.frombuffer(fused[:m], np.uint8); b = np.frombuffer(other[:m], np.uint8)
        codes_a = np.stack([a & 15, a >> 4]); codes_b = np.stack([b & 15, b >> 4])
        assert np.mean(codes_a != codes_b) < 0.02


def test_cli_bank_equals_single_stream(tmp_path):
    fft, every, avg = 4096, 2867, 5
    rng = np.random.default_rng(12)
    n = _n_for_rows(fft, every, avg, 3) + 1000
    args, singles = [], []
    for k in range(3):
        data = _stream(rng, "u8", n, tone=0.02 + 0.05 * k).tobytes()
        (tmp_path / ("in%d" % k)).write_bytes(data)
        args += [str(tmp_path / ("in%d" % k)), str(tmp_path / ("out%d" % k))]
        singles.append(_run([CSDR, "waterfall_u8", str(fft), str(every), "HAMMING", "-70", str(avg), "adpcm"], data)[0])
    _run([CSDR, "waterfall_bank_u8", str(fft), str(every), "HAMMING", "-70", str(avg), "adpcm"] + args, b"")
    for k in range(3):
        got = (tmp_path / ("out%d" % k)).read_bytes()
        assert len(got) == 3 * ((fft + 10) // 2) and got == singles[k]


def test_dropin_accumulate_power_and_log():
    import torch  # noqa: F401
    import csdr_amd
    L = csdr_amd.lib()
    L.accumulate_power_cf.argtypes = [C.c_void_p, C.c_void_p, C.c_int]; L.accumulate_power_cf.restype = None
    L.log_ff.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float]; L.log_ff.restype = None
    rng = np.random.default_rng(13)
    n = 5000
    a = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    b = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    acc = np.zeros(n, np.float32)
    L.accumulate_power_cf(a.ctypes.data, acc.ctypes.data, n)
    L.accumulate_power_cf(b.ctypes.data, acc.ctypes.data, n)
    want = np.abs(a.astype(np.complex128)) ** 2 + np.abs(b.astype(np.complex128)) ** 2
    assert wm.relrms(acc, want) <= 1e-6
    out = np.zeros(n, np.float32)
    L.log_ff(acc.ctypes.data, out.ctypes.data, n, C.c_float(-3.0))
    assert np.abs(out - (10 * np.log10(acc.astype(np.float64)) - 3.0)).max() <= 1e-4
