"""Every kernel path of the demodulator and audio-rate blocks (audio.hip, f2blocks.hip) at its switch points, through raw C-ABI calls: input rows with
pitch > n and 1e30 in the padding, output buffers pre-filled with a pattern that must survive behind n and between rows.  Blocks whose kernels restate the
reference operation for operation are held to the oracle's bits; the others to a per-sample gate against float64 (audio_model.py; the gates are established by
test_audio_blocks_cpu.py).  deemphasis_wfm_ff, agc_ff and fractional_decimator_ff cases assert the path they mean to hit (csdr_amd_audio_last_path), so a change
in the dispatch fails here instead of silently dropping coverage."""
import ctypes as C
import numpy as np
import pytest

import audio_model as am
from audio_model import f32, f64, c64, SENTINEL, PATTERN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _report(*a):
    print("RATIO", *a)


def _path(ctx):
    return ctx.L.csdr_amd_audio_last_path().decode()


# ------------------------------------------------------------------ pitched rows, sentinel padding, patterned outputs
class Rows:
    """a device array of s rows of `pitch` elements behind `lead` elements (lead: to move the first row off 16-byte alignment)"""

    def __init__(self, ctx, s, pitch, dtype=f32, fill=PATTERN, lead=0, tail=8):
        self.ctx, self.s, self.pitch, self.dtype, self.lead, self.fill = ctx, s, pitch, dtype, lead, fill
        self.count = lead + s * pitch + tail
        self.host = np.full(self.count, fill, dtype)
        self.buf = None

    @classmethod
    def of(cls, ctx, x, pitch, lead=0):
        """input rows: x [s, n] with SENTINEL in the padding"""
        x = np.atleast_2d(x)
        r = cls(ctx, x.shape[0], pitch, x.dtype.type, SENTINEL * (1 + 1j) if x.dtype == c64 else SENTINEL, lead)
        r.host[lead:lead + r.s * pitch].reshape(r.s, pitch)[:, :x.shape[1]] = x
        return r.up()

    def up(self):
        self.buf = self.ctx.upload(self.host)
        return self

    def at(self, col=0):
        return self.buf.at(self.host.itemsize * (self.lead + col))

    def get(self, n, col=0):
        """columns col .. col + n of every row; everything outside columns 0 .. col + n must still hold the fill"""
        full = self.ctx.download(self.buf, self.dtype, self.count)
        body = full[self.lead:self.lead + self.s * self.pitch].reshape(self.s, self.pitch)
        keep = np.concatenate([full[:self.lead], body[:, col + n:].ravel(), full[self.lead + self.s * self.pitch:]])
        assert np.all(keep.view(np.uint32) == np.array([self.fill], self.dtype).view(np.uint32)[0]), "padding behind n / between rows was written"
        return body[:, col:col + n].copy()


def _state(ctx, v):
    return ctx.upload(np.ascontiguousarray(v))


# ================================================================== agc_ff: bits of the oracle, outputs and last_gain_io
def _agc(ctx, x, block, p, gains, calls):
    s, n = x.shape
    di = Rows.of(ctx, x, n + 5); do = Rows(ctx, s, n + 3).up(); dg = _state(ctx, gains.astype(f32))
    at, paths = 0, []
    for k in calls:
        ctx.check(ctx.L.csdr_amd_agc_ff(ctx.h, di.at(at), do.at(at), s, k, block, di.pitch, do.pitch, p["reference"], p["attack_rate"], p["decay_rate"], p["max_gain"],
                                        p["hang_time"], p["attack_wait"], p["filter_alpha"], dg.ptr), "agc_ff")
        paths.append(_path(ctx)); at += k
    return do.get(n), ctx.download(dg, f32, s), paths


@pytest.mark.parametrize("pi", range(len(am.AGC_PARAMS)))
@pytest.mark.parametrize("si", range(len(am.AGC_SHAPES)), ids=["%dx%d-b%d" % sh[:3] for sh in am.AGC_SHAPES])
def test_agc_ff_bits(ctx, port, si, pi):
    s, n, block, want = am.AGC_SHAPES[si]
    p = am.AGC_PARAMS[pi]
    x, g0, n1 = am.agc_case(si, pi)
    assert am.agc_path(s, n) == want
    for calls in ([n], [n1, n - n1]):                                # one call; two calls with the gain carried, the first not a multiple of block
        y, g, paths = _agc(ctx, x, block, p, g0, calls)
        assert paths == ([want] if len(calls) == 1 else [am.agc_path(s, k) for k in calls]), paths
        for r in range(s):
            at, gain, ys = 0, g0[r], []
            for k in calls:
                yr, gain = am.port_agc(port, x[r, at:at + k], block, p, gain); ys.append(yr); at += k
            am.assert_bits(y[r], np.concatenate(ys), "%s stream %d calls %r" % (paths, r, calls))
            am.assert_bits(g[r:r + 1], [gain], "%s stream %d last_gain" % (paths, r))
    _report("agc_ff", want, "%dx%d block %d params %d" % (s, n, block, pi), "bits")


# ================================================================== deemphasis_wfm_ff: bits of the oracle, outputs and last_io
def _deemph(ctx, x, tau, fs, last, in_place=False):
    s, n = x.shape
    di = Rows.of(ctx, x, n + 7); dl = _state(ctx, np.asarray(last, f32))
    do = di if in_place else Rows(ctx, s, n + 3).up()
    ctx.check(ctx.L.csdr_amd_deemphasis_wfm_ff(ctx.h, di.at(), do.at(), s, n, di.pitch, do.pitch, tau, int(fs), dl.ptr), "deemphasis_wfm_ff")
    path = _path(ctx)
    if in_place:
        full = ctx.download(di.buf, f32, di.count)[:s * di.pitch].reshape(s, di.pitch)
        assert np.all(full[:, n:] == f32(SENTINEL))
        return full[:, :n].copy(), ctx.download(dl, f32, s), path
    return do.get(n), ctx.download(dl, f32, s), path


def _deemph_check(port, x, tau, fs, last, y, lo, what):
    for r in range(x.shape[0]):
        w, wl = port.deemphasis_wfm_ff(x[r], tau, fs, float(last[r]))
        am.assert_bits(y[r], w, "%s stream %d" % (what, r))
        am.assert_bits(lo[r:r + 1], [wl], "%s stream %d last_io" % (what, r))


@pytest.mark.parametrize("s,n", am.DEEMPH_SHAPES, ids=["%dx%d" % sh for sh in am.DEEMPH_SHAPES])
def test_deemphasis_wfm_switch_points(ctx, port, s, n):
    """31 / 32 streams, n = 2047 / 2048 / 2049, the 64-chunk wave edge (16384 samples), a ragged tile of the serial kernel; carried states 0.37, NaN, 1e-40"""
    rng = np.random.default_rng(s * 100003 + n)
    x = rng.uniform(-1, 1, (s, n)).astype(f32)
    last = np.array([am.DEEMPH_STATES[r % 3] for r in range(s)], f32)
    want = "k_deemph_wfm_spec<1>" if s < 32 and n >= 2048 else "k_deemph_wfm"
    assert am.deemph_path(50e-6, 48000, s, n) == want
    y, lo, path = _deemph(ctx, x, 50e-6, 48000, last)
    assert path == want
    _deemph_check(port, x, 50e-6, 48000, last, y, lo, path)
    _report("deemphasis_wfm_ff", path, "%dx%d" % (s, n), "bits")


@pytest.mark.parametrize("tau,fs,M", am.DEEMPH_TAUS, ids=["M%d" % t[2] for t in am.DEEMPH_TAUS])
def test_deemphasis_wfm_run_in_lengths(ctx, port, tau, fs, M):
    rng = np.random.default_rng(fs + M)
    x = rng.uniform(-1, 1, (2, 4500)).astype(f32)
    last = np.array([0.37, np.nan], f32)
    y, lo, path = _deemph(ctx, x, tau, fs, last)
    assert path == ("k_deemph_wfm_spec<%d>" % M if M else "k_deemph_wfm") == am.deemph_path(tau, fs, 2, 4500)
    _deemph_check(port, x, tau, fs, last, y, lo, path)
    _report("deemphasis_wfm_ff", path, "tau %g fs %d" % (tau, fs), "bits")


def test_deemphasis_wfm_in_place(ctx, port):
    x = np.random.default_rng(5).uniform(-1, 1, (1, 5000)).astype(f32)
    assert am.deemph_path(50e-6, 48000, 1, 5000, in_place=True) == "k_deemph_wfm"
    y, lo, path = _deemph(ctx, x, 50e-6, 48000, [0.37], in_place=True)
    assert path == "k_deemph_wfm"
    _deemph_check(port, x, 50e-6, 48000, [0.37], y, lo, "in place")


@pytest.mark.parametrize("ci", range(len(am.DEEMPH_DENORMAL)))
def test_deemphasis_wfm_denormals(ctx, ci):
    """inputs at 1e-38: every product and state is subnormal (the expected bits were computed before anything could switch the process to flush-to-zero)"""
    assert am.DENORMALS_LIVE
    tau, fs, x, last, want = am.DEEMPH_DENORMAL[ci]
    y, lo, path = _deemph(ctx, x, tau, fs, last)
    assert path == am.deemph_path(tau, fs, *x.shape)
    am.assert_bits(y, want, path)
    am.assert_bits(lo, want[:, -1], path + " last_io")
    assert np.count_nonzero(want) > want.size // 2


@pytest.mark.parametrize("tau,fs,M", [t for t in am.DEEMPH_TAUS if t[2] in (1, 2, 8)], ids=["M1", "M2", "M8"])
@pytest.mark.parametrize("kind", ["1e30", "nan", "inf"])
def test_deemphasis_wfm_repair(ctx, port, kind, tau, fs, M):
    """a sample the run-in cannot forget: chunks arrive with the wrong state and k_deemph_wfm_check / k_deemph_wfm_fix have to redo them"""
    rng = np.random.default_rng(M)
    x = np.stack([am.deemph_repair_input(rng, 6000, kind) for _ in range(2)])
    last = np.array([0.0, 0.37], f32)
    alpha = am.deemph_alpha(tau, fs)
    counts = [am.deemph_spec_mismatches(x[r], alpha, M, last[r]) for r in range(2)]
    assert min(counts) > 0, counts
    y, lo, path = _deemph(ctx, x, tau, fs, last)
    assert path == "k_deemph_wfm_spec<%d>" % M
    _deemph_check(port, x, tau, fs, last, y, lo, path + " repair " + kind)
    _report("deemphasis_wfm_ff repair", path, kind, "chunks redone (model) %r" % counts, "bits")


# ================================================================== fastagc_ff: bits of the oracle
def _fastagc(ctx, x, block, calls, state, reference=1.0, lead=0, odd_pitch=False):
    s, n = x.shape
    pitch = n + 4 + (-n % 4) + (1 if odd_pitch else 0)           # a multiple of 4 floats (every row 16-byte aligned), or odd
    di = Rows.of(ctx, x, pitch, lead); do = Rows(ctx, s, pitch, lead=lead).up(); ds = _state(ctx, state)
    b = 0
    for k in calls:
        ctx.check(ctx.L.csdr_amd_fastagc_ff(ctx.h, di.at(b * block), do.at(b * block), s, k, block, pitch, pitch, reference, ds.ptr), "fastagc_ff"); b += k
    return do.get(n), ctx.download(ds, f32, state.size).reshape(state.shape)


def _fastagc_check(ctx, port, s, block, calls, zero_state, lead=0, odd_pitch=False, what=""):
    nb = sum(calls)
    x = am.fastagc_input(s, block, nb, block * 7 + nb)
    st = am.fastagc_state(s, block, zero_state, block)
    y, st_out = _fastagc(ctx, x, block, calls, st, lead=lead, odd_pitch=odd_pitch)
    for r in range(s):
        w, ws = am.port_fastagc(port, x[r], block, 1.0, st[r])
        am.assert_bits(y[r], w, "fastagc_ff %s block %d calls %r stream %d" % (what, block, calls, r))
        am.assert_bits(st_out[r, :2 * block + 3], ws[:2 * block + 3], "fastagc_ff %s block %d stream %d state" % (what, block, r))
    if zero_state:
        assert np.all(y[:, :block] == 0) and np.all(x[:, :block] == 0)


@pytest.mark.parametrize("s,block,calls", am.FASTAGC_CASES, ids=["%dx-b%d-%d" % (c[0], c[1], len(c[2])) for c in am.FASTAGC_CASES])
def test_fastagc_ff_bits(ctx, port, s, block, calls):
    """block % 4 == 0 on aligned rows: the float4 path; every other block: the scalar one.  Zero state (a silent first block: peak 0, gain capped at 50) and a
    live one."""
    for zero in (True, False):
        _fastagc_check(ctx, port, s, block, calls, zero)
    _report("fastagc_ff", "block %d streams %d calls %r" % (block, s, calls), "bits")


@pytest.mark.parametrize("block", [1024, 1000])
def test_fastagc_ff_unaligned_rows(ctx, port, block):
    """block % 4 == 0, but the input pointer is 4 bytes off 16-byte alignment / the pitch is odd: the scalar path"""
    _fastagc_check(ctx, port, 3, block, [3, 1, 2], True, lead=1, what="lead 4 bytes")
    _fastagc_check(ctx, port, 3, block, [3, 1, 2], False, odd_pitch=True, what="odd pitch")


# ================================================================== fractional_decimator_ff: bits of the oracle, count, input_processed, where
def _fracdec_call(ctx, d, x, n_out_max):
    s, n = x.shape
    di = Rows.of(ctx, x, n + 9); do = Rows(ctx, s, n_out_max + 5).up()
    proc = C.c_int(-12345)
    no = ctx.check(ctx.L.csdr_amd_fractional_decimator_ff(ctx.h, d, di.at(), do.at(), s, n, di.pitch, do.pitch, C.byref(proc)), "fractional_decimator_ff")
    path = _path(ctx)
    ctx.sync()
    return do.get(no), proc.value, path


@pytest.mark.parametrize("rate,P,T,bufsize,cls", am.FRACDEC_CASES, ids=["r%g-P%d-T%d-w%d" % c[:4] for c in am.FRACDEC_CASES])
def test_fractional_decimator_ff_bits(ctx, port, rate, P, T, bufsize, cls):
    taps = am.asym_taps(T, 900 + P) if T else None
    rng = np.random.default_rng(int(rate * 1000) + P)
    x = rng.uniform(-1, 1, (3, 3 * max(am.FRACDEC_CALLS) + 100)).astype(f32)
    d = ctx.L.csdr_amd_fracdec_create(rate, P, None if taps is None else taps.ctypes.data_as(C.c_void_p), T)
    assert d
    try:
        if bufsize:
            ctx.L.csdr_amd_fracdec_set_cli_bufsize(d, bufsize)
        model = am.FracdecPath(rate, P, T, bufsize)
        orc = [am.PortFracdec(port, rate, P, taps, bufsize) for _ in range(3)]
        base, paths, w2 = 0, [], None
        for call, n in enumerate(am.FRACDEC_CALLS + am.FRACDEC_CALLS[1:]):
            if call == 2:                                            # the third call: the second's size from the second's `where` -> the cached plan
                ctx.L.csdr_amd_fracdec_set_where(d, w2)
                for o in orc:
                    o.where = w2
            w_before = ctx.L.csdr_amd_fracdec_get_where(d)
            assert w_before == orc[0].where
            if call == 1:
                w2 = w_before
            want_path = model.path(w_before, n)
            y, proc, path = _fracdec_call(ctx, d, x[:, base:base + n], n)
            assert path == want_path, (call, path, want_path)
            paths.append(path)
            for r in range(3):
                w, wp = orc[r].call(x[r, base:base + n])
                assert y.shape[1] == w.size and proc == wp, (call, y.shape, w.size, proc, wp)
                am.assert_bits(y[r], w, "rate %g P %d call %d stream %d (%s)" % (rate, P, call, r, path))
            assert ctx.L.csdr_amd_fracdec_get_where(d) == orc[0].where
            base += proc
        assert paths[0] == "fracdec:" + cls and paths[2] == "fracdec:cached", paths
    finally:
        ctx.L.csdr_amd_fracdec_destroy(d)
    _report("fractional_decimator_ff", "rate %g P %d taps %d window %d" % (rate, P, T, bufsize), " ".join(paths), "bits")


@pytest.mark.parametrize("P,T", [(2, 0), (12, 0), (4, 33)])
def test_fractional_decimator_ff_shortest_inputs(ctx, port, P, T):
    """inputs of P + taps samples (no output) and P + taps + 1 (one output for P = 2, else none)"""
    taps = am.asym_taps(T, 5) if T else None
    x = np.random.default_rng(P).uniform(-1, 1, (3, P + T + 1)).astype(f32)
    for n in (P + T, P + T + 1):
        d = ctx.L.csdr_amd_fracdec_create(2.5, P, None if taps is None else taps.ctypes.data_as(C.c_void_p), T)
        try:
            y, proc, _ = _fracdec_call(ctx, d, x[:, :n], 4)
            o = am.PortFracdec(port, 2.5, P, taps)
            w, wp = o.call(x[0, :n])
            assert y.shape[1] == w.size == (1 if P == 2 and n == P + T + 1 else 0) and proc == wp
            assert ctx.L.csdr_amd_fracdec_get_where(d) == o.where
            for r in range(3):
                am.assert_bits(y[r], am.PortFracdec(port, 2.5, P, taps).call(x[r, :n])[0], "shortest input")
        finally:
            ctx.L.csdr_amd_fracdec_destroy(d)


# ================================================================== dcblock_ff: per-sample gate against float64
def _dcblock(ctx, x, a, state, calls):
    s, n = x.shape
    di = Rows.of(ctx, x, n + 5); do = Rows(ctx, s, n + 3).up(); ds = _state(ctx, np.asarray(state, f32))
    at = 0
    for k in calls:
        ctx.check(ctx.L.csdr_amd_dcblock_ff(ctx.h, di.at(at), do.at(at), s, k, di.pitch, do.pitch, a, ds.ptr), "dcblock_ff"); at += k
    return do.get(n), ctx.download(ds, f32, 2 * s).reshape(s, 2)


@pytest.mark.parametrize("ci", range(len(am.DC_CASES)), ids=["%dx%d-a%g" % c for c in am.DC_CASES])
def test_dcblock_ff_gate(ctx, ci):
    s, n, a = am.DC_CASES[ci]
    x, y64, B, st64 = am.dc_case(ci)
    y, st = _dcblock(ctx, x, a, np.zeros((s, 2)), [n])
    k = am.KAPPA["dcblock_ff"]
    g = am.gate_ratio(y, y64, B, k)
    gs = am.gate_ratio(st[:, 1], st64[1], B[:, -1], k)
    _report("dcblock_ff", "%dx%d a %g" % (s, n, a), "%.4f state %.4f" % (g, gs))
    assert g <= 1.0 and gs <= 1.0, "error %.3g x the gate (state %.3g)" % (g, gs)
    assert np.array_equal(st[:, 0], x[:, -1])


def test_dcblock_ff_three_calls(ctx):
    """calls of 33, 1 and 4000 samples with the state carried = one run over 4034"""
    calls = [33, 1, 4000]
    x = am.dc_input(3, sum(calls), 99)
    st0 = np.array([[0.5, -0.25], [100.0, 3.0], [0.0, 0.0]], f32)
    y64, B, st64, _ = am.dcblock_f64(x, 0.95, (st0[:, 0], st0[:, 1]))
    y, st = _dcblock(ctx, x, 0.95, st0, calls)
    k = am.KAPPA["dcblock_ff"]
    g = am.gate_ratio(y, y64, B, k); gs = am.gate_ratio(st[:, 1], st64[1], B[:, -1], k)
    _report("dcblock_ff", "three calls", "%.4f state %.4f" % (g, gs))
    assert g <= 1.0 and gs <= 1.0 and np.array_equal(st[:, 0], x[:, -1])


# ================================================================== fastdcblock_ff: per-sample gate against float64
@pytest.mark.parametrize("s,block,calls", am.FASTDC_CASES, ids=["%dx-b%d-%d" % (c[0], c[1], len(c[2])) for c in am.FASTDC_CASES])
def test_fastdcblock_ff_gate(ctx, s, block, calls):
    nb = sum(calls)
    x = am.dc_input(s, nb * block, 300 + block)
    last = np.array([0.1 * (r % 5) for r in range(s)], f32)
    pitch = nb * block + 3
    di = Rows.of(ctx, x, pitch); do = Rows(ctx, s, pitch).up(); dl = _state(ctx, last)
    b = 0
    for k in calls:
        ctx.check(ctx.L.csdr_amd_fastdcblock_ff(ctx.h, di.at(b * block), do.at(b * block), s, k, block, pitch, pitch, dl.ptr), "fastdcblock_ff"); b += k
    y = do.get(nb * block); lo = ctx.download(dl, f32, s)
    y64, S, l64 = am.fastdcblock_f64(x, block, last)
    k = am.KAPPA["fastdcblock_ff"]
    g = am.gate_ratio(y, y64, S, k); gl = am.gate_ratio(lo, l64, S[:, -1], k)
    _report("fastdcblock_ff", "%d streams block %d calls %r" % (s, block, calls), "%.4f level %.4f" % (g, gl))
    assert g <= 1.0 and gl <= 1.0, (g, gl)


# ================================================================== fmdemod_quadri_cf: ulp gate against the reference's value
def _fmdemod(ctx, x, last, calls):
    s, n = x.shape
    di = Rows.of(ctx, x, n + 3); do = Rows(ctx, s, n + 5).up(); dl = _state(ctx, np.asarray(last, c64))
    at = 0
    for k in calls:
        ctx.check(ctx.L.csdr_amd_fmdemod_quadri_cf(ctx.h, di.at(at), do.at(at), s, k, di.pitch, do.pitch, dl.ptr), "fmdemod_quadri_cf"); at += k
    return do.get(n), ctx.download(dl, c64, s)


@pytest.mark.parametrize("s,n,calls", am.FM_CASES, ids=["%dx%d-%dcalls" % (c[0], c[1], len(c[2])) for c in am.FM_CASES])
def test_fmdemod_quadri_cf_ulp_gate(ctx, s, n, calls):
    """|x| ~ 0.7 with exact-zero samples planted; 262145 samples are past the 1024-block grid cap; `last` carried over three calls"""
    x, last, zeros = am.fm_case(s, n)
    y, lo = _fmdemod(ctx, x, last, calls)
    am.assert_bits(lo.view(f32), x[:, -1].copy().view(f32), "last_io")
    worst = 0.0
    for r in range(s):
        gate = am.fmdemod_quadri_ulp_bound(x[r], last[r])
        d, n_abs = am.fmdemod_quadri_check(y[r], x[r], last[r], gate)
        # compared absolutely: the planted zeros and the sample behind each (x (x - 0) has an exactly zero cross product); stream with last = 0: also sample 0
        expect = len(set(zeros) | {k + 1 for k in zeros if k + 1 < n})
        assert n_abs == expect, (r, n_abs, expect)
        assert d <= gate, "stream %d: %.2f ulp, gate %.2f" % (r, d, gate)
        worst = max(worst, d / gate)
    _report("fmdemod_quadri_cf", "%dx%d calls %r" % (s, n, calls), "%.4f" % worst)


def test_fmdemod_quadri_cf_magnitude_sweep(ctx):
    """|x| = 2^k, k = -70 .. 60: a subnormal power (k < -63) and one whose reciprocal is subnormal; wherever the reference is finite the result must be finite
    and inside the gate"""
    assert am.DENORMALS_LIVE
    x = am.FM_SWEEP_X[None, :]
    y, _ = _fmdemod(ctx, x, [am.FM_SWEEP_LAST], [x.shape[1]])
    ref = am.FM_SWEEP_REF
    fin = np.isfinite(ref)
    assert fin.sum() >= ref.size - 3 and np.all(np.abs(ref[fin]) >= np.finfo(f32).tiny)
    bad = np.nonzero(fin & ~np.isfinite(y[0]))[0]
    assert bad.size == 0, "non-finite output at |x| = 2^%d (%d samples) where the reference gives %r" % (am.FM_SWEEP_K[bad[0]], bad.size, ref[bad[0]])
    am.assert_bits(np.where(fin, 0, y[0]), np.where(fin, 0, ref), "inf positions")
    gate = am.fmdemod_quadri_ulp_bound(am.FM_SWEEP_X, am.FM_SWEEP_LAST)
    d = np.abs(y[0, fin].astype(f64) - ref[fin].astype(f64)) / am.ulp_of(ref[fin])
    _report("fmdemod_quadri_cf", "magnitude sweep", "%.4f" % (d.max() / gate), "worst at |x| = 2^%d" % am.FM_SWEEP_K[fin][np.argmax(d)])
    assert d.max() <= gate, "%.3g ulp at |x| = 2^%d, gate %.2f" % (d.max(), am.FM_SWEEP_K[fin][np.argmax(d)], gate)


# ================================================================== fmdemod_atan_cf: absolute gate against float64
@pytest.mark.parametrize("n,calls", am.ATAN_CASES, ids=["%d-%dcalls" % (c[0], len(c[1])) for c in am.ATAN_CASES])
def test_fmdemod_atan_cf_gate(ctx, n, calls):
    x, last = am.atan_case(n)
    di = Rows.of(ctx, x, n + 3); do = Rows(ctx, 3, n + 5).up(); dl = _state(ctx, last)
    at = 0
    for k in calls:
        ctx.check(ctx.L.csdr_amd_fmdemod_atan_cf(ctx.h, di.at(at), do.at(at), 3, k, di.pitch, do.pitch, dl.ptr), "fmdemod_atan_cf"); at += k
    y = do.get(n); lo = ctx.download(dl, f32, 3)
    worst = 0.0
    for r in range(3):
        w, S, ph = am.fmdemod_atan_f64(x[r], last[r])
        worst = max(worst, am.gate_ratio(y[r], w, S, am.KAPPA["fmdemod_atan_cf"]), abs(float(lo[r]) - ph) / (am.KAPPA["fmdemod_atan_cf"] * am.U * np.pi))
    _report("fmdemod_atan_cf", "3x%d calls %r" % (n, calls), "%.4f" % worst)
    assert worst <= 1.0


# ================================================================== the flat element-wise blocks, one length past each grid cap
N_FLAT_F, N_FLAT_C = am.N_FLAT_F, am.N_FLAT_C


def _flat(ctx, fn, x, n, *extra):
    """flat arrays: SENTINEL behind the input's n elements, the pattern behind the output's"""
    di = Rows.of(ctx, x[None, :n], n + 8); do = Rows(ctx, 1, n + 8).up()
    ctx.check(fn(ctx.h, di.at(), do.at(), n, *extra), fn.__name__)
    return do.get(n)[0]


def test_limit_and_gain_ff_bits(ctx, port):
    x = am.flat_f_input()
    for n in (N_FLAT_F, 7, 3):
        am.assert_bits(_flat(ctx, ctx.L.csdr_amd_limit_ff, x[-n:] if n < 10 else x, n, 1.0), port.limit_ff(x[-n:] if n < 10 else x[:n], 1.0), "limit_ff n=%d" % n)
        am.assert_bits(_flat(ctx, ctx.L.csdr_amd_gain_ff, x[-n:] if n < 10 else x, n, 0.37), port.gain_ff(x[-n:] if n < 10 else x[:n], 0.37), "gain_ff n=%d" % n)


def test_amdemod_and_logpower_cf_gate(ctx):
    x = am.flat_c_input()
    y = _flat(ctx, ctx.L.csdr_amd_amdemod_cf, x, N_FLAT_C)
    w, S = am.amdemod_f64(x)
    ga = am.gate_ratio(y, w, S, am.KAPPA["amdemod_cf"])
    y = _flat(ctx, ctx.L.csdr_amd_logpower_cf, x, N_FLAT_C, -70.0)
    w, S = am.logpower_f64(x, -70.0)
    gl = am.gate_ratio(y, w, S, am.KAPPA["logpower_cf"])
    _report("amdemod_cf", "n=%d" % N_FLAT_C, "%.4f" % ga)
    _report("logpower_cf", "n=%d" % N_FLAT_C, "%.4f" % gl)
    assert ga <= 1.0 and gl <= 1.0, (ga, gl)
