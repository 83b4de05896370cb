"""The pulse-shaped receive object on the GPU: both kernels against the float32 model (pulserx_model.py) bit for bit at every shape of the CPU tests and at
the ring limit, every `lanes` choice, cut and batch invariance, per-channel reset and state, a correction of a whole half symbol, output bounds, argument
errors, lifecycle, `csdr chain` with the fused run against the compiled reference's pipeline, and the loop back through the transmit object."""
import functools
import os
import subprocess

import numpy as np
import pytest

import pulse_model as pm
import pulserx_model as rm
import test_pulserx_cpu as tc
from test_pulserx_cpu import u32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CSDR = os.path.join(ROOT, "oracle", "_ref", "csdr")
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
TILED, GENERIC = "k_pulserx_tiled", "k_pulserx_generic"
CHANNELS = [1, 3, 65]
LANES = [1, 2, 4, 8, 16]
# the ring of k_pulserx_tiled is the next power of two >= 3 D/2 + T - 1 + 128 samples and 4096 of them (32 KiB) is the most that fits 63 KiB beside the
# taps: the largest taps count at D = 8 and at D = 2048 that still fits, and one more
LIMIT_SHAPES = [((8, 3957), TILED), ((8, 3958), GENERIC), ((2048, 897), TILED), ((2048, 898), GENERIC)]
CONFIGS = [(rm.GARDNER, 1), (rm.EARLYLATE, 0)]


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def kernel_of(shape, forced=False):
    D, T = shape
    return TILED if not forced and 3 * (D // 2) + T - 1 + 128 <= 4096 else GENERIC


def lanes_of(shape, want, sliced=False):
    """channels per wave of k_pulserx_tiled: 16, 8, 4, 2 or 1 as asked for, the next smaller one while ring, taps and byte staging do not fit 63 KiB"""
    D, T = shape
    R = 256
    while R < 3 * (D // 2) + T - 1 + 128:
        R *= 2
    C = 16 if want >= 16 else 8 if want >= 8 else 4 if want >= 4 else 2 if want >= 2 else 1
    while C > 0 and 8 * C * R + 4 * ((T + 1) & ~1) + (512 * C if sliced else 0) > 63 * 1024:
        C //= 2
    return C


MODEL_ROWS = (0, 1, 64)


def walked(x, params, first):
    """every channel through the CPU walk (the kernels' step functions, bit-equal to the model by test_pulserx_cpu): the expected outputs of a batch"""
    import csdr_amd
    out = []
    for row in x:
        st = csdr_amd.PulseRxChan()
        y, e, i = csdr_amd.pulserx_debug_walk(params, first, "timing", row, state=st, with_extras=True)
        out.append(dict(sym=y, err=e, idx=i, state=(st.tail_len, st.correction_offset, st.base)))
    return out


@functools.lru_cache(maxsize=None)
def case(shape, alg, q, first="filter", channels=65):
    """one case's input and the expected outputs of every channel, computed once and left unchanged: the numpy model on the rows MODEL_ROWS (the batch's
    first two channels and its last), the CPU walk on all of them, the two equal by bits where both exist"""
    import csdr_amd
    taps = tc.taps_of(shape)
    x = tc.case_signal(shape, alg, q, 4, n_channels=channels, seed=3)
    if first == "timing":
        x = tc.filtered32(x, taps)
    rows = [r for r in MODEL_ROWS if r < channels]
    models = rm.receive(x[rows], taps, first=rm.FILTER if first == "filter" else rm.TIMING, last=rm.TIMING, **tc.model_kw(shape, alg, q))
    want = walked(x, csdr_amd.pulserx_params(taps, alg, shape[0], tc.LOOP_GAIN, tc.MAX_ERROR, q), first)
    for r, m in zip(rows, models):
        assert np.array_equal(u32(want[r]["sym"]), u32(m["sym"])) and np.array_equal(u32(want[r]["err"]), u32(m["err"]))
        assert np.array_equal(want[r]["idx"], m["idx"]) and want[r]["state"] == m["state"]
        assert np.mean(m["corr"] != 0) >= 0.01 or not tc.can_correct(shape, alg)
    x.setflags(write=False)
    return dict(x=x, taps=taps, models=want, gain=1.0 / tc.rms_of(shape, alg, q))


@functools.lru_cache(maxsize=None)
def limit_case(shape, channels=3):
    """noise through asymmetric taps at a ring-limit shape, a few symbols long, scaled so that the loop corrects"""
    D, T = shape
    rng = np.random.default_rng(D + T)
    taps = (rng.uniform(-1, 1, T) * np.linspace(1.0, 0.25, T) / np.sqrt(T / 3)).astype(np.float32)
    n = T + 3 * D // 2 + 40 * D
    x = (1.2 * (rng.standard_normal((channels, n)) + 1j * rng.standard_normal((channels, n)))).astype(np.complex64)
    models = rm.receive(x, taps, first=rm.FILTER, last=rm.TIMING, decimation=D, algorithm=rm.GARDNER, use_q=True, loop_gain=0.5, max_error=2.0)
    x.setflags(write=False)
    return dict(x=x, taps=taps, models=models)


def want_bytes(model, gain, slice_q, n_symbols):
    soft = (np.float32(gain) * (model["sym"].view(np.float32) if slice_q else np.ascontiguousarray(model["sym"].real))).astype(np.float32)
    return pm.slicer(soft, n_symbols)


def assert_timing(res, models, tag):
    for ch, ((y, e, i), m) in enumerate(zip(res, models)):
        assert y.size == m["sym"].size, (tag, ch, y.size, m["sym"].size)
        assert np.array_equal(u32(y), u32(m["sym"])), (tag, ch, "symbols")
        assert np.array_equal(u32(e), u32(m["err"])), (tag, ch, "errors")
        assert np.array_equal(i, m["idx"]), (tag, ch, "indexes")


def assert_state(o, models, tag):
    for ch in sorted({0, len(models) - 1}):
        st = o.get_channel(ch)
        assert (st.tail_len, st.correction_offset, st.base) == models[ch]["state"], (tag, ch)


# ------------------------------------------------------------------ 1. both kernels against the model
@pytest.mark.parametrize("alg,q", CONFIGS)
@pytest.mark.parametrize("shape", tc.SHAPES)
def test_kernels_equal_model(ctx, shape, alg, q):
    _kernels_equal_model(ctx, shape, alg, q)


@pytest.mark.parametrize("alg,q", [(rm.GARDNER, 0), (rm.EARLYLATE, 1)])
def test_kernels_equal_model_other_loop_variants(ctx, alg, q):
    """the two combinations of algorithm and Q that CONFIGS leaves out, at one shape"""
    _kernels_equal_model(ctx, (8, 65), alg, q)


def _kernels_equal_model(ctx, shape, alg, q):
    import csdr_amd
    m = case(shape, alg, q)
    p = csdr_amd.pulserx_params(m["taps"], alg, shape[0], tc.LOOP_GAIN, tc.MAX_ERROR, q)
    for ch in CHANNELS:
        with ctx.pulse_rx(p, ch, "filter", "timing") as o:
            for lanes, forced in [(l, False) for l in LANES] + [(0, True)]:
                o.reset(); o.set_lanes(lanes); o.force_generic(forced)
                res = o.process(m["x"][:ch], with_extras=True)
                assert o.kernel_name() == kernel_of(shape, forced), (ch, lanes, forced)
                if not forced:
                    assert o.lanes() == lanes_of(shape, lanes)
                assert_timing(res, m["models"][:ch], (ch, lanes, forced))
                assert_state(o, m["models"][:ch], (ch, lanes, forced))
    # the sliced outputs, both byte layouts, on the widest batch
    for sq, ns in ((1, 4), (0, 2), (0, 3)):
        ps = csdr_amd.pulserx_params(m["taps"], alg, shape[0], tc.LOOP_GAIN, tc.MAX_ERROR, q, m["gain"], ns, sq)
        with ctx.pulse_rx(ps, 65, "filter", "slice") as o:
            for lanes, forced in ((0, False), (16, False), (0, True)):
                o.reset(); o.set_lanes(lanes); o.force_generic(forced)
                res = o.process(m["x"])
                assert o.kernel_name() == kernel_of(shape, forced)
                for ch in range(65):
                    want = want_bytes(m["models"][ch], m["gain"], sq, ns)
                    assert res[ch].dtype == np.uint8 and res[ch].size == want.size and np.array_equal(res[ch], want), (sq, ns, lanes, forced, ch)


@pytest.mark.parametrize("alg,q", CONFIGS)
@pytest.mark.parametrize("shape", [(8, 65), (2, 7), (256, 513)])
def test_from_timing_on(ctx, shape, alg, q):
    """first_stage TIMING: the input is the stream the loop reads, its bits kept"""
    import csdr_amd
    m = case(shape, alg, q, "timing", 5)
    p = csdr_amd.pulserx_params(None, alg, shape[0], tc.LOOP_GAIN, tc.MAX_ERROR, q, m["gain"], 4, 1)
    for forced in (False, True):
        with ctx.pulse_rx(p, 5, "timing", "timing") as o:
            o.force_generic(forced)
            assert_timing(o.process(m["x"], with_extras=True), m["models"], forced)
            assert o.kernel_name() == (GENERIC if forced else TILED)
        with ctx.pulse_rx(p, 5, "timing", "slice") as o:
            o.force_generic(forced)
            res = o.process(m["x"])
            for ch in range(5):
                assert np.array_equal(res[ch], want_bytes(m["models"][ch], m["gain"], 1, 4)), (forced, ch)


@pytest.mark.parametrize("shape,kernel", LIMIT_SHAPES)
def test_ring_limit(ctx, shape, kernel):
    import csdr_amd
    m = limit_case(shape)
    assert kernel_of(shape) == kernel
    assert min(np.count_nonzero(c["corr"]) for c in m["models"]) > 0
    p = csdr_amd.pulserx_params(m["taps"], 0, shape[0], 0.5, 2.0, 1)
    with ctx.pulse_rx(p, 3, "filter", "timing") as o:
        for forced in (False, True):
            o.reset(); o.force_generic(forced)
            res = o.process(m["x"], calls=[m["x"].shape[1] // 2, m["x"].shape[1] - m["x"].shape[1] // 2], with_extras=True)
            assert o.kernel_name() == (GENERIC if forced else kernel)
            assert_timing(res, m["models"], forced)
            assert_state(o, m["models"], forced)


# ------------------------------------------------------------------ 2. cuts, batch position, per-channel state
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("shape", [(8, 65), (16, 129), (2, 7)])
def test_cut_invariance(ctx, shape, forced):
    import csdr_amd
    alg, q = rm.GARDNER, 1
    m = case(shape, alg, q)
    n = m["x"].shape[1]
    cuts = list(tc.cuts_of(shape))
    calls = cuts + [n - sum(cuts)]
    p = csdr_amd.pulserx_params(m["taps"], alg, shape[0], tc.LOOP_GAIN, tc.MAX_ERROR, q, m["gain"], 4, 1)
    with ctx.pulse_rx(p, 65, "filter", "timing") as o:
        o.force_generic(forced)
        assert_timing(o.process(m["x"], calls=calls, with_extras=True), m["models"], "cuts")
        assert_state(o, m["models"], "cuts")
        assert o.kernel_name() == kernel_of(shape, forced)
    with ctx.pulse_rx(p, 65, "filter", "slice") as o:
        o.force_generic(forced)
        res = o.process(m["x"], calls=calls + [0])
        for ch in (0, 1, 37, 64):
            assert np.array_equal(res[ch], want_bytes(m["models"][ch], m["gain"], 1, 4)), ch
    with ctx.pulse_rx(p, 1, "filter", "timing") as o:                      # channel 64 of the batch, alone
        o.force_generic(forced)
        assert_timing([o.process(m["x"][64], with_extras=True)], m["models"][64:], "alone")


@pytest.mark.parametrize("forced", [False, True])
def test_reset_channel_and_state_round_trip(ctx, forced):
    import csdr_amd
    shape, alg, q = (8, 65), rm.GARDNER, 1
    m = case(shape, alg, q)
    x = m["x"][:5]; n = x.shape[1]; h = n // 2 + 3
    p = csdr_amd.pulserx_params(m["taps"], alg, shape[0], tc.LOOP_GAIN, tc.MAX_ERROR, q)
    second = rm.receive(x[:, h:], m["taps"], first=rm.FILTER, last=rm.TIMING, **tc.model_kw(shape, alg, q))
    with ctx.pulse_rx(p, 5, "filter", "timing") as o:
        o.force_generic(forced)
        a = o.process(x[:, :h], with_extras=True)
        o.reset_channel(1)
        st = o.get_channel(2)
        assert st.tail_len > 0 and st.base + st.tail_len == h
        o.set_channel(2, st)                                               # a round trip mid-stream changes nothing
        st3 = o.get_channel(3)
        st3.base += 1000                                                   # the indexes of channel 3 move with its base, nothing else does
        o.set_channel(3, st3)
        b = o.process(x[:, h:], with_extras=True)
        for ch in (0, 2, 3, 4):
            whole = m["models"][ch]
            y = np.concatenate([a[ch][0], b[ch][0]]); e = np.concatenate([a[ch][1], b[ch][1]]); i = np.concatenate([a[ch][2], b[ch][2]])
            assert np.array_equal(u32(y), u32(whole["sym"])) and np.array_equal(u32(e), u32(whole["err"])), ch
            shift = np.where(np.arange(i.size) >= a[ch][2].size, 1000 if ch == 3 else 0, 0)
            assert np.array_equal(i, (whole["idx"].astype(np.int64) + shift).astype(np.uint32)), ch
        assert_timing([b[1]], [second[1]], "the reset channel starts a new stream")
        with pytest.raises(csdr_amd.CsdrAmdError):
            bad = o.get_channel(0); bad.tail_len = 3 * 4 + 65; o.set_channel(0, bad)
        with pytest.raises(csdr_amd.CsdrAmdError):
            o.get_channel(5)


# ------------------------------------------------------------------ 3. a correction of half a symbol
@pytest.mark.parametrize("alg", [rm.GARDNER, rm.EARLYLATE])
def test_largest_correction(ctx, alg):
    """loop_gain max_error = 1 and an amplitude at which nearly every error clips: the correction is -D/2 or +D/2.  Under GARDNER the next symbol's left
    point then lies behind this symbol's right point; the ring and the tail still hold it."""
    import csdr_amd
    shape = (16, 129)
    taps = tc.taps_of(shape)
    x = rm.signal(4, 16, taps, 200, 5, rms=12.0, seed=9)[0]
    models = rm.receive(x, taps, first=rm.FILTER, last=rm.TIMING, decimation=16, algorithm=alg, use_q=True, loop_gain=0.5, max_error=2.0)
    for mm in models:
        step = np.diff(mm["idx"].astype(np.int64))
        assert np.count_nonzero(mm["corr"] == -8) > 10 and np.count_nonzero(mm["corr"] == 8) > 10
        if alg == rm.GARDNER:
            assert np.count_nonzero(step < 16) > 10                        # next left point (idx + step) behind this right point (idx + 16)
    p = csdr_amd.pulserx_params(taps, alg, 16, 0.5, 2.0, 1)
    with ctx.pulse_rx(p, 5, "filter", "timing") as o:
        for lanes, forced in ((1, False), (4, False), (16, False), (0, True)):
            o.reset(); o.set_lanes(lanes); o.force_generic(forced)
            assert_timing(o.process(x, calls=[1000, 7, x.shape[1] - 1007], with_extras=True), models, (lanes, forced))
            assert_state(o, models, (lanes, forced))


def test_nan_and_inf_samples(ctx):
    """an inf and a NaN sample: the symbols they reach are inf or NaN, a NaN error corrects by 0 and the loop walks on; positions, counts and state equal the
    CPU walk's, the symbols equal it by bits wherever they are numbers"""
    import csdr_amd
    shape, alg, q = (8, 65), rm.GARDNER, 1
    x = np.array(case(shape, alg, q)["x"][:3])
    x[0, 700] = np.inf; x[1, 900] = np.nan; x[2, 500] = complex(0, -np.inf); x[2, 1500] = np.nan
    taps = tc.taps_of(shape)
    p = csdr_amd.pulserx_params(taps, alg, 8, tc.LOOP_GAIN, tc.MAX_ERROR, q)
    want = walked(x, p, "filter")
    assert all(np.isnan(w["err"]).any() and np.all(np.diff(w["idx"].astype(np.int64)) >= 4) for w in want)
    with ctx.pulse_rx(p, 3, "filter", "timing") as o:
        for lanes, forced in ((1, False), (16, False), (0, True)):
            o.reset(); o.set_lanes(lanes); o.force_generic(forced)
            res = o.process(x, calls=[800, x.shape[1] - 800], with_extras=True)
            for ch, ((y, e, i), w) in enumerate(zip(res, want)):
                assert np.array_equal(i, w["idx"]), (lanes, forced, ch)
                for got, ref in ((y.view(np.float32), w["sym"].view(np.float32)), (e, w["err"])):
                    num = ~np.isnan(ref)
                    assert np.array_equal(np.isnan(got), ~num) and np.array_equal(u32(got[num]), u32(ref[num])), (lanes, forced, ch)
            assert_state(o, want, (lanes, forced))


# ------------------------------------------------------------------ 4. bounds, errors, lifecycle
def test_max_out_and_short_pitch(ctx):
    import csdr_amd
    shape, alg, q = (8, 65), rm.GARDNER, 1
    m = case(shape, alg, q)
    x = m["x"][:3]; n = x.shape[1]
    for sq in (0, 1):
        p = csdr_amd.pulserx_params(m["taps"], alg, 8, tc.LOOP_GAIN, tc.MAX_ERROR, q, m["gain"], 4, sq)
        with ctx.pulse_rx(p, 3, "filter", "slice") as o:
            assert o.max_out(n) == ((n + 3 * 4 + 65) // 4 + 1) * (1 + sq) and o.max_out(0) == (77 // 4 + 1) * (1 + sq) and o.max_out(-1) == 0
            di = ctx.upload(x); do = ctx.alloc(o.max_out(n) * 3 + 256); dc = ctx.alloc(256)
            with pytest.raises(csdr_amd.CsdrAmdError):
                o.process_dev(di.ptr, n, n, do.ptr, o.max_out(n) - 1, dc.ptr)            # a short out_pitch consumes nothing ...
            with pytest.raises(csdr_amd.CsdrAmdError):
                o.process_dev(di.ptr, n, n - 1, do.ptr, o.max_out(n), dc.ptr)
            with pytest.raises(csdr_amd.CsdrAmdError):
                o.process_dev(di.ptr, n, n, do.ptr, o.max_out(n), None)
            with pytest.raises(csdr_amd.CsdrAmdError):
                o.process_dev(di.ptr, n, n, do.ptr, o.max_out(n), dc.ptr, d_err=do.ptr)  # errors and indexes only to TIMING
            st = o.get_channel(0)
            assert (st.tail_len, st.correction_offset, st.base) == (0, 0, 0)
            res = o.process(x)                                                           # ... so the stream still starts here
            for ch in range(3):
                assert np.array_equal(res[ch], want_bytes(m["models"][ch], m["gain"], sq, 4))


def test_create_errors(ctx):
    import csdr_amd
    taps = tc.taps_of((8, 65))
    good = dict(taps=taps, algorithm=0, decimation=8, loop_gain=0.5, max_error=2.0, use_q=1, gain=1.0, n_symbols=4, slice_q=0)
    for kw, stages, ch in [(dict(decimation=1), ("filter", "slice"), 1), (dict(algorithm=2), ("filter", "slice"), 1), (dict(loop_gain=0.6), ("filter", "slice"), 1),
                           (dict(n_symbols=1), ("filter", "slice"), 1), (dict(taps=None), ("filter", "timing"), 1), (dict(), ("timing", "filter"), 1),
                           (dict(), (0, 3), 1), (dict(), ("filter", "slice"), 0)]:
        with pytest.raises(csdr_amd.CsdrAmdError):
            ctx.pulse_rx(csdr_amd.pulserx_params(**dict(good, **kw)), ch, stages[0], stages[1])
    with ctx.pulse_rx(csdr_amd.pulserx_params(**good), 2) as o:
        with pytest.raises(csdr_amd.CsdrAmdError):
            o.set_lanes(65)
        assert o.kernel_name() == "" and o.lanes() in LANES


def test_pulserx_cycles(ctx):
    import csdr_amd
    import test_lifecycle_gpu as tl
    taps = tc.taps_of((8, 65))
    p = csdr_amd.pulserx_params(taps, 0, 8, 0.5, 2.0, 1, 1.0, 4, 1)
    tl._object_cycles(ctx, lambda c: csdr_amd.PulseRx(c, p, 2), tl._noise((2, 4096), np.complex64, 8))


# ------------------------------------------------------------------ 5. the command line
def _run(cmd, data, timeout=120):
    r = subprocess.run(cmd, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr.decode()


FILTER_CMD, TIMING_CMD = "pulse_shaping_filter_cc RRC 8 65 0.35", "timing_recovery_cc GARDNER 8 0.5 2 --add_q"


def _cli_case():
    import csdr_amd
    shape, alg, q = (8, 65), rm.GARDNER, 1
    taps = csdr_amd.firdes_rrc_f(65, 8, 0.35)
    x = rm.signal(4, 8, taps, 2000, 1, rms=tc.rms_of(shape, alg, q), seed=4)[0][0]
    gain = np.float32(1.0 / tc.rms_of(shape, alg, q))
    return shape, alg, q, taps, x, gain, repr(float(gain))


def test_cli_chain_is_fused(ctx):
    """the four fusable runs give the object's stream: the CPU walk's bits"""
    import csdr_amd
    shape, alg, q, taps, x, gain, gtxt = _cli_case()
    p = lambda ns=2, sq=0: csdr_amd.pulserx_params(taps, alg, 8, 0.5, 2.0, q, gain, ns, sq)
    out, err = _run([CSDR, "chain", "%s | %s | realpart_cf | gain_ff %s | generic_slicer_f_u8 4" % (FILTER_CMD, TIMING_CMD, gtxt)], x.tobytes())
    assert "pulse_shaping_filter_cc .. generic_slicer_f_u8 recognised" in err and "one fused pulse-shaped receive object" in err
    want = csdr_amd.pulserx_debug_walk(p(4, 0), "filter", "slice", x)
    assert out == want.tobytes() and want.size > 1900
    out_q, err = _run([CSDR, "chain", "%s | %s | gain_ff %s | generic_slicer_f_u8 3" % (FILTER_CMD, TIMING_CMD, gtxt)], x.tobytes())
    assert "one fused pulse-shaped receive object" in err and out_q == csdr_amd.pulserx_debug_walk(p(3, 1), "filter", "slice", x).tobytes()
    out_t, err = _run([CSDR, "chain", "%s | %s" % (FILTER_CMD, TIMING_CMD)], x.tobytes())
    sym = csdr_amd.pulserx_debug_walk(p(), "filter", "timing", x)
    assert "pulse_shaping_filter_cc .. timing_recovery_cc recognised" in err and out_t == sym.tobytes()
    out_c, err = _run([CSDR, "chain", "%s | %s | realpart_cf | gain_ff %s" % (FILTER_CMD, TIMING_CMD, gtxt)], x.tobytes())     # the prefix fuses, the rest follows
    assert "pulse_shaping_filter_cc .. timing_recovery_cc recognised" in err
    assert out_c == (gain * np.ascontiguousarray(sym.real)).astype(np.float32).tobytes()


def test_cli_chain_vs_reference_pipeline(ctx):
    """the fused run against the compiled reference's pipeline of five processes on whole blocks, on the prefix in which the order of a float32 sum
    cannot decide a truncation: bytes equal except beside a slicer limit"""
    if not os.path.exists(REF_CSDR):
        pytest.skip("reference binary not built (oracle/_ref/csdr)")
    if not os.path.exists(tc.REF_LIB):
        pytest.skip("reference library not built (oracle/_ref/libcsdr_ref.so)")
    import ctypes as C
    import test_pulse_cpu as tp
    import test_psk31_cpu as tk
    shape, alg, q, taps, x, gain, gtxt = _cli_case()
    out, err = _run([CSDR, "chain", "%s | %s | realpart_cf | gain_ff %s | generic_slicer_f_u8 4" % (FILTER_CMD, TIMING_CMD, gtxt)], x.tobytes())
    assert "one fused pulse-shaped receive object" in err
    L = tp.bind_modem(C.CDLL(tc.REF_LIB))
    L.timing_recovery_init.restype = tk.TRState
    L.timing_recovery_init.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_char_p]
    L.timing_recovery_cc.restype = None
    L.timing_recovery_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(tk.TRState)]
    _, _, ridx, _ = tk.ref_timing(L, tp.lib_fir(L, x, taps), alg, 8, 0.5, 2.0, True)
    k, f64, gr, gi, _ = tc.reference_prefix(shape, alg, q, x, taps, ridx)
    assert k >= 0.9 * ridx.size
    pipe = " | ".join("%s %s" % (REF_CSDR, c) for c in (FILTER_CMD, TIMING_CMD, "realpart_cf", "gain_ff %s" % gtxt, "generic_slicer_f_u8 4"))
    ref_out = subprocess.run(["sh", "-c", pipe], input=x.tobytes() + bytes(8 * 1024 * 16), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=120).stdout
    rb = np.frombuffer(ref_out, np.uint8); b = np.frombuffer(out, np.uint8)
    kk = min(k, b.size)
    assert kk > 1700 and rb.size >= kk
    near = tc.near_a_limit(f64[:kk], gr[:kk], gi[:kk], float(gain), 0, 4)
    assert not np.any((b[:kk] != rb[:kk]) & ~near) and np.count_nonzero(near) <= 0.02 * kk


def test_cli_unfusable_runs_stay_unfused(ctx):
    import csdr_amd
    taps = csdr_amd.firdes_rrc_f(65, 8, 0.35)
    x = rm.signal(4, 8, taps, 400, 1, rms=1.4, seed=6)[0][0]
    filtered, _ = _run([CSDR, "pulse_shaping_filter_cc", "RRC", "8", "65", "0.35"], x.tobytes())
    for opt, dtype in (("--output_error", np.float32), ("--output_indexes", np.uint32)):
        out, err = _run([CSDR, "chain", "%s | %s %s" % (FILTER_CMD, TIMING_CMD, opt)], x.tobytes())
        assert "pulse_rx" not in err and "pulse-shaped receive" not in err
        alone, _ = _run([CSDR] + TIMING_CMD.split() + [opt], filtered)
        assert out == alone and np.frombuffer(out, dtype).size > 350
    r = subprocess.run([CSDR, "chain", "%s | %s --octave 1" % (FILTER_CMD, TIMING_CMD)], input=x.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode != 0 and b"not supported" in r.stderr and b"pulse_rx" not in r.stderr
    # a gain and a slicer without the timing loop in front, and a loop a BPSK31 run has taken, are nobody's fused receive run
    out, err = _run([CSDR, "chain", "%s | realpart_cf | gain_ff 0.5 | generic_slicer_f_u8 4" % FILTER_CMD], x.tobytes())
    assert "pulse_rx" not in err and len(out) == x.size - 64
    out, err = _run([CSDR, "chain", "%s | %s | dbpsk_decoder_c_u8" % (FILTER_CMD, TIMING_CMD)], x.tobytes())
    assert "fused BPSK31 object" in err and "pulse_rx" not in err


# ------------------------------------------------------------------ 6. the loop back
@pytest.mark.parametrize("forced", [False, True])
def test_loopback_through_the_transmit_object(ctx, forced):
    """PulseTx (QPSK, 8 samples per symbol, RRC 65) -> delays of 3, 4, 5 samples -> PulseRx with the same taps and a three-level slicer per component.
    Symbol m peaks at sample 8 m - 64 behind both filters (each takes (T - 1) / 2 = 32), so the receiver's index j belongs to symbol round((j + 64) / 8):
    every transmitted symbol in reach is sampled once and sliced to the levels of its constellation point."""
    import csdr_amd
    I, T, n = 8, 65, 600
    taps = csdr_amd.firdes_rrc_f(T, I, 0.35)
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 4, (3, n)).astype(np.uint8)
    with ctx.pulse_tx(3, 4, I, taps) as tx:
        y = tx.process(idx)
    scale, delays = 8.0, (3, 4, 5)
    x = np.zeros((3, y.shape[1] + 8), np.complex64)
    for ch, d in enumerate(delays):
        x[ch, d:d + y.shape[1]] = scale * y[ch]
    peak = float(np.sum(taps.astype(np.float64) ** 2))
    levels = {(2, 1): 0, (1, 2): 1, (0, 1): 2, (1, 0): 3}                  # (I level, Q level) of the symbols 1, i, -1, -i
    p = csdr_amd.pulserx_params(taps, "GARDNER", I, 0.5, 2.0, True, 1.0 / (scale * peak), 3, True)
    with ctx.pulse_rx(p, 3, "filter", "timing") as o:
        o.force_generic(forced)
        timing = o.process(x, with_extras=True)
    with ctx.pulse_rx(p, 3, "filter", "slice") as o:
        o.force_generic(forced)
        sliced = o.process(x)
    for ch, d in enumerate(delays):
        j = timing[ch][2].astype(np.int64) - d
        m = np.rint((j + 64) / I).astype(np.int64)
        b = sliced[ch].reshape(-1, 2)
        assert b.shape[0] == m.size > n - 30
        ok = (m >= 8) & (m < n - 8)
        assert np.array_equal(m[ok], np.arange(8, n - 8)), ch
        dec = np.array([levels.get((int(u), int(v)), -1) for u, v in b[ok]])
        assert np.array_equal(dec, idx[ch, 8:n - 8]), ch
