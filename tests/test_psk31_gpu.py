"""GPU checks of the BPSK31 receive chain (psk31.hip): the fused object and every stage range against the float32 model bit for bit, against the
reference library and binary, cut and batch invariance, channel reset, the CLI commands and `csdr chain` fusion, argument errors and lifecycle."""
import os
import subprocess
import numpy as np
import pytest

import psk31_model as pm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")
REF_CSDR = os.path.join(ROOT, "oracle", "_ref", "csdr")
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
STAGES = ["agc", "timing", "dbpsk", "varicode"]
OWRX = "simple_agc_cc 0.001 0.5 | timing_recovery_cc GARDNER 256 0.5 2 --add_q | dbpsk_decoder_c_u8 | psk31_varicode_decoder_u8_u8"


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _model_stages(x, D=256, alg=pm.GARDNER, use_q=True):
    a, _ = pm.agc(x, 0.001, 0.5)
    s, e, i, _, _ = pm.timing(a, alg, D, 0.5, 2.0, use_q)
    b = pm.dbpsk(s)
    t, _ = pm.varicode_decode(b)
    return dict(agc=a, timing=s, errors=e, indexes=i, dbpsk=b, varicode=np.frombuffer(t, np.uint8))


def _input_for(stage, x, m):
    return {"agc": x, "timing": m["agc"], "dbpsk": m["timing"], "varicode": m["dbpsk"]}[stage]


def _eq(a, b):
    a = np.asarray(a); b = np.asarray(b)
    if a.dtype == np.complex64:
        return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


@pytest.mark.parametrize("D,alg,use_q", [(256, pm.GARDNER, True), (40, pm.EARLYLATE, False), (12, pm.GARDNER, False)])
def test_every_stage_range_vs_model(ctx, D, alg, use_q):
    import csdr_amd
    x = pm.psk31_signal("stage ranges " + str(D), decimation=D, carrier=0.0009, timing_offset=D // 3, snr_db=14, seed=D)
    m = _model_stages(x, D, alg, use_q)
    P = csdr_amd.psk31_params(algorithm=alg, decimation=D, use_q=use_q)
    for f in range(4):
        for l in range(f, 4):
            o = ctx.psk31(P, 1, STAGES[f], STAGES[l])
            got = o.process(_input_for(STAGES[f], x, m))
            assert _eq(got, m[STAGES[l]]), (STAGES[f], STAGES[l])
            assert o.kernel_name() == ("k_psk31_tiled" if f == 0 and l >= 1 else "k_psk31")
            o.close()
    o = ctx.psk31(P, 1, "agc", "timing")
    s, e, i = o.process(x, with_extras=True)
    assert _eq(s, m["timing"]) and np.array_equal(e.view(np.uint32), m["errors"].view(np.uint32)) and np.array_equal(i.astype(np.int64), m["indexes"])


def test_fused_vs_reference(ctx):
    import csdr_amd
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built")
    import ctypes as C
    import test_psk31_cpu as tc
    L = C.CDLL(REF_LIB)
    for fn, (rt, at) in {"simple_agc_cc": (None, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p]),
                         "timing_recovery_init": (tc.TRState, [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_char_p]),
                         "timing_recovery_cc": (None, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(tc.TRState)]),
                         "dbpsk_decoder_c_u8": (None, [C.c_void_p, C.c_void_p, C.c_int]),
                         "psk31_varicode_decoder_push": (C.c_char, [C.POINTER(C.c_ulonglong), C.c_ubyte])}.items():
        getattr(L, fn).restype = rt; getattr(L, fn).argtypes = at
    texts = ["CQ CQ DE MI355X K", "the quick brown fox jumps over the lazy dog 0123456789"]
    xs = [pm.psk31_signal(t, carrier=0.0004 * k, phase=0.3 * k, timing_offset=37 * k, snr_db=[30, 20, 10][k % 3], seed=k)
          for k, t in enumerate(texts * 2)]
    n = max(v.size for v in xs)
    X = np.stack([np.concatenate([v, v[-1] * np.ones(n - v.size, np.complex64)]) for v in xs])     # the shorter bursts padded with their last sample
    o = ctx.psk31(csdr_amd.psk31_params(), X.shape[0], "agc", "varicode")
    got = o.process(X)
    ob = ctx.psk31(csdr_amd.psk31_params(), X.shape[0], "agc", "dbpsk")
    gotb = ob.process(X)
    for k in range(X.shape[0]):
        a, _ = tc.ref_agc(L, X[k], 0.001, 0.5, 65535.0)
        s, _, _, _ = tc.ref_timing(L, a, 0, 256, 0.5, 2.0, True)
        b = tc.ref_dbpsk(L, s)
        t = tc.ref_varicode(L, b)
        assert np.array_equal(gotb[k], b), k
        assert got[k].tobytes() == t, k
        if k < 2:
            assert texts[k].encode() in t
    o.close(); ob.close()


def test_cut_invariance(ctx):
    import csdr_amd
    D = 64
    x = pm.psk31_signal("cut invariance", decimation=D, carrier=0.001, timing_offset=5, snr_db=12, seed=3)
    m = _model_stages(x, D)
    rng = np.random.default_rng(1)
    cuts = [0, 1, 1, D // 2 + 1, 3 * D // 2 - 1, D * 3 // 2, 0] + list(rng.integers(0, 4 * D, 60))
    cuts = [int(c) for c in cuts]
    cuts.append(x.size - sum(cuts))
    assert cuts[-1] > 0
    P = csdr_amd.psk31_params(decimation=D)
    for last in ["agc", "timing", "dbpsk", "varicode"]:
        o = ctx.psk31(P, 1, "agc", last)
        assert _eq(o.process(x, calls=cuts), m[last]), last
    o = ctx.psk31(P, 1, "agc", "timing")
    s, e, i = o.process(x, calls=cuts, with_extras=True)
    assert np.array_equal(i.astype(np.int64), m["indexes"])


def test_batch_invariance_and_lanes(ctx):
    import csdr_amd
    D = 32
    base = [pm.psk31_signal("ch%d" % k, decimation=D, carrier=0.0003 * (k % 5), timing_offset=k % D, snr_db=15, seed=k) for k in range(16)]
    n = min(v.size for v in base)
    X = np.stack([base[k % 16][:n] for k in range(1024)])
    P = csdr_amd.psk31_params(decimation=D)
    o = ctx.psk31(P, 1024, "agc", "varicode")
    many = o.process(X)
    for lanes in (1, 64):
        o.reset(); o.set_lanes(lanes)
        again = o.process(X)
        assert all(np.array_equal(a, b) for a, b in zip(many, again)), lanes
    for k in (0, 5, 511, 1023):
        one = ctx.psk31(P, 1, "agc", "varicode").process(X[k])
        assert np.array_equal(one, many[k]), k
        assert np.array_equal(one, csdr_amd.psk31_debug_walk(P, "agc", "varicode", X[k])), k


def test_reset_channel_and_max_out(ctx):
    import csdr_amd
    D = 16
    x = pm.psk31_signal("reset me", decimation=D, snr_db=20, seed=8)
    X = np.stack([x, x, x])
    P = csdr_amd.psk31_params(decimation=D)
    o = ctx.psk31(P, 3, "agc", "timing")
    first = o.process(X)
    o.reset_channel(1)
    st = o.get_channel(1)
    assert st.tail_len == 0 and st.gain == 1.0 and st.base == 0
    second = o.process(X)
    assert _eq(second[1], first[1])                             # channel 1 starts over
    assert not _eq(second[0][:len(first[0])], first[0])         # channel 0 continues
    for calls in ([1], [D], [D * 3 // 2 + 5], [10 * D]):
        for c in range(3):
            o.reset()
            r = o.process(X[:, :sum(calls)], calls=calls)
            assert all(len(v) <= o.max_out(calls[0]) for v in r)


def test_simple_agc_standalone(ctx):
    rng = np.random.default_rng(2)
    x = ((rng.standard_normal((3, 5000)) + 1j * rng.standard_normal((3, 5000))) * 0.2).astype(np.complex64)
    x[:, ::50] = 0
    y, g = ctx.simple_agc_cc(x, 0.01, 0.5, 30.0, gain=[1.0, 2.0, 0.5])
    for k, g0 in enumerate([1.0, 2.0, 0.5]):
        want, gw = pm.agc(x[k], 0.01, 0.5, 30.0, gain=g0)
        assert _eq(y[k], want) and g[k] == gw


def _run(cmd, data, timeout=120):
    r = subprocess.run(cmd, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr.decode()


def test_cli_commands_and_chain(ctx):
    x = pm.psk31_signal("hello from the cli", carrier=0.0002, timing_offset=100, snr_db=18, seed=11)
    m = _model_stages(x)
    raw = x.tobytes()
    out, _ = _run([CSDR, "simple_agc_cc", "0.001", "0.5"], raw)
    assert _eq(np.frombuffer(out, np.complex64), m["agc"])
    out, _ = _run([CSDR, "timing_recovery_cc", "GARDNER", "256", "0.5", "2", "--add_q"], m["agc"].tobytes())
    assert _eq(np.frombuffer(out, np.complex64), m["timing"])
    out, _ = _run([CSDR, "timing_recovery_cc", "GARDNER", "256", "0.5", "2", "--add_q", "--output_indexes"], m["agc"].tobytes())
    assert np.array_equal(np.frombuffer(out, np.uint32).astype(np.int64), m["indexes"])
    out, _ = _run([CSDR, "dbpsk_decoder_c_u8"], m["timing"].tobytes())
    assert np.array_equal(np.frombuffer(out, np.uint8), m["dbpsk"])
    out, _ = _run([CSDR, "psk31_varicode_decoder_u8_u8"], m["dbpsk"].tobytes())
    assert out == m["varicode"].tobytes()
    out, err = _run([CSDR, "chain", OWRX], raw)
    assert out == m["varicode"].tobytes() and b"hello from the cli" in out
    assert "fused BPSK31 object" in err
    if os.path.exists(REF_CSDR):
        ref_out = subprocess.run(["sh", "-c", "%s simple_agc_cc 0.001 0.5 | %s timing_recovery_cc GARDNER 256 0.5 2 --add_q | %s dbpsk_decoder_c_u8 | "
                                  "%s psk31_varicode_decoder_u8_u8" % ((REF_CSDR,) * 4)], input=raw + bytes(8 * 16384 * 4),
                                 stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=120).stdout
        assert b"hello from the cli" in ref_out and out in ref_out


def test_argument_errors(ctx):
    import csdr_amd
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.psk31(csdr_amd.psk31_params(decimation=10))
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.psk31(csdr_amd.psk31_params(loop_gain=2.0, max_error=2.0))
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.psk31(csdr_amd.psk31_params(), 1, "varicode", "agc")
    o = ctx.psk31(csdr_amd.psk31_params(), 2)
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.reset_channel(2)
    r = subprocess.run([CSDR, "timing_recovery_cc", "GARDNER", "10"], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode != 0 and b"divisible by 4" in r.stderr
    r = subprocess.run([CSDR, "timing_recovery_cc", "GARDNER", "16", "0.5", "2", "--octave", "1"], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode != 0 and b"not supported" in r.stderr


def test_lifecycle_no_growth(ctx):
    import csdr_amd
    import torch
    x = np.zeros((64, 4096), np.complex64)
    def cycle():
        o = ctx.psk31(csdr_amd.psk31_params(decimation=64), 64)
        o.process(x)
        o.close()
    cycle()
    ctx.sync() if hasattr(ctx, "sync") else None
    f0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        cycle()
    f1 = torch.cuda.mem_get_info(0)[0]
    assert f1 >= f0 - (4 << 20)


def test_dropin_symbols_vs_reference(ctx):
    """simple_agc_cc, timing_recovery_init / _cc, dbpsk_decoder_c_u8 and psk31_varicode_decoder_push of libcsdr_amd.so through ctypes, as a client built
    against the reference's headers calls them, against the model and (where built) the reference library"""
    import ctypes as C
    import csdr_amd
    import test_psk31_cpu as tc
    A = C.CDLL(csdr_amd.lib()._name)
    A.simple_agc_cc.restype = None
    A.simple_agc_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p]
    A.timing_recovery_init.restype = tc.TRState
    A.timing_recovery_init.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_char_p]
    A.timing_recovery_cc.restype = None
    A.timing_recovery_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(tc.TRState)]
    A.dbpsk_decoder_c_u8.restype = None
    A.dbpsk_decoder_c_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    A.psk31_varicode_decoder_push.restype = C.c_char
    A.psk31_varicode_decoder_push.argtypes = [C.POINTER(C.c_ulonglong), C.c_ubyte]
    A.timing_recovery_get_algorithm_from_string.restype = C.c_int
    A.timing_recovery_get_algorithm_from_string.argtypes = [C.c_char_p]
    A.timing_recovery_get_string_from_algorithm.restype = C.c_char_p
    A.timing_recovery_get_string_from_algorithm.argtypes = [C.c_int]
    assert A.timing_recovery_get_algorithm_from_string(b"EARLYLATE") == 1 and A.timing_recovery_get_algorithm_from_string(b"x") == 0
    assert A.timing_recovery_get_string_from_algorithm(1) == b"EARLYLATE"
    D = 64
    x = pm.psk31_signal("drop in", decimation=D, carrier=0.0005, timing_offset=9, snr_db=16, seed=21)
    # AGC in two calls, the gain carried through current_gain
    want, gw = pm.agc(x, 0.001, 0.5)
    y1, g = tc.ref_agc(A, x[:1000], 0.001, 0.5, 65535.0)
    y2, g = tc.ref_agc(A, x[1000:], 0.001, 0.5, 65535.0, gain=g)
    assert _eq(np.concatenate([y1, y2]), want) and g == gw
    # timing recovery: the CLI's loop (csdr.c:2625-2646) over 1000-sample buffers against one model call over the stream
    ws, we, wi, _, _ = pm.timing(want, 0, D, 0.5, 2.0, True)
    st = A.timing_recovery_init(0, D, 1, 0.5, 2.0, -1, None)
    buf = want[:1000].copy(); at = 1000; syms, idxs, base = [], [], 0
    while True:
        out = np.zeros(1000, np.complex64); err = np.zeros(1000, np.float32); idx = np.zeros(1000, np.int32)
        A.timing_recovery_cc(buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), buf.size, err.ctypes.data_as(C.c_void_p),
                             idx.ctypes.data_as(C.c_void_p), C.byref(st))
        syms.append(out[:st.output_size]); idxs.append(idx[:st.output_size].astype(np.int64) + base)
        base += st.input_processed
        if at >= want.size:
            break
        take = min(st.input_processed, want.size - at)
        buf = np.concatenate([buf[st.input_processed:], want[at:at + take]]); at += take
    s = np.concatenate(syms)
    m = min(s.size, ws.size)
    assert m > 20 and _eq(s[:m], ws[:m]) and np.array_equal(np.concatenate(idxs)[:m], wi[:m])
    # dbpsk: one process-wide last_input, carried across calls
    z = np.zeros(1, np.complex64); zb = np.zeros(1, np.uint8)
    A.dbpsk_decoder_c_u8(z.ctypes.data_as(C.c_void_p), zb.ctypes.data_as(C.c_void_p), 1)
    b = np.zeros(ws.size, np.uint8)
    h = ws.size // 2
    A.dbpsk_decoder_c_u8(ws[:h].ctypes.data_as(C.c_void_p), b[:h].ctypes.data_as(C.c_void_p), h)
    b2 = np.zeros(ws.size - h, np.uint8)
    A.dbpsk_decoder_c_u8(np.ascontiguousarray(ws[h:]).ctypes.data_as(C.c_void_p), b2.ctypes.data_as(C.c_void_p), ws.size - h)
    bits = np.concatenate([b[:h], b2])
    assert np.array_equal(bits, pm.dbpsk(ws))
    assert tc.ref_varicode(A, bits) == pm.varicode_decode(bits)[0]
    if os.path.exists(REF_LIB):
        L = C.CDLL(REF_LIB)
        for fn in ("psk31_varicode_decoder_push",):
            getattr(L, fn).restype = C.c_char; getattr(L, fn).argtypes = [C.POINTER(C.c_ulonglong), C.c_ubyte]
        L.dbpsk_decoder_c_u8.restype = None; L.dbpsk_decoder_c_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        assert np.array_equal(tc.ref_dbpsk(L, ws), bits)
        assert tc.ref_varicode(L, bits) == tc.ref_varicode(A, bits)


@pytest.mark.parametrize("D,alg,use_q", [(256, pm.GARDNER, True), (8, pm.EARLYLATE, True), (40, pm.GARDNER, False), (12, pm.EARLYLATE, False)])
def test_tiled_equals_generic(ctx, D, alg, use_q):
    """k_psk31_tiled (LDS ring, AGC split off the chain lane) against k_psk31 and the model: every fused range, several channel counts per wave, cut
    into calls that end inside a tile, a symbol and the tail"""
    import csdr_amd
    base = [pm.psk31_signal("tile %d" % k, decimation=D, carrier=0.0004 * (k % 3), timing_offset=(7 * k) % D, snr_db=13 + k % 5, seed=50 + k) for k in range(37)]
    n = min(v.size for v in base)
    X = np.stack([v[:n] for v in base])
    P = csdr_amd.psk31_params(algorithm=alg, decimation=D, use_q=use_q)
    rng = np.random.default_rng(D)
    cuts = [0, 1, 63, 64, 65] + [int(c) for c in rng.integers(0, 5 * 64, 12)]
    while sum(cuts) >= n:                                      # (short streams at small D)
        cuts.pop()
    cuts.append(n - sum(cuts))
    m0 = _model_stages(X[0], D, alg, use_q)
    for last in ("timing", "dbpsk", "varicode"):
        g = ctx.psk31(P, X.shape[0], "agc", last); g.force_generic()
        want = g.process(X, calls=cuts)
        assert g.kernel_name() == "k_psk31"
        assert _eq(want[0], m0[last]), last
        for lanes in (0, 1, 3, 16, 64):
            t = ctx.psk31(P, X.shape[0], "agc", last); t.set_lanes(lanes)
            got = t.process(X, calls=cuts)
            assert t.kernel_name() == "k_psk31_tiled"
            assert all(_eq(a, b) for a, b in zip(got, want)), (last, lanes)
            sg, st_ = g.get_channel(36), t.get_channel(36)
            assert (sg.gain, sg.tail_len, sg.correction_offset, sg.base) == (st_.gain, st_.tail_len, st_.correction_offset, st_.base)
            t.close()
        g.close()
    t = ctx.psk31(P, X.shape[0], "agc", "timing")
    s, e, i = t.process(X, calls=cuts, with_extras=True)[5]
    w = _model_stages(X[5], D, alg, use_q)
    assert np.array_equal(e.view(np.uint32), w["errors"].view(np.uint32)) and np.array_equal(i.astype(np.int64), w["indexes"])


def test_large_decimation_runs_generic(ctx):
    import csdr_amd
    D = 8192                                                   # the ring (3 D/2 + 66 samples) does not fit: k_psk31
    x = pm.psk31_signal("big", decimation=D, snr_db=20, seed=4)[: 40 * D]
    o = ctx.psk31(csdr_amd.psk31_params(decimation=D), 1, "agc", "timing")
    got = o.process(x)
    assert o.kernel_name() == "k_psk31"
    assert _eq(got, _model_stages(x, D)["timing"])
