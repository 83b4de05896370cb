"""The FIR resamplers on the MI355X (resampler.hip): the batch objects against the float64 model (resampler_model.py), call-cut and batch invariance bit for bit,
the CLI loop modes, the drop-in functions and the CLI commands against the reference, argument errors and the objects' device-memory lifecycle."""
import ctypes as C
import os
import struct
import subprocess
import numpy as np
import pytest

import resampler_model as rm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "csdr_amd", "csdr")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libcsdr_ref.so")
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "csdr")
GRID = [(1, 4), (1, 6), (3, 2), (2, 3), (5, 7), (4, 1), (147, 160)]
TOL = 1e-5


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _shapes():
    for I, D in GRID:
        yield I, D, 81
    yield 4, 1, 3
    yield 5, 7, 3
    yield 3, 2, 80
    yield 147, 160, 4001


def _taps(T, I, D):
    import csdr_amd
    return csdr_amd.rational_resampler_get_lowpass_f(T, I, D)


def _ftaps(ctx, T, I):
    return ctx.firdes_lowpass_f(T, np.float32(0.5) / np.float32(I))


@pytest.mark.parametrize("I,D,T", list(_shapes()))
@pytest.mark.parametrize("generic", [False, True])
def test_resampler_matches_model(ctx, I, D, T, generic):
    import csdr_amd
    rng = np.random.default_rng(I + 3 * D + T)
    taps = _taps(T, I, D)
    x = rng.uniform(-1, 1, (3, 60000)).astype(np.float32)
    r = csdr_amd.Resampler(ctx, I, D, taps, 3)
    if generic:
        r.force_generic()
    y = r.process(x, [20000, 1, 0, 39999])
    assert r.kernel_name() == ("k_rr_generic" if generic else "k_rr_poly")
    for s in range(3):
        want, _ = rm.rational_resampler_ff(x[s], I, D, taps)
        assert y.shape[1] == want.size
        if want.size:
            assert rm.relrms(y[s], want) <= TOL or np.abs(y[s] - want).max() <= 1e-6
    r.close()


def test_resampler_incoming_delay(ctx):
    import csdr_amd
    rng = np.random.default_rng(2)
    for I, D, T in [(147, 160, 401), (3, 2, 80), (5, 7, 81)]:
        taps = _taps(T, I, D)
        x = rng.uniform(-1, 1, 9000).astype(np.float32)
        for L in (1, I - 1):
            r = csdr_amd.Resampler(ctx, I, D, taps, 1, last_taps_delay=L)
            y = r.process(x)
            s, d, _ = rm.rr_schedule(y.size + 1, I, D, T, L)
            want = rm._rr_values(x, I, taps, s[:y.size], d[:y.size])
            assert s[y.size] + T // I + 1 > x.size and s[y.size - 1] + T // I + 1 <= x.size
            assert rm.relrms(y, want) <= TOL
            r.close()


@pytest.mark.parametrize("I,D,T", [(147, 160, 4001), (1, 4, 81), (3, 2, 80), (4, 1, 3)])
def test_resampler_call_cut_invariance(ctx, I, D, T):
    import csdr_amd
    rng = np.random.default_rng(5)
    taps = _taps(T, I, D)
    x = rng.uniform(-1, 1, (2, 30000)).astype(np.float32)
    r = csdr_amd.Resampler(ctx, I, D, taps, 2)
    whole = r.process(x)
    cuts = [int(v) for v in rng.integers(0, 700, 40)]
    cuts.append(30000 - sum(cuts)); assert cuts[-1] >= 0
    r.reset()
    pieces = r.process(x, cuts)
    r.reset()
    ones = r.process(x[:, :3000], [1] * 1500 + [0] * 3 + [1500])
    assert np.array_equal(whole.view(np.uint32), pieces.view(np.uint32))
    assert np.array_equal(whole[:, :ones.shape[1]].view(np.uint32), ones.view(np.uint32))
    r.force_generic()
    r.reset()
    gen = r.process(x, cuts)
    assert np.array_equal(whole.view(np.uint32), gen.view(np.uint32))       # same summation order in both kernels
    r.close()


def test_resampler_batch_invariance(ctx):
    import csdr_amd
    rng = np.random.default_rng(6)
    I, D, T = 147, 160, 401
    taps = _taps(T, I, D)
    x = rng.uniform(-1, 1, (1024, 8192)).astype(np.float32)
    r = csdr_amd.Resampler(ctx, I, D, taps, 1024)
    y = r.process(x, [5000, 3192])
    r.close()
    one = csdr_amd.Resampler(ctx, I, D, taps, 1)
    for s in list(range(0, 1024, 97)) + [1023]:
        one.reset()
        assert np.array_equal(one.process(x[s]).view(np.uint32), y[s].view(np.uint32))
    one.close()


def test_resampler_reset(ctx):
    import csdr_amd
    rng = np.random.default_rng(7)
    taps = _taps(81, 3, 2)
    x = rng.uniform(-1, 1, 10000).astype(np.float32)
    r = csdr_amd.Resampler(ctx, 3, 2, taps, 1)
    a = r.process(x)
    r.process(rng.uniform(-1, 1, 777).astype(np.float32))
    r.reset()                                       # a fresh stream: no history, schedule from output 0
    assert np.array_equal(r.process(x).view(np.uint32), a.view(np.uint32))
    r.close()


@pytest.mark.parametrize("I,D,tbw", [(3, 2, 0.05), (147, 160, 0.001), (5, 7, 0.8), (147, 160, 0.05)])
def test_resampler_cli_bufsize_mode(ctx, I, D, tbw):
    import csdr_amd
    rng = np.random.default_rng(8)
    T = ctx.firdes_filter_len(tbw)
    taps = _taps(T, I, D)
    x = rng.uniform(-1, 1, 40000).astype(np.float32)
    want = rm.rational_resampler_cli(x, I, D, taps, 1024)
    r = csdr_amd.Resampler(ctx, I, D, taps, 1, bufsize=1024)
    y = r.process(x, [10000, 3, 29997])
    assert y.size == want.size and rm.relrms(y, want) <= TOL
    r.close()


@pytest.mark.parametrize("I,T", [(1, 81), (2, 81), (4, 81), (5, 81), (4, 3), (3, 80), (16, 161), (7, 4001)])
@pytest.mark.parametrize("generic", [False, True])
def test_interp_matches_model(ctx, I, T, generic):
    import csdr_amd
    rng = np.random.default_rng(I + T)
    taps = _ftaps(ctx, T, I)
    x = (rng.uniform(-1, 1, (2, 20000)) + 1j * rng.uniform(-1, 1, (2, 20000))).astype(np.complex64)
    p = csdr_amd.Interpolator(ctx, I, taps, 2)
    if generic:
        p.force_generic()
    y = p.process(x, [7000, 1, 0, 12999])
    assert p.kernel_name() == ("k_interp_generic" if generic else "k_interp_poly")
    for s in range(2):
        want = rm.fir_interpolate_cc(x[s], I, taps)
        assert y.shape[1] == want.size and rm.relrms(y[s], want) <= TOL
    p.force_generic(not generic)
    p.reset()
    cuts = [int(v) for v in rng.integers(0, 2000, 10)]
    z = p.process(x, cuts + [20000 - sum(cuts)])
    assert np.array_equal(z[:, :y.shape[1]].view(np.uint32), y.view(np.uint32))      # call cuts and kernel choice change no bit
    p.close()


def test_interp_batch_and_cli_mode(ctx):
    import csdr_amd
    rng = np.random.default_rng(9)
    taps = _ftaps(ctx, 81, 4)
    x = (rng.uniform(-1, 1, (1024, 2048)) + 1j * rng.uniform(-1, 1, (1024, 2048))).astype(np.complex64)
    p = csdr_amd.Interpolator(ctx, 4, taps, 1024)
    y = p.process(x)
    p.close()
    one = csdr_amd.Interpolator(ctx, 4, taps, 1)
    for s in (0, 511, 1023):
        one.reset()
        assert np.array_equal(one.process(x[s]).view(np.uint32), y[s].view(np.uint32))
    one.set_cli_bufsize(16384)
    got = one.process(x[3], [1000, 1048])
    want = rm.fir_interpolate_cli(x[3], 4, taps, 16384)
    assert got.size == want.size and rm.relrms(got, want) <= TOL
    one.close()


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built")

    class St(C.Structure):
        _fields_ = [("input_processed", C.c_int), ("output_size", C.c_int), ("last_taps_delay", C.c_int)]
    L = C.CDLL(REF_LIB)
    L.rational_resampler_ff.restype = St
    L.rational_resampler_ff.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.fir_interpolate_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    return L, St


def test_dropin_functions(ctx, ref):
    import csdr_amd
    R, St = ref
    A = C.CDLL(csdr_amd.LIB_PATH)
    A.rational_resampler_ff.restype = St
    A.rational_resampler_ff.argtypes = R.rational_resampler_ff.argtypes
    A.fir_interpolate_cc.argtypes = R.fir_interpolate_cc.argtypes
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rng = np.random.default_rng(10)
    for I, D, T in [(147, 160, 401), (5, 7, 5), (3, 2, 79), (1, 4, 81), (4, 1, 3)]:
        taps = _taps(T, I, D)
        x = rng.uniform(-1, 1, 1024).astype(np.float32)
        for L0 in sorted({0, I - 1}):
            a = np.zeros(1024 * I // D + 8, np.float32); b = np.zeros(1024 * I // D + 8, np.float32)
            sr = R.rational_resampler_ff(p(x), p(a), 1024, I, D, p(taps), T, L0)
            sa = A.rational_resampler_ff(p(x), p(b), 1024, I, D, p(taps), T, L0)
            assert (sa.input_processed, sa.output_size, sa.last_taps_delay) == (sr.input_processed, sr.output_size, sr.last_taps_delay)
            if sr.output_size:
                assert rm.relrms(b[:sr.output_size], a[:sr.output_size]) <= TOL or np.abs(b - a).max() <= 1e-6
    for I, T in [(4, 81), (3, 80)]:
        taps = _ftaps(ctx, T, I)
        x = (rng.uniform(-1, 1, 3000) + 1j * rng.uniform(-1, 1, 3000)).astype(np.complex64)
        a = np.zeros(3000 * I, np.complex64); b = np.zeros(3000 * I, np.complex64)
        kr = R.fir_interpolate_cc(p(x), p(a), 3000, I, p(taps), T)
        ka = A.fir_interpolate_cc(p(x), p(b), 3000, I, p(taps), T)
        assert ka == kr and rm.relrms(b[:ka], a[:kr]) <= TOL


def _run(cli, args, data, env_extra=None):
    env = dict(os.environ); env.pop("CSDR_FIXED_BUFSIZE", None); env.pop("CSDR_DYNAMIC_BUFSIZE_ON", None)
    env.update(env_extra or {})
    return subprocess.run([cli] + [str(a) for a in args], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)


def _need_ref_cli():
    if not os.path.exists(REF_CLI):
        pytest.skip("reference binary not built")


@pytest.mark.parametrize("mode", ["default", "fixed", "setbuf"])
def test_cli_rational_resampler(mode):
    _need_ref_cli()
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, 60000).astype(np.float32)
    env = {"fixed": {"CSDR_FIXED_BUFSIZE": "2000"}, "setbuf": {"CSDR_DYNAMIC_BUFSIZE_ON": "1"}}.get(mode)
    pre = b"csdr" + struct.pack("<i", 3000) if mode == "setbuf" else b""
    for cmd, I, D, tbw in [("rational_resampler_ff", 147, 160, 0.05), ("suboptimal_rational_resampler_ff", 3, 2, 0.05), ("rational_resampler_ff", 5, 7, 0.8)]:
        ours = _run(CLI, [cmd, I, D, tbw], pre + x.tobytes(), env)
        assert ours.returncode == 0, ours.stderr.decode()
        theirs = _run(REF_CLI, [cmd, I, D, tbw], pre + x.tobytes(), env).stdout
        if mode == "setbuf":
            assert ours.stdout[:8] == theirs[:8] == b"csdr" + struct.pack("<i", 3000 * I // D)
        o = np.frombuffer(ours.stdout[len(pre):], np.float32); t = np.frombuffer(theirs[len(pre):], np.float32)
        m = min(o.size, t.size)
        assert m >= o.size - 3000 and m > 10000 and rm.relrms(o[:m], t[:m]) <= TOL


@pytest.mark.parametrize("mode", ["default", "fixed", "setbuf"])
def test_cli_fir_interpolate(mode):
    _need_ref_cli()
    rng = np.random.default_rng(12)
    x = (rng.uniform(-1, 1, 50000) + 1j * rng.uniform(-1, 1, 50000)).astype(np.complex64)
    env = {"fixed": {"CSDR_FIXED_BUFSIZE": "4000"}, "setbuf": {"CSDR_DYNAMIC_BUFSIZE_ON": "1"}}.get(mode)
    pre = b"csdr" + struct.pack("<i", 3000) if mode == "setbuf" else b""
    ours = _run(CLI, ["fir_interpolate_cc", 4], pre + x.tobytes(), env)
    assert ours.returncode == 0, ours.stderr.decode()
    theirs = _run(REF_CLI, ["fir_interpolate_cc", 4], pre + x.tobytes(), env).stdout
    if mode == "setbuf":
        assert ours.stdout[:8] == theirs[:8] == b"csdr" + struct.pack("<i", 12000)
    o = np.frombuffer(ours.stdout[len(pre):], np.complex64); t = np.frombuffer(theirs[len(pre):], np.complex64)
    m = min(o.size, t.size)
    assert m > 100000 and m >= o.size - 4 * 16384 - 400 and rm.relrms(o[:m], t[:m]) <= TOL


def test_cli_chain_and_handoff(tmp_path):
    _need_ref_cli()
    rng = np.random.default_rng(13)
    x = rng.uniform(-1, 1, 60000).astype(np.float32)
    pipe = "rational_resampler_ff 147 160 | gain_ff 0.5 | rational_resampler_ff 3 2"
    ours = _run(CLI, ["chain", pipe], x.tobytes())
    assert ours.returncode == 0, ours.stderr.decode()
    t1 = _run(REF_CLI, ["rational_resampler_ff", 147, 160], x.tobytes()).stdout
    t2 = _run(REF_CLI, ["gain_ff", 0.5], t1).stdout
    t3 = np.frombuffer(_run(REF_CLI, ["rational_resampler_ff", 3, 2], t2).stdout, np.float32)
    o = np.frombuffer(ours.stdout, np.float32)
    m = min(o.size, t3.size - 1024)
    assert m > 40000 and rm.relrms(o[:m], t3[:m]) <= TOL
    xc = (rng.uniform(-1, 1, 40000) + 1j * rng.uniform(-1, 1, 40000)).astype(np.complex64)
    ours = _run(CLI, ["chain", "fir_interpolate_cc 2 | realpart_cf"], xc.tobytes())
    assert ours.returncode == 0, ours.stderr.decode()
    t = np.frombuffer(_run(REF_CLI, ["realpart_cf"], _run(REF_CLI, ["fir_interpolate_cc", 2], xc.tobytes()).stdout).stdout, np.float32)
    o = np.frombuffer(ours.stdout, np.float32)
    m = min(o.size, t.size - 1024)                  # (the reference's last realpart_cf block holds stale samples after a short read)
    assert m > 40000 and rm.relrms(o[:m], t[:m]) <= TOL
    # one two-process link: `csdr rational_resampler_ff 147 160 | csdr fir_interpolate_cc 2`-style hand-off between adjacent processes
    env = dict(os.environ, CSDR_AMD_IPC_VERBOSE="1", CSDR_AMD_IPC_WAIT_MS="3000")
    e0, e1 = open(tmp_path / "e0", "wb"), open(tmp_path / "e1", "wb")
    p0 = subprocess.Popen([CLI, "rational_resampler_ff", "147", "160"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=e0, env=env)
    p1 = subprocess.Popen([CLI, "rational_resampler_ff", "3", "2"], stdin=p0.stdout, stdout=subprocess.PIPE, stderr=e1, env=env)
    p0.stdout.close()
    import threading
    th = threading.Thread(target=lambda: (p0.stdin.write(x.tobytes()), p0.stdin.close()))
    th.start()
    out = p1.stdout.read()
    th.join(); p0.wait(timeout=60); p1.wait(timeout=60)
    assert p0.returncode == 0 and p1.returncode == 0
    e0.close(); e1.close()
    errs = open(tmp_path / "e0").read() + open(tmp_path / "e1").read()
    want = np.frombuffer(_run(REF_CLI, ["rational_resampler_ff", 3, 2], t1).stdout, np.float32)
    o = np.frombuffer(out, np.float32)
    m = min(o.size, want.size)
    assert m > 40000 and rm.relrms(o[:m], want[:m]) <= TOL
    assert "hand-off" in errs, errs


def test_cli_help_and_argument_errors():
    h = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    for c in (b"rational_resampler_ff", b"suboptimal_rational_resampler_ff", b"fir_interpolate_cc"):
        assert c in h.stderr
    for args in (["rational_resampler_ff"], ["rational_resampler_ff", "3"], ["rational_resampler_ff", "0", "2"], ["rational_resampler_ff", "3", "0"],
                 ["rational_resampler_ff", "3", "2", "0"], ["fir_interpolate_cc"], ["fir_interpolate_cc", "0"], ["fir_interpolate_cc", "2", "1.5"],
                 ["fir_interpolate_cc", "2", "0"], ["fir_interpolate_cc", "2", "-0.1"]):
        p = subprocess.run([CLI] + args, input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode != 0 and p.stderr, args


def test_lifecycle_flat_device_memory(ctx):
    import csdr_amd
    import torch
    rng = np.random.default_rng(14)
    x = rng.uniform(-1, 1, (64, 20000)).astype(np.float32)
    xc = (x + 1j * x).astype(np.complex64)
    taps = _taps(401, 147, 160)
    ftaps = _ftaps(ctx, 81, 4)

    def cycle():
        r = csdr_amd.Resampler(ctx, 147, 160, taps, 64, bufsize=None)
        r.process(x, [7000, 13000]); r.set_cli_bufsize(1024); r.process(x); r.close()
        p = csdr_amd.Interpolator(ctx, 4, ftaps, 64)
        p.process(xc); p.set_cli_bufsize(16384); p.process(xc); p.close()
        ctx.sync()
    for _ in range(3):
        cycle()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        cycle()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free0 - free1 <= 4 << 20, (free0, free1)


@pytest.mark.parametrize("I,D,T", [(5, 7, 3), (1, 6, 3), (2, 3, 1), (147, 160, 81), (1, 4, 81)])
def test_resampler_stream_lengths_match_one_call(ctx, I, D, T):
    """Streaming output = the reference function run once over the whole stream, output_size = n I / D cap included (it binds when
    D > (T/I + 1) I - last_taps_delay), for every stream length, whole and cut into calls."""
    import csdr_amd
    rng = np.random.default_rng(I * 31 + D + T)
    taps = _taps(T, I, D)
    x = rng.uniform(-1, 1, 7300).astype(np.float32)
    r = csdr_amd.Resampler(ctx, I, D, taps, 1)
    for n in list(range(1, 30)) + [701, 1001, 1002, 1003, 7001, 7300]:
        want, _ = rm.rational_resampler_ff(x[:n], I, D, taps)
        for calls in ([n], [n // 2, n - n // 2], [1] * min(n, 12) + [n - min(n, 12)]):
            r.reset()
            y = r.process(x[:n], calls)
            assert y.size == want.size, (n, calls[:3])
            if want.size:
                assert rm.relrms(y, want) <= TOL or np.abs(y - want).max() <= 1e-6
    r.close()


def test_cli_unit_ratio_copies_inside_chain():
    """`rational_resampler_ff 1 1` and `fractional_decimator_ff 1` copy their input (csdr.c:1427, 1494), also as a stage of `csdr chain`."""
    rng = np.random.default_rng(15)
    x = rng.uniform(-1, 1, 30011).astype(np.float32)
    for pipe in ("rational_resampler_ff 1 1 | gain_ff 1", "gain_ff 1 | rational_resampler_ff 1 1", "fractional_decimator_ff 1 | gain_ff 1"):
        p = _run(CLI, ["chain", pipe], x.tobytes())
        assert p.returncode == 0, p.stderr.decode()
        assert p.stdout == x.tobytes(), pipe
    p = _run(CLI, ["rational_resampler_ff", 1, 1], x.tobytes())
    assert p.returncode == 0 and p.stdout == x.tobytes()
