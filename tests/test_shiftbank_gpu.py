"""The shifter bank on the GPU (csdr_amd_shiftbank): every stream against the library's own shared-rate path by bits -- the same device functions, the same
operations in the same order: nothing to tolerate -- and against the CPU oracle at the shifters' gates of tests/test_gpu_parity.py; invariance under the
cuts into calls, the shared input row, real input, retunes, the state round trip, the scan that runs ahead, arguments and the command line."""
import os
import subprocess
import numpy as np
import pytest
from oracle import relrms
import shiftbank_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "csdr_amd", "csdr")
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "csdr")
c64, f32 = np.complex64, np.float32
TOL = 1e-5
CUTS = (1, 63, 1000, 0, 961)
N = 2 * 1024 + 17
SMAX = 65
STREAMS = [1, 3, 65]
# (variant, chunk, aux)
CONFIGS = [("addition", 1024, 0), ("addition", 100, 0), ("math", 1024, 0), ("table", 1024, 65536), ("table", 1024, 16)]
TILED = {"addition": "k_shiftbank_addition", "math": "k_shiftbank_math", "table": "k_shiftbank_table"}


@pytest.fixture(scope="module")
def gpu():
    import torch  # noqa: F401  (loads the HIP runtime torch bundles first, as bench.py does)
    import csdr_amd
    ctx = csdr_amd.Context(0)
    assert ctx.arch().startswith("gfx950")
    yield ctx
    ctx.close()


def rate_of(s): return M.RATES[s % len(M.RATES)]
def phase_of(variant, s): return f32(-3.0 + 0.09 * s) if variant == "addition" else f32(0.1 + 0.09 * s)


X = (lambda rng: (rng.uniform(-1, 1, (SMAX, N)) + 1j * rng.uniform(-1, 1, (SMAX, N))).astype(c64))(np.random.default_rng(31))
XR = np.random.default_rng(32).uniform(-1, 1, (SMAX, N)).astype(f32)
_want = {}


def want(gpu, variant, chunk, aux):
    """the shared-rate path, one call per stream: ([SMAX, N] outputs, [SMAX] end phases); computed once per configuration and left unchanged"""
    key = (variant, chunk, aux)
    if key not in _want:
        y, p = np.zeros((SMAX, N), c64), np.zeros(SMAX, f32)
        for s in range(SMAX):
            y[s], p[s] = gpu.shift_cc(X[s], rate_of(s), variant, phase=float(phase_of(variant, s)), chunk=chunk, aux=aux)
        y.setflags(write=False); p.setflags(write=False)
        _want[key] = (y, p)
    return _want[key]


def make(gpu, variant, chunk, aux, streams, generic=False, in_format="cf32", start=True):
    import csdr_amd
    b = csdr_amd.ShiftBank(gpu, variant, [rate_of(s) for s in range(streams)], chunk=chunk, aux=aux, in_format=in_format, max_samples_per_call=4096)
    if start:
        for s in range(streams):
            st = b.get_channel(s)
            st.phase = phase_of(variant, s)
            b.set_channel(s, st)
    b.force_generic(generic)
    return b


def bits(a): return np.ascontiguousarray(a).view(np.uint32)
def end_phases(b, variant, streams): return np.array([M.end_phase(variant, b.get_channel(s)) for s in range(streams)], f32)


def oracle_call(port, variant, x, rate, chunk, aux, phase):
    if variant == "addition":
        return port.shift_addition_cc(x, rate, chunk=chunk, phase=phase)
    if variant == "math":
        return port.shift_math_cc(x, rate, phase=phase)
    return port.shift_table_cc(x, rate, table_size=aux, phase=phase)


def at_oracle_gates(y, p, o, po, variant):
    e, dp = relrms(y, o), abs(float(p) - float(po))
    print(variant, "relrms", e, "end phase off by", dp)
    assert e < (1e-6 if variant == "addition" else TOL)
    assert dp < (1e-6 if variant == "addition" else 1e-5)


@pytest.mark.parametrize("streams", STREAMS)
@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("variant,chunk,aux", CONFIGS)
def test_bits_against_the_shared_rate_path(gpu, port, variant, chunk, aux, generic, streams):
    wy, wp = want(gpu, variant, chunk, aux)
    with make(gpu, variant, chunk, aux, streams, generic) as b:
        y = b.process(X[:streams])
        assert b.kernel_name() == ("k_shiftbank_generic" if generic else TILED[variant])
        p = end_phases(b, variant, streams)
    for s in range(streams):
        assert np.array_equal(bits(y[s]), bits(wy[s])), s
        assert p[s] == wp[s], s
    for s in sorted({0, min(1, streams - 1), streams - 1}):
        o, po = oracle_call(port, variant, X[s], rate_of(s), chunk, aux, float(phase_of(variant, s)))
        at_oracle_gates(y[s], p[s], o, po, variant)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("variant,chunk,aux", CONFIGS)
def test_cut_invariance(gpu, variant, chunk, aux, generic):
    wy, wp = want(gpu, variant, chunk, aux)
    with make(gpu, variant, chunk, aux, SMAX, generic) as b:
        y = b.process(X, calls=CUTS + (N - sum(CUTS),))
        assert b.kernel_name() == ("k_shiftbank_generic" if generic else TILED[variant])
        assert np.array_equal(bits(y), bits(wy))
        assert np.array_equal(end_phases(b, variant, SMAX), wp)
        with make(gpu, variant, chunk, aux, SMAX, generic) as one:
            one.process(X)
            for s in (0, 1, 7, SMAX - 1):
                assert bytes(one.get_channel(s)) == bytes(b.get_channel(s)), s


@pytest.mark.parametrize("variant,chunk,aux", CONFIGS[:4])
def test_shared_input_row(gpu, variant, chunk, aux):
    with make(gpu, variant, chunk, aux, SMAX) as a, make(gpu, variant, chunk, aux, SMAX) as b:
        ya, yb = a.process(X[5]), b.process(np.repeat(X[5][None], SMAX, 0))
        assert np.array_equal(bits(ya), bits(yb))
        wy, _ = want(gpu, variant, chunk, aux)
        assert np.array_equal(bits(ya[5]), bits(wy[5]))


@pytest.mark.parametrize("generic", [False, True])
def test_real_input(gpu, generic):
    import csdr_amd
    with make(gpu, "addition", 1024, 0, SMAX, generic, in_format="f32") as b:
        y = b.process(XR)
        p = end_phases(b, "addition", SMAX)
    for s in range(SMAX):
        w, wp = gpu.shift_addition_fc(XR[s], rate_of(s), phase=float(phase_of("addition", s)))
        assert np.array_equal(bits(y[s]), bits(w)) and p[s] == f32(wp), s
    for variant in ("math", "table"):
        with pytest.raises(csdr_amd.CsdrAmdError, match="ADDITION only"):
            csdr_amd.ShiftBank(gpu, variant, [0.1], in_format="f32")


@pytest.mark.parametrize("at", [1024 + 300, 2048])
@pytest.mark.parametrize("variant,chunk,aux", [CONFIGS[0], CONFIGS[2], CONFIGS[3]])
def test_retune(gpu, variant, chunk, aux, at):
    """a set_rate mid-chunk and on a chunk boundary against the shared-rate path called piecewise with the phase carried, by bits; the other streams go on as
    if nothing had happened"""
    wy, wp = want(gpu, variant, chunk, aux)
    retuned = {2: 0.3141, 64: -0.5, 7: 1e-7}
    with make(gpu, variant, chunk, aux, SMAX) as b:
        y1 = b.process(X[:, :at])
        for s, r in retuned.items():
            b.set_rate(s, r)
            assert b.get_rate(s) == f32(r)
        y2 = b.process(X[:, at:])
        y = np.concatenate([y1, y2], 1)
        p = end_phases(b, variant, SMAX)
        for s in retuned:
            st = b.get_channel(s)
            assert st.pending == 0 and st.rate == f32(retuned[s]) and st.pos == ((N - at) % chunk if variant == "addition" else 0)
    for s in range(SMAX):
        if s in retuned:
            a1, p1 = gpu.shift_cc(X[s, :at], rate_of(s), variant, phase=float(phase_of(variant, s)), chunk=chunk, aux=aux)
            a2, p2 = gpu.shift_cc(X[s, at:], retuned[s], variant, phase=p1, chunk=chunk, aux=aux)
            assert np.array_equal(bits(y[s]), bits(np.concatenate([a1, a2]))) and p[s] == f32(p2), s
        else:
            assert np.array_equal(bits(y[s]), bits(wy[s])) and p[s] == wp[s], s


@pytest.mark.parametrize("variant,chunk,aux", CONFIGS[:4])
def test_state_round_trip(gpu, variant, chunk, aux):
    wy, wp = want(gpu, variant, chunk, aux)
    half = 1024 + 211
    with make(gpu, variant, chunk, aux, SMAX) as a, make(gpu, variant, chunk, aux, SMAX, start=False) as b:
        y1 = a.process(X[:, :half])
        for s in range(SMAX):
            b.set_channel(s, a.get_channel(s))
        y2 = b.process(X[:, half:])
        assert np.array_equal(bits(np.concatenate([y1, y2], 1)), bits(wy))
        assert np.array_equal(end_phases(b, variant, SMAX), wp)


@pytest.mark.parametrize("variant,aux", [("math", 0), ("table", 65536)])
def test_scan_ahead(gpu, variant, aux):
    """four calls of equal length: the last three find their scan done; another length, or a set_rate in between, scans in the call"""
    import csdr_amd
    n = 256
    x = np.tile(X[:, :2 * n], 3)                         # [SMAX, 6 n]
    with make(gpu, variant, 1024, aux, SMAX) as b:
        y = b.process(x, calls=(n, n, n, n))
        assert b.scans_ahead() == 3
        y5 = b.process(x[:, 4 * n:4 * n + 100])
        assert b.scans_ahead() == 3
        y6 = b.process(x[:, 4 * n + 100:4 * n + 200])
        assert b.scans_ahead() == 4
        b.set_rate(3, rate_of(3))                        # the same rate again: still a retune
        y7 = b.process(x[:, 4 * n + 200:4 * n + 300])
        assert b.scans_ahead() == 4
        got = np.concatenate([y[:, :4 * n], y5, y6, y7], 1)
        p = end_phases(b, variant, SMAX)
    for s in range(SMAX):
        w, wp = gpu.shift_cc(x[s, :got.shape[1]], rate_of(s), variant, phase=float(phase_of(variant, s)), aux=aux)
        assert np.array_equal(bits(got[s]), bits(w)) and p[s] == f32(wp), s
    with csdr_amd.ShiftBank(gpu, "addition", [0.1, 0.2]) as a:
        a.process(X[:2, :512], calls=(256, 256))
        assert a.scans_ahead() == 0


@pytest.mark.parametrize("variant,chunk,aux", CONFIGS)
def test_gpu_against_the_cpu_walk(gpu, variant, chunk, aux):
    """not bit equality: the device's and the host's double cos need not round alike"""
    import csdr_amd
    wy, wp = want(gpu, variant, chunk, aux)
    for s in (0, 1, SMAX - 1):
        st = csdr_amd.ShiftBankChan(rate=rate_of(s), phase=phase_of(variant, s), c=1.0, s=0.0, pos=0, pending=0, old_rate=rate_of(s), pad=0)
        y = csdr_amd.shiftbank_debug_walk(variant, rate_of(s), X[s], chunk=chunk, aux=aux, state=st)
        at_oracle_gates(wy[s], wp[s], y, M.end_phase(variant, st), variant)


def test_arguments_and_lifecycle(gpu):
    import csdr_amd
    L = csdr_amd.lib()
    r = np.array([0.1, 0.2], f32)
    rp = r.ctypes.data
    assert L.csdr_amd_shiftbank_create(None, 0, 2, rp, 1024, 0, 0, 4096) is None and b"null context" in L.csdr_amd_last_error()
    assert L.csdr_amd_shiftbank_create(gpu.h, 0, 0, rp, 1024, 0, 0, 4096) is None and b"n_streams" in L.csdr_amd_last_error()
    for variant in ("unroll", "addfast"):
        with pytest.raises(csdr_amd.CsdrAmdError, match="one rate per call"):
            csdr_amd.ShiftBank(gpu, variant, r)
    with pytest.raises(csdr_amd.CsdrAmdError, match="chunk"):
        csdr_amd.ShiftBank(gpu, "addition", r, chunk=0)
    b = csdr_amd.ShiftBank(gpu, "addition", r, max_samples_per_call=1000)
    with pytest.raises(csdr_amd.CsdrAmdError, match="max_samples_per_call"):
        b.process(X[:2, :1001])
    assert b.process(X[:2, :0]).shape == (2, 0)
    for call in (lambda: b.set_rate(2, 0.1), lambda: b.set_rate(-1, 0.1), lambda: b.get_rate(2), lambda: b.get_channel(2), lambda: b.reset_channel(5)):
        with pytest.raises(csdr_amd.CsdrAmdError, match="out of range"):
            call()
    y = b.process(X[:2, :1000])
    b.reset()
    assert np.array_equal(bits(b.process(X[:2, :1000])), bits(y))
    b.process(X[:2, :300]); b.reset_channel(1)
    z = b.process(X[:2, :1000])
    assert np.array_equal(bits(z[1]), bits(y[1])) and not np.array_equal(bits(z[0]), bits(y[0]))
    b.close(); b.close()
    with csdr_amd.ShiftBank(gpu, "math", r) as m:
        m.process(X[:2, :100])
    assert m.h is None
    # an object that is still open when its context closes is dropped, not destroyed
    ctx2 = csdr_amd.Context(0)
    left = csdr_amd.ShiftBank(ctx2, "table", r)
    left.process(X[:2, :100])
    ctx2.sync(); ctx2.close()
    left.close()


def run_cli(args, data, pass_fds=()):
    assert os.path.exists(CLI), "csdr_amd/csdr not built (make -C csdr_amd/csrc)"
    p = subprocess.run([CLI] + [str(a) for a in args], input=np.ascontiguousarray(data).tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                       pass_fds=pass_fds)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout


def test_cli(tmp_path):
    rng = np.random.default_rng(33)
    x = (rng.uniform(-1, 1, 5 * 1024 + 100) + 1j * rng.uniform(-1, 1, 5 * 1024 + 100)).astype(c64)
    rates = [-0.085, 0.3141, 4e-4]
    outs = [str(tmp_path / ("out%d" % k)) for k in range(3)]
    run_cli(["shift_bank_cc", "addition", "-"] + [v for k in range(3) for v in (outs[k], rates[k])], x)
    single = [run_cli(["shift_addition_cc", r], x) for r in rates]
    bank_out = [open(o, "rb").read() for o in outs]
    for k in range(3):
        assert bank_out[k] == single[k], k
    # a control line that is there before the stream starts: channel 1 runs at that rate from the first sample
    ctl = tmp_path / "ctl"
    ctl.write_text("1 0.25\n")
    run_cli(["shift_bank_cc", "addition", str(ctl)] + [v for k in range(3) for v in (outs[k], rates[k])], x)
    assert open(outs[1], "rb").read() == run_cli(["shift_addition_cc", 0.25], x)
    assert open(outs[0], "rb").read() == single[0] and open(outs[2], "rb").read() == single[2]
    run_cli(["shift_bank_cc", "table:4096", "-", outs[0], rates[1]], x)
    assert open(outs[0], "rb").read() == run_cli(["shift_table_cc", rates[1], 4096], x)
    if os.path.exists(REF_CLI):                          # the reference binary writes whole buffers: it pads the stream's ragged end, and the stream's part is compared
        for k in range(3):
            p = subprocess.run([REF_CLI, "shift_addition_cc", str(rates[k])], input=x.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            ref = np.frombuffer(p.stdout, c64)
            assert ref.size >= x.size
            assert relrms(np.frombuffer(bank_out[k], c64), ref[:x.size]) < 1e-6, k
