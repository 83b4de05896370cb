"""The WFM receive bank on the GPU (csdr_amd_wfmrx / csdr_amd.WfmRx): both kernel paths against the oracle's stages under the gates of wfmrx_model; the two
paths and every cut of a stream into calls, bit for bit; reset_channel; the refusals; behind the channelizer; the two commands.  The shapes are the smallest at
which a path can still go wrong: one channel, a partly filled group of the front kernel's 8 channels, two groups plus one channel; several windows and several
output tiles per call; every rate class (exact and not exact in float) and two interpolation orders."""
import os
import subprocess

import numpy as np
import pytest

import wfmrx_model as wm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
FUSED, GENERIC = "k_wfmrx_front", "k_fracdec"
GROUP = 8                                                                # channels of a workgroup of k_wfmrx_front
# (rate, P, channels, samples): 7 windows at rate 5 for 1 channel, a partly filled group and two groups plus one; 6 windows for the other rates and orders
ORACLE_CASES = [(5, 12, 1, 7300), (5, 12, GROUP - 3, 7300), (5, 12, 2 * GROUP + 1, 7300), (2.5, 12, GROUP - 3, 6200), (5.2083335, 12, GROUP - 3, 6200),
                (3.3, 12, GROUP - 3, 6200), (5, 4, GROUP - 3, 6200)]


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    assert c.arch().startswith("gfx950")
    yield c
    c.close()


_inputs, _expected = {}, {}


def case_input(n_ch, n):
    if (n_ch, n) not in _inputs:
        x = wm.make_input(n_ch, n)
        x.setflags(write=False)
        _inputs[(n_ch, n)] = x
    return _inputs[(n_ch, n)]


def case_expected(port, rate, P, n_ch, n, taps=None):
    key = (rate, P, n_ch, n, taps is not None)
    if key not in _expected:
        _expected[key] = [wm.expected(port, row, rate, P, taps) for row in case_input(n_ch, n)]
    return _expected[key]


def run(ctx, x, calls=None, generic=False, rate=5, P=12, taps=None, kernel=None, obj=None, alternate=False, **kw):
    """x [n_channels, n] through one object in calls of `calls` samples (the rest in one more) -> (s16, float audio, per-call counts).  Every count, `held` and
    `where` is checked against csdr_amd_wfmrx_plan and its restatement, every count against max_output, every call's kernel_name against `kernel` (default: the
    path asked for).  alternate: the path changes at every call, starting with `generic`."""
    import csdr_amd
    x = np.atleast_2d(x)
    n = x.shape[1]
    calls = [n] if calls is None else list(calls)
    if sum(calls) < n:
        calls.append(n - sum(calls))
    o = obj or csdr_amd.WfmRx(ctx, x.shape[0], rate=rate, num_poly_points=P, prefilter_taps=taps, max_samples_per_call=max(max(calls), 1))
    nt = 0 if taps is None else len(taps)
    try:
        pcm, af, counts, at = [], [], [], 0
        for i, k in enumerate(calls):
            g = generic ^ (alternate and i % 2 == 1)
            o.force_generic(g)
            want = o.plan(k)
            assert want == wm.plan(rate, P, nt, wm.W, o.where(), o.held(), k)
            s16, f, got = o.process(x[:, at:at + k], with_float=True, **kw)
            assert (got, o.where(), o.held()) == want and got <= o.max_output(k) == o.max_out(k)
            if k:
                assert o.kernel_name() == (kernel or (GENERIC if g else FUSED))
            pcm.append(s16); af.append(f); counts.append(got); at += k
        return np.concatenate(pcm, axis=1), np.concatenate(af, axis=1), counts
    finally:
        if obj is None:
            o.close()


def same_audio(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def same_bits(a, b):
    return same_audio(a, b) and a[2] == b[2]


def window_cuts(rate, P, n):
    """calls that each complete exactly one window: the first of W samples, then what the object is short of the next"""
    cuts, where, held, at = [], wm.fresh_where(P), 0, 0
    while at + wm.W - held <= n:
        cuts.append(wm.W - held)
        at += cuts[-1]
        _, where, held = wm.plan(rate, P, 0, wm.W, where, held, cuts[-1])
    return cuts


# ---------------------------------------------------------------- 1. both paths against the oracle
@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
@pytest.mark.parametrize("rate,P,n_ch,n", ORACLE_CASES)
def test_wfmrx_against_oracle(ctx, port, rate, P, n_ch, n, generic):
    pcm, af, counts = run(ctx, case_input(n_ch, n), generic=generic, rate=rate, P=P)
    assert counts == [wm.plan(rate, P, 0, wm.W, wm.fresh_where(P), 0, n)[0]]
    for c, (want_s16, want_af) in enumerate(case_expected(port, rate, P, n_ch, n)):
        wm.assert_gates(pcm[c], af[c], want_s16, want_af, what="%s ch %d (%s) @ %g / %d" % ("generic" if generic else "fused", c, wm.KINDS[c % 4], rate, P))


def test_wfmrx_prefilter_takes_the_generic_path(ctx, port):
    rate, n_ch, n = 5.2083335, GROUP - 3, 6200
    taps = wm.prefilter_taps(rate)
    assert taps.size == 133
    pcm, af, counts = run(ctx, case_input(n_ch, n), [2500], rate=rate, taps=taps, kernel=GENERIC)      # (not forced: the object chooses)
    assert sum(counts) == wm.plan(rate, 12, 133, wm.W, 5.0, 0, n)[0] > 0
    for c, (want_s16, want_af) in enumerate(case_expected(port, rate, 12, n_ch, n, taps)):
        wm.assert_gates(pcm[c], af[c], want_s16, want_af, what="prefilter ch %d (%s)" % (c, wm.KINDS[c % 4]))


# ---------------------------------------------------------------- 2. the two paths give the same bits, the next call's included
@pytest.mark.parametrize("rate,P,n_ch,n", ORACLE_CASES)
def test_wfmrx_paths_same_bits(ctx, rate, P, n_ch, n):
    x = case_input(n_ch, n)
    a, b = run(ctx, x, [3100], rate=rate, P=P), run(ctx, x, [3100], generic=True, rate=rate, P=P)      # three windows in the first call, the others from the carry
    assert a[2][0] > 0 and a[2][1] > 0 and same_bits(a, b)
    assert same_audio(run(ctx, x, rate=rate, P=P), a)


def test_wfmrx_paths_same_bits_with_every_cu_busy(ctx, port):
    """1024 channels x 8 windows: 128 channel groups x 7 output tiles of the one-kernel path, more than three workgroups to a compute unit.  What goes wrong only
    while many workgroups stage their rows at once shows here and not in the small cases."""
    n = 8300
    rows = wm.make_input(16, n, seed=5)
    x = np.tile(rows, (64, 1))
    a, b = run(ctx, x), run(ctx, x, generic=True)
    assert a[2] == [wm.plan(5, 12, 0, wm.W, 5.0, 0, n)[0]] and a[2][0] > 6 * 256 and same_bits(a, b)
    assert np.array_equal(a[0][:16], a[0][1008:]) and not np.array_equal(a[0][0], a[0][4])
    for c in (0, 1, 3, 4, 5, 7, 520, 1023):
        want_s16, want_af = wm.expected(port, x[c], 5)
        wm.assert_gates(a[0][c], a[1][c], want_s16, want_af, what="busy ch %d" % c)


def test_wfmrx_paths_shapes_that_leave_the_fused_kernel(ctx):
    import csdr_amd
    x = case_input(GROUP - 3, 7300)
    n = x.shape[1]
    ref = run(ctx, x, [3100], generic=True)
    odd, even = n | 1, (n + 3) & ~1
    assert same_bits(run(ctx, x, [3100], kernel=GENERIC, in_pitch=odd), ref)                # rows off 16-byte boundaries
    assert same_bits(run(ctx, x, [3100], kernel=GENERIC, in_offset=8), ref)                  # the base 8 bytes off
    assert same_bits(run(ctx, x, [3100], kernel=FUSED, in_pitch=even, in_offset=16), ref)   # (an even pitch on an aligned base stays)
    assert same_bits(run(ctx, x, [3100], kernel=FUSED, out_pitch=1501), ref)                 # an odd out_pitch: unaligned audio rows
    assert same_bits(run(ctx, x, [3100], generic=True, out_pitch=1501), ref)
    for generic in (False, True):                                                            # audio_s16 only, audio_f only
        with csdr_amd.WfmRx(ctx, GROUP - 3, max_samples_per_call=n) as o:
            o.force_generic(generic)
            s1, c1 = o.process(x[:, :3100])
            s2, c2 = o.process(x[:, 3100:])
            assert o.kernel_name() == (GENERIC if generic else FUSED)
            assert [c1, c2] == ref[2] and np.array_equal(np.concatenate([s1, s2], axis=1), ref[0])
        with csdr_amd.WfmRx(ctx, GROUP - 3, max_samples_per_call=n) as o:
            o.force_generic(generic)
            none, f1, c1 = o.process(x, with_float=True, with_s16=False)
            assert none is None and np.array_equal(f1.view(np.uint32), ref[1].view(np.uint32))


@pytest.mark.parametrize("rate", [5, 3.3])
def test_wfmrx_paths_alternate_within_a_stream(ctx, rate):
    """the held samples move between the two paths' buffers: a stream that changes path at every call has the bits of one that does not"""
    x = case_input(2 * GROUP + 1, 7300)
    ref = run(ctx, x, generic=True, rate=rate)
    calls = [341, 1500, 900, 2100, 64, 700]
    assert same_audio(run(ctx, x, calls, rate=rate, alternate=True), ref)
    assert same_audio(run(ctx, x, calls, rate=rate, alternate=True, generic=True), ref)


# ---------------------------------------------------------------- 3. any cut into calls gives the same bits
@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
@pytest.mark.parametrize("rate", [5, 5.2083335])
def test_wfmrx_cuts(ctx, rate, generic):
    x = case_input(GROUP - 3, 7300)
    one = run(ctx, x, generic=generic, rate=rate)
    per_window = window_cuts(rate, 12, x.shape[1])
    assert len(per_window) == 7
    for calls in ([341, 0, 1, 2053], per_window,
                  [wm.W],                       # a first call of exactly one window
                  [wm.W - 1, 1]):               # then held = W - 1 and one sample completes the window: its inputs are all held ones but the last
        got = run(ctx, x, calls, generic=generic, rate=rate)
        assert sum(got[2]) == one[2][0] and same_audio(got, one), calls
    assert all(c > 0 for c in run(ctx, x, per_window, generic=generic, rate=rate)[2][:7])
    assert run(ctx, x, [wm.W - 1, 1], generic=generic, rate=rate)[2][:2] == [0, 202 if rate == 5 else 194]


@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
def test_wfmrx_one_call_per_sample(ctx, generic):
    x = case_input(3, 2100)
    one = run(ctx, x, generic=generic)
    got = run(ctx, x, [1] * 2100, generic=generic)
    assert sum(got[2]) == one[2][0] == 404 and same_audio(got, one)


# ---------------------------------------------------------------- 4. reset_channel, reset
@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
def test_wfmrx_reset_channel(ctx, generic):
    import csdr_amd
    x = wm.make_input(3, 7300, seed=3)
    first = 2500                                                         # two windows out, then some hundred samples held
    undisturbed = run(ctx, x, [first], generic=generic)
    with csdr_amd.WfmRx(ctx, 3, max_samples_per_call=x.shape[1]) as o:
        a = run(ctx, x[:, :first], obj=o, generic=generic)
        assert a[2] == [404] and 0 < o.held() < wm.W
        held, where = o.held(), o.where()
        for bad in (3, -1):
            with pytest.raises(csdr_amd.CsdrAmdError, match="wfmrx: channel out of range"):
                o.reset_channel(bad)
        o.reset_channel(1)
        assert (o.held(), o.where()) == (held, where)
        b = run(ctx, x[:, first:], obj=o, generic=generic)
        # the reset channel holds zeros, its previous sample is (0, 0) and its de-emphasis state 0: so does a fresh channel fed zeros up to here (zeros demodulate
        # to exact zeros, which de-emphasise to exact zeros)
        fresh = run(ctx, np.concatenate([np.zeros((1, first), np.complex64), x[1:2, first:]], axis=1), [first], generic=generic)
        assert fresh[2] == a[2] + b[2] and not fresh[0][0, :404].any()
        assert np.array_equal(b[0][1], fresh[0][0, 404:]) and np.array_equal(b[1][1].view(np.uint32), fresh[1][0, 404:].view(np.uint32))
        for c in (0, 2):
            assert np.array_equal(np.concatenate([a[0][c], b[0][c]]), undisturbed[0][c])
            assert np.array_equal(np.concatenate([a[1][c], b[1][c]]).view(np.uint32), undisturbed[1][c].view(np.uint32))
        o.reset()
        assert (o.held(), o.where()) == (0, 5.0)
        assert same_bits(run(ctx, x, [first], obj=o, generic=generic), undisturbed)


# ---------------------------------------------------------------- 5. the refusals
def test_wfmrx_arguments(ctx):
    import csdr_amd
    for kw, msg in ((dict(rate=1.0), "wfmrx: rate should be > 1"), (dict(rate=0.3), "wfmrx: rate"), (dict(num_poly_points=11), "wfmrx: num_poly_points should be even, 2 .. 64"),
                    (dict(num_poly_points=66), "wfmrx: num_poly_points"), (dict(num_poly_points=0), "wfmrx: num_poly_points"), (dict(window=18), "wfmrx: window 18 is too short"),
                    (dict(window=150, prefilter_taps=np.ones(133, np.float32)), "wfmrx: window 150 is too short"), (dict(rate=30.0, num_poly_points=4), "wfmrx: rate 30 is too large"),
                    (dict(n_channels=0), "wfmrx: n_channels should be 1"), (dict(tau=0.0), "wfmrx: tau")):
        args = dict(n_channels=2)
        args.update(kw)
        with pytest.raises(csdr_amd.CsdrAmdError, match=msg):
            csdr_amd.WfmRx(ctx, **args)
    assert ctx.L.csdr_amd_wfmrx_create(ctx.h, 2, 1.0, 12, None, 0, 0, 50e-6, 48000, 4096) is None
    x = wm.make_input(2, 4096)
    with ctx.wfm_rx(2, max_samples_per_call=3000, window=0) as o:         # window 0: 1024
        di, ds = ctx.upload(x), ctx.alloc(2 * 2 * 4096 + 256)
        assert ctx.L.csdr_amd_wfmrx_process(o.h, di.ptr, 4096, 3001, ds.ptr, None, 4096) == -3 and "wfmrx: n_in should be 0 .. max_samples_per_call (3000)" in ctx.err()
        assert ctx.L.csdr_amd_wfmrx_process(o.h, di.ptr, 4096, 3000, ds.ptr, None, 403) == -3 and "wfmrx: out_pitch 403 smaller than the 404 audio samples" in ctx.err()
        assert (o.held(), o.where()) == (0, 5.0)                         # a refused call changes nothing
        assert o.process_dev(di.ptr, 4096, 0, ds.ptr, None, 0) == 0 and (o.held(), o.where()) == (0, 5.0)
        assert o.process_dev(di.ptr, 4096, 3000, ds.ptr, None, 404) == 404
        assert o.max_output(3000) >= 404 and o.max_out(3000) == o.max_output(3000) and o.max_output(0) == 0
    with ctx.wfm_rx(1, max_samples_per_call=4096) as o:                  # one channel: the row is as long as the caller says
        assert o.process_dev(ctx.upload(x[0]).ptr, 0, 3000, ctx.alloc(2 * 4096).ptr, None, 0) == 404
    with ctx.wfm_rx(1, rate=3, num_poly_points=2, max_samples_per_call=4096) as o:      # two points: the first output's window starts at sample -1, which reads as 0
        a = o.process(x[0], with_float=True)
        o.reset(); o.force_generic(True)
        b = o.process(x[0], with_float=True)
        assert a[2] == b[2] > 0 and same_audio(a, b)


# ---------------------------------------------------------------- 6. behind the channelizer
def bank_input(n, seed=77):
    """one FM signal at -0.1 of the wide rate (deviation 0.02 cycles per wide sample, 0.04 per decimated one) for channels tuned at and beside it: every channel
    sees a constant envelope, as the gates need"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return (wm.fm_baseband(rng, n, dev=0.02) * np.exp(-2j * np.pi * 0.1 * t)).astype(np.complex64)


def test_wfmrx_behind_the_channelizer(ctx, port):
    """WfmRx on ctx.fastddc_bank rows at the smallest channelizer geometry (transition_bw 0.05, decimation 2: fft 1024), call by call with the bank's counts,
    against the oracle chain on the bank's own output rows"""
    D, tbw, rates = 2, 0.05, [0.1, 0.104, 0.097]
    ddc, _ = ctx.fastddc_init(tbw, D, 0.0)
    x = bank_input(16 * ddc.input_size)
    out, y, counts = wm.bank_composition(ctx, x, tbw, D, rates, 4, 5)
    assert len(counts) == 4 and sum(counts) >= 6 * wm.W
    got = np.concatenate(out, axis=1)
    for c in range(3):
        want_s16, want_af = wm.expected(port, y[c][:sum(counts)], 5)
        d = np.abs(got[c].astype(np.int32) - want_s16.astype(np.int32))
        print("bank ch %d: %d samples, s16 max diff %d, differing %.4f %%" % (c, want_s16.size, d.max(), 100 * (d > 0).mean()))
        assert got[c].shape == want_s16.shape and want_s16.size > 1000 and np.abs(want_s16).max() > 1000
        assert d.max() <= 1 and (d > 0).mean() < wm.S16_FRACTION
    with ctx.wfm_rx(3, max_samples_per_call=sum(counts)) as o:           # the float audio too, in one call
        s16, af, n_out = o.process(np.stack([row[:sum(counts)] for row in y]), with_float=True)
        assert np.array_equal(s16, got)
        for c in range(3):
            want_s16, want_af = wm.expected(port, y[c][:sum(counts)], 5)
            wm.assert_gates(s16[c], af[c], want_s16, want_af, what="bank ch %d" % c)


# ---------------------------------------------------------------- 7. the two commands
def read_exactly(fd, nbytes, seconds=60):
    """nbytes from a descriptor whose other end a child process writes: a bounded wait per piece, never an open-ended one"""
    import select
    buf = b""
    while len(buf) < nbytes:
        ready, _, _ = select.select([fd], [], [], seconds)
        assert ready, "no output within %d s (%d of %d bytes)" % (seconds, len(buf), nbytes)
        piece = os.read(fd, nbytes - len(buf))
        assert piece, "the output ended after %d of %d bytes" % (len(buf), nbytes)
        buf += piece
    return buf


def test_wfmrx_cli_bank_equals_python_composition(ctx, tmp_path):
    """`csdr fastddc_wfm_bank_s16` on 3 channels at the smallest channelizer geometry against ctx.fastddc_bank -> WfmRx with the same blocks per call
    (wfmrx_model.bank_composition), byte for byte.  Channel 0's audio goes to a fifo: once the first batch's bytes have arrived the command is waiting for input,
    and the retune and reset lines written then are applied in front of the second batch, as they are in the composition.  The composition runs in a Python
    process of its own without torch (as tests/test_fmrx_gpu.py explains: the command links the system's hipFFT, a process with torch runs torch's copy)."""
    import math
    import sys
    assert os.path.exists(CSDR), "csdr_amd/csdr not built (make -C csdr_amd/csrc)"
    D, tbw, rates = 2, 0.05, [0.1, 0.104, 0.097]
    ddc, _ = ctx.fastddc_init(tbw, D, 0.0)
    inp = ddc.input_size
    per = 1024 // math.gcd(inp, 1024)                                    # blocks per call: the command takes CSDR_AMD_BLOCK in multiples of 1024 samples
    x = bank_input(2 * per * inp)
    env = {k: v for k, v in os.environ.items() if k != "CSDR_AMD_WORLD"}
    np.savez(str(tmp_path / "in.npz"), x=x, tbw=tbw, decimation=D, rates=rates, per=per, frac_rate=5.0, retune_channel=1, retune_rate=0.101, reset_channel=2)
    c = subprocess.run(["timeout", "-k", "5", "90", sys.executable, os.path.join(ROOT, "tests", "wfmrx_model.py"), str(tmp_path / "in.npz"), str(tmp_path / "want.npz")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, CSDR_AMD_NO_TORCH_PRELOAD="1"), timeout=120)
    assert c.returncode == 0, c.stderr.decode()
    w = np.load(str(tmp_path / "want.npz"))
    want = [w["first"], w["second"]]
    assert not w["torch_loaded"]
    assert want[0].shape[1] > 0 and want[1].shape[1] > 0 and want[0].shape[1] + want[1].shape[1] >= 1000
    outs = [str(tmp_path / ("audio%d" % k)) for k in range(3)]
    ctl = str(tmp_path / "ctl")
    os.mkfifo(outs[0]); os.mkfifo(ctl)
    fo, fc = os.open(outs[0], os.O_RDWR | os.O_NONBLOCK), os.open(ctl, os.O_RDWR | os.O_NONBLOCK)      # (both ends held here: neither side's open waits for the other)
    args = ["timeout", "-k", "5", "90", CSDR, "fastddc_wfm_bank_s16", D, tbw, "HAMMING", 5, 48000, "50e-6", ctl]
    for path, r in zip(outs, rates):
        args += [path, r]
    p = subprocess.Popen([str(a) for a in args], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, CSDR_AMD_BLOCK=str(per * inp)))
    try:
        p.stdin.write(x[:per * inp].tobytes()); p.stdin.flush()
        first = read_exactly(fo, 2 * want[0].shape[1])
        os.write(fc, b"1 0.101\n2 reset\n")
        p.stdin.write(x[per * inp:].tobytes()); p.stdin.close()
        second = read_exactly(fo, 2 * want[1].shape[1])
        assert p.wait(timeout=60) == 0, p.stderr.read().decode()
        err = p.stderr.read().decode()
    finally:
        if p.poll() is None:
            p.kill(); p.wait(timeout=10)
        os.close(fo); os.close(fc)
    assert "channel 1 retuned to 0.101" in err and "channel 2 reset" in err
    want_all = np.concatenate(want, axis=1)
    assert first + second == want_all[0].tobytes()
    for k in (1, 2):
        assert open(outs[k], "rb").read() == want_all[k].tobytes(), k
    # without the two lines channels 1 and 2 differ from this: the lines did something
    plain = w["plain"]
    assert np.array_equal(plain[0], want_all[0]) and not np.array_equal(plain[1], want_all[1]) and not np.array_equal(plain[2], want_all[2])


def test_wfmrx_cli_single_stream_world_refusal_and_usage(ctx, tmp_path):
    import csdr_amd
    assert os.path.exists(CSDR), "csdr_amd/csdr not built (make -C csdr_amd/csrc)"
    x = case_input(1, 7300)[0]
    env = dict(os.environ, CSDR_AMD_BLOCK="4096")
    for rate in (5, 5.2083335):
        p = subprocess.run(["timeout", "-k", "5", "90", CSDR, "wfm_rx_cc_s16", repr(rate)], input=x.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
        assert p.returncode == 0, p.stderr.decode()
        with csdr_amd.WfmRx(ctx, 1, rate=rate, max_samples_per_call=x.size) as o:
            want = o.process(x)[0][0]
        assert want.size >= 1300 and p.stdout == want.tobytes()
    p = subprocess.run(["timeout", "-k", "5", "90", CSDR, "wfm_rx_cc_s16"], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode != 0 and "usage: wfm_rx_cc_s16 <rate> [audio_rate [tau [num_poly_points [--prefilter [transition_bw [window]]]]]]" in p.stderr.decode()
    bank = ["timeout", "-k", "5", "90", CSDR, "fastddc_wfm_bank_s16", "2", "0.05", "HAMMING", "5", "48000", "50e-6", "-", str(tmp_path / "a")]
    p = subprocess.run(bank + ["0.1"], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, CSDR_AMD_WORLD="1"), timeout=120)
    assert p.returncode != 0 and "fastddc_wfm_bank_s16: runs on one GPU only: CSDR_AMD_WORLD is set" in p.stderr.decode()
    assert not os.path.exists(str(tmp_path / "a"))
    p = subprocess.run(bank, input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={k: v for k, v in os.environ.items() if k != "CSDR_AMD_WORLD"}, timeout=120)
    assert p.returncode != 0 and "usage: fastddc_wfm_bank_s16 <decimation> <transition_bw> <window> <frac_rate> <audio_rate> <tau> <ctl|-> <out_0> <rate_0>" in p.stderr.decode()
