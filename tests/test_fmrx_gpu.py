"""The FM receive bank on the GPU (csdr_amd_fmrx / csdr_amd.FmRx): both kernel paths against the oracle's stages under the chain's gates; the two paths, every
cut of a stream into calls, and csdr_amd_nfm on the same u8 input, bit for bit; reset_channel; the refusals; the two commands.  The shapes are the smallest at
which a path can still go wrong: one channel, a partly filled 16-row group, two groups plus one channel; several spans per call; every tap count."""
import os
import subprocess

import numpy as np
import pytest

import fmrx_model as fm
from tests_helpers import nfm_signal_u8

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
FUSED, GENERIC = "k_fmrx_front", "k_nfm_deemph_mfma"
ORACLE_CASES = [(48000, 1, 7), (48000, 17, 7), (48000, 33, 7), (44100, 17, 6), (8000, 17, 6), (11025, 17, 6)]      # (audio rate, channels, blocks of 1024)


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    assert c.arch().startswith("gfx950")
    yield c
    c.close()


_inputs, _expected = {}, {}


def case_input(rate, n_ch, blocks):
    key = (rate, n_ch, blocks)
    if key not in _inputs:
        x = fm.make_input(n_ch, fm.n_for_blocks(blocks, fm.taps_of(rate).size))
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]


def case_expected(port, rate, n_ch, blocks):
    key = (rate, n_ch, blocks)
    if key not in _expected:
        taps = fm.taps_of(rate)
        _expected[key] = [fm.expected(port, row, taps) for row in case_input(rate, n_ch, blocks)]
    return _expected[key]


def run(ctx, x, calls=None, generic=False, rate=48000, block=1024, kernel=None, obj=None, **kw):
    """x [n_channels, n] through one object in calls of `calls` samples (the rest in one more) -> (s16, float audio, per-call counts).  Every count is checked
    against csdr_amd_fmrx_plan and max_output, every call's kernel_name against `kernel` (default: the path asked for)."""
    import csdr_amd
    x = np.atleast_2d(x)
    n = x.shape[1]
    calls = [n] if calls is None else list(calls)
    if sum(calls) < n:
        calls.append(n - sum(calls))
    o = obj or csdr_amd.FmRx(ctx, x.shape[0], audio_rate=rate, agc_block=block, max_samples_per_call=max(max(calls), 1))
    try:
        o.force_generic(generic)
        pcm, af, counts, at = [], [], [], 0
        for k in calls:
            want = csdr_amd.fmrx_plan(o.fill(), k, o.taps_length, block)
            assert want == fm.plan(o.fill(), k, o.taps_length, block)
            s16, f, got = o.process(x[:, at:at + k], with_float=True, **kw)
            assert (got, o.fill()) == want and got <= o.max_output(k)
            if k:
                assert o.kernel_name() == (kernel or (GENERIC if generic else FUSED))
            pcm.append(s16); af.append(f); counts.append(got); at += k
        return np.concatenate(pcm, axis=1), np.concatenate(af, axis=1), counts
    finally:
        if obj is None:
            o.close()


def same_bits(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[2] == b[2]


# ---------------------------------------------------------------- 1. both paths against the oracle
@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
@pytest.mark.parametrize("rate,n_ch,blocks", ORACLE_CASES)
def test_fmrx_against_oracle(ctx, port, rate, n_ch, blocks, generic):
    x = case_input(rate, n_ch, blocks)
    pcm, af, counts = run(ctx, x, generic=generic, rate=rate)
    assert counts == [blocks * 1024]
    for c, (want_s16, want_af) in enumerate(case_expected(port, rate, n_ch, blocks)):
        fm.assert_gates(pcm[c], af[c], want_s16, want_af, what="%s ch %d (%s) @ %d" % ("generic" if generic else "fused", c, fm.KINDS[c % 4], rate))


# ---------------------------------------------------------------- 2. the two paths give the same bits, the next call's included
@pytest.mark.parametrize("rate,n_ch,blocks", ORACLE_CASES)
def test_fmrx_paths_same_bits(ctx, rate, n_ch, blocks):
    x = case_input(rate, n_ch, blocks)
    first = fm.n_for_blocks(3, fm.taps_of(rate).size, extra=5)          # three spans in the first call, the others from the carry in the second
    a, b = run(ctx, x, [first], rate=rate), run(ctx, x, [first], generic=True, rate=rate)
    assert a[2] == [3 * 1024, (blocks - 3) * 1024] and same_bits(a, b)


def test_fmrx_paths_same_bits_with_every_cu_busy(ctx):
    """512 channels x 24 spans: 768 workgroups of the one-kernel path, three to a compute unit.  What goes wrong only while many workgroups stage their rows
    at once shows here and not in the small cases (an earlier form of the staging, byte stores by neighbouring lanes into one LDS word, lost some at this size)."""
    ld = fm.taps_of(48000).size
    rows = fm.make_input(16, fm.n_for_blocks(24, ld), seed=5)
    x = np.tile(rows, (32, 1))
    a, b = run(ctx, x), run(ctx, x, generic=True)
    assert a[2] == [24 * 1024] and same_bits(a, b)
    assert np.array_equal(a[0][:16], a[0][496:]) and not np.array_equal(a[0][0], a[0][1])


def test_fmrx_paths_shapes_that_leave_the_fused_kernel(ctx):
    import csdr_amd
    x = case_input(48000, 17, 7)
    n = x.shape[1]
    first = fm.n_for_blocks(3, fm.taps_of(48000).size, extra=5)
    ref = run(ctx, x, [first], generic=True)
    odd, even = n | 1, (n + 3) & ~1
    assert same_bits(run(ctx, x, [first], kernel=GENERIC, in_pitch=odd), ref)               # rows off 16-byte boundaries
    assert same_bits(run(ctx, x, [first], kernel=GENERIC, in_offset=8), ref)                 # the base 8 bytes off
    assert same_bits(run(ctx, x, [first], kernel=FUSED, in_pitch=even, in_offset=16), ref)  # (an even pitch on an aligned base stays)
    b512 = run(ctx, x, [first], kernel=GENERIC, block=512)                                   # an AGC block that is not the span
    assert same_bits(b512, run(ctx, x, [first], generic=True, block=512)) and sum(b512[2]) == 7 * 1024
    for generic in (False, True):                                                            # audio_s16 only
        with csdr_amd.FmRx(ctx, 17, max_samples_per_call=n) as o:
            o.force_generic(generic)
            s1, c1 = o.process(x[:, :first])
            s2, c2 = o.process(x[:, first:])
            assert o.kernel_name() == (GENERIC if generic else FUSED)
            assert [c1, c2] == ref[2] and np.array_equal(np.concatenate([s1, s2], axis=1), ref[0])
        with csdr_amd.FmRx(ctx, 17, max_samples_per_call=n) as o:                            # audio_f only
            o.force_generic(generic)
            _, f1, c1 = o.process(x, with_float=True, with_s16=False)
            assert np.array_equal(f1.view(np.uint32), ref[1].view(np.uint32))


def test_fmrx_paths_alternate_within_a_stream(ctx):
    """the held input moves between the two paths' buffers: a stream that changes path at every call has the bits of one that does not"""
    import csdr_amd
    x = case_input(48000, 17, 7)
    ref = run(ctx, x, generic=True)
    calls = [341, 1500, 900, 2100, 64]
    with csdr_amd.FmRx(ctx, 17, max_samples_per_call=x.shape[1]) as o:
        pcm, at = [], 0
        for i, k in enumerate(calls + [x.shape[1] - sum(calls)]):
            o.force_generic(i % 2 == 1)
            s16, f, got = o.process(x[:, at:at + k], with_float=True)
            pcm.append((s16, f)); at += k
        assert np.array_equal(np.concatenate([p[0] for p in pcm], axis=1), ref[0])
        assert np.array_equal(np.concatenate([p[1] for p in pcm], axis=1).view(np.uint32), ref[1].view(np.uint32))


# ---------------------------------------------------------------- 3. any cut into calls gives the same bits
@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
def test_fmrx_cuts(ctx, generic):
    x = case_input(48000, 17, 7)
    n, ld = x.shape[1], fm.taps_of(48000).size
    one = run(ctx, x, generic=generic)
    for calls in ([341, 0, 1, 2053], [1024] * (n // 1024),
                  [ld + 1023, 1],              # then fill = taps + agc_block - 1 and one sample completes a block: its inputs are almost all held ones
                  [ld]):                       # a first call of exactly the taps: one block, the held / new boundary inside the window tail
        got = run(ctx, x, calls, generic=generic)
        assert sum(got[2]) == 7 * 1024 and np.array_equal(got[0], one[0]) and np.array_equal(got[1].view(np.uint32), one[1].view(np.uint32)), calls
    assert run(ctx, x, [ld + 1023, 1], generic=generic)[2][:2] == [1024, 1024] and run(ctx, x, [ld], generic=generic)[2][0] == 1024


@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
def test_fmrx_one_call_per_sample(ctx, generic):
    x = case_input(48000, 1, 7)
    one = run(ctx, x, generic=generic)
    got = run(ctx, x, [1] * 300, generic=generic)
    assert np.array_equal(got[0], one[0]) and np.array_equal(got[1].view(np.uint32), one[1].view(np.uint32))


# ---------------------------------------------------------------- 4. on the front end's rows: csdr_amd_nfm's bits
@pytest.mark.parametrize("n_streams", [3, 19])
def test_fmrx_on_ddc_rows_equals_nfm_chain(ctx, n_streams):
    """csdr_amd_ddc_process is csdr_amd_nfm's front end without the fused epilogue; its rows through FmRx, call by call, are the chain object's audio.
    The calls are [1024 * 60, 1024 * 37 + 512 * 2, the rest]: the front end takes a call that is not a multiple of 1024 samples only as a stream's last one (a
    middle call of 1024 * 37 + 512 is refused by csdr_amd_nfm_process itself), and 50 divides none of the three, so every call ends between two decimated samples
    and the rows handed over are 1228, 779 and 1049 samples long."""
    n = 1024 * 150
    calls = [1024 * 60, 1024 * 37 + 512 * 2]
    u8 = np.stack([nfm_signal_u8(8000 + s, n) for s in range(n_streams)])
    want_s16, want_f = ctx.nfm_chain(u8, -0.11, block=calls)
    taps = np.ascontiguousarray(ctx.firdes_lowpass_f(ctx.firdes_filter_len(0.005), 0.5 / 50), np.float32)
    y = ctx.ddc_u8(u8, -0.11, 50, taps, block=calls)
    # what the front end had written after each call: the same stream, ended there
    ends = [ctx.ddc_u8(u8[:, :2 * sum(calls[:k])], -0.11, 50, taps, block=calls[:k]).shape[1] for k in (1, 2)]
    assert 0 < ends[0] < ends[1] < y.shape[1]
    for generic in (False, True):
        got = run(ctx, y, [ends[0], ends[1] - ends[0]], generic=generic)
        assert got[0].shape == want_s16.shape and want_s16.shape[1] >= 2 * 1024
        assert np.array_equal(got[0], want_s16) and np.array_equal(got[1].view(np.uint32), want_f.view(np.uint32))


# ---------------------------------------------------------------- 5. reset_channel, reset
@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
def test_fmrx_reset_channel(ctx, generic):
    import csdr_amd
    x = fm.make_input(3, 2 * 1024 + 100 + 5 * 1024, seed=3)
    first = 2 * 1024 + 100                                               # two blocks out, then 1024 + 100 samples held
    undisturbed = run(ctx, x, [first], generic=generic)
    with csdr_amd.FmRx(ctx, 3, max_samples_per_call=x.shape[1]) as o:
        a = run(ctx, x[:, :first], obj=o, generic=generic)
        assert a[2] == [2 * 1024] and o.fill() == fm.PREFIX + 100
        for bad in (3, -1):
            with pytest.raises(csdr_amd.CsdrAmdError, match="fmrx: channel out of range"):
                o.reset_channel(bad)
        o.reset_channel(1)
        assert o.fill() == fm.PREFIX + 100
        b = run(ctx, x[:, first:], obj=o, generic=generic)
        # the reset channel holds 1024 + 100 zeros and no history: so does a fresh channel fed 100 zero samples, which demodulate to exact zeros and, fewer than
        # the taps, write nothing
        fresh = run(ctx, np.concatenate([np.zeros((1, 100), np.complex64), x[1:2, first:]], axis=1), [100], generic=generic)
        assert fresh[2] == [0] + b[2]
        assert np.array_equal(b[0][1], fresh[0][0]) and np.array_equal(b[1][1].view(np.uint32), fresh[1][0].view(np.uint32))
        for c in (0, 2):
            assert np.array_equal(np.concatenate([a[0][c], b[0][c]]), undisturbed[0][c])
            assert np.array_equal(np.concatenate([a[1][c], b[1][c]]).view(np.uint32), undisturbed[1][c].view(np.uint32))
        o.reset()
        assert o.fill() == fm.PREFIX
        assert same_bits(run(ctx, x, [first], obj=o, generic=generic), undisturbed)


# ---------------------------------------------------------------- 6. the refusals
def test_fmrx_arguments(ctx):
    import csdr_amd
    for kw, msg in ((dict(audio_rate=22050), "fmrx: no de-emphasis table for sample rate 22050"), (dict(agc_block=1000), "fmrx: agc_block should be a multiple of 16"),
                    (dict(agc_block=0), "fmrx: agc_block"), (dict(agc_block=1552), "fmrx: agc_block"), (dict(limit=0.0), "fmrx: limit_max should be > 0"),
                    (dict(limit=-1.0), "fmrx: limit_max"), (dict(n_channels=0), "fmrx: n_channels should be 1")):
        args = dict(n_channels=2)
        args.update(kw)
        with pytest.raises(csdr_amd.CsdrAmdError, match=msg):
            csdr_amd.FmRx(ctx, **args)
    assert ctx.L.csdr_amd_fmrx_create(ctx.h, 2, 22050, 1024, 1.0, 1.0, 4096) is None
    x = fm.make_input(2, 4096)
    with ctx.fm_rx(2, max_samples_per_call=3000) as o:
        di, ds = ctx.upload(x), ctx.alloc(2 * 2 * 4096 + 256)
        assert ctx.L.csdr_amd_fmrx_process(o.h, di.ptr, 4096, 3001, ds.ptr, None, 4096) == -3 and "fmrx: n_in should be 0 .. max_samples_per_call (3000)" in ctx.err()
        assert ctx.L.csdr_amd_fmrx_process(o.h, di.ptr, 4096, 3000, ds.ptr, None, 2047) == -3 and "fmrx: out_pitch 2047 smaller than the 3072 audio samples" in ctx.err()
        assert o.fill() == fm.PREFIX                                     # a refused call changes nothing
        assert o.process_dev(di.ptr, 4096, 0, ds.ptr, None, 0) == 0 and o.fill() == fm.PREFIX
        assert o.process_dev(di.ptr, 4096, 3000, ds.ptr, None, 3072) == 3072
        assert o.max_output(3000) == 3072 and o.max_out(3000) == 3072 and o.max_output(0) == 0
    with ctx.fm_rx(1, max_samples_per_call=4096) as o:                   # one channel: the row is as long as the caller says
        assert o.process_dev(ctx.upload(x[0]).ptr, 0, 3000, ctx.alloc(2 * 4096).ptr, None, 0) == 3072


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


def test_fmrx_cli_bank_equals_python_composition(ctx, tmp_path):
    """`csdr fastddc_nfm_bank_s16` on 3 channels at the smallest channelizer geometry (transition_bw 0.05, decimation 2: fft 1024) against ctx.fastddc_bank ->
    FmRx with the same blocks per call (fmrx_model.bank_composition), byte for byte.  Channel 0's audio goes to a fifo: once the first batch's bytes have
    arrived the command is waiting for input, and the retune and reset lines written then are applied in front of the second batch, as they are in the
    composition.  The composition runs in a Python process of its own without torch: this geometry transforms with hipFFT, and a process that has imported
    torch runs the copy torch ships, whose last bits are not those of the system's copy that the command links (measured: every channel's baseband then differs
    in its low bits and 24 to 92 of 7168 audio samples per channel by one step; on the same library not one)."""
    import math
    import sys
    assert os.path.exists(CSDR), "csdr_amd/csdr not built (make -C csdr_amd/csrc)"
    D, tbw, rates = 2, 0.05, [-0.1, 0.2, -0.3]
    ddc, _ = ctx.fastddc_init(tbw, D, 0.0)
    inp = ddc.input_size
    per = 1024 // math.gcd(inp, 1024)                                    # blocks per call: the command takes CSDR_AMD_BLOCK in multiples of 1024 samples (8 x 896 here)
    rng = np.random.default_rng(77)
    t = np.arange(2 * per * inp)
    x = sum(0.3 * fm.fm_baseband(rng, t.size, dev=5e3 / 96e3) * np.exp(-2j * np.pi * r * t) for r in rates).astype(np.complex64)
    env = {k: v for k, v in os.environ.items() if k != "CSDR_AMD_WORLD"}
    # the composition
    np.savez(str(tmp_path / "in.npz"), x=x, tbw=tbw, decimation=D, rates=rates, per=per, retune_channel=1, retune_rate=0.25, reset_channel=2)
    c = subprocess.run(["timeout", "-k", "5", "120", sys.executable, os.path.join(ROOT, "tests", "fmrx_model.py"), str(tmp_path / "in.npz"), str(tmp_path / "want.npz")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, CSDR_AMD_NO_TORCH_PRELOAD="1"), timeout=150)
    assert c.returncode == 0, c.stderr.decode()
    w = np.load(str(tmp_path / "want.npz"))
    want = [w["first"], w["second"]]
    assert not w["torch_loaded"]
    assert want[0].shape[1] > 0 and want[1].shape[1] > 0 and want[0].shape[1] + want[1].shape[1] >= 6 * 1024
    # the command
    outs = [str(tmp_path / ("audio%d" % k)) for k in range(3)]
    ctl = str(tmp_path / "ctl")
    os.mkfifo(outs[0]); os.mkfifo(ctl)
    fo, fc = os.open(outs[0], os.O_RDWR | os.O_NONBLOCK), os.open(ctl, os.O_RDWR | os.O_NONBLOCK)      # (both ends held here: neither side's open waits for the other)
    args = ["timeout", "-k", "5", "90", CSDR, "fastddc_nfm_bank_s16", D, tbw, "HAMMING", 48000, ctl]
    for path, r in zip(outs, rates):
        args += [path, r]
    p = subprocess.Popen([str(a) for a in args], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, CSDR_AMD_BLOCK=str(per * inp)))
    try:
        p.stdin.write(x[:per * inp].tobytes()); p.stdin.flush()
        first = read_exactly(fo, 2 * want[0].shape[1])
        os.write(fc, b"1 0.25\n2 reset\n")
        p.stdin.write(x[per * inp:].tobytes()); p.stdin.close()
        second = read_exactly(fo, 2 * want[1].shape[1])
        assert p.wait(timeout=60) == 0, p.stderr.read().decode()
        err = p.stderr.read().decode()
    finally:
        if p.poll() is None:
            p.kill(); p.wait(timeout=10)
        os.close(fo); os.close(fc)
    assert "channel 1 retuned to 0.25" in err and "channel 2 reset" in err
    want_all = np.concatenate(want, axis=1)
    assert first + second == want_all[0].tobytes()
    for k in (1, 2):
        assert open(outs[k], "rb").read() == want_all[k].tobytes(), k
    # without the two lines channels 1 and 2 differ from this: the lines did something
    plain = w["plain"]
    assert np.array_equal(plain[0], want_all[0]) and not np.array_equal(plain[1], want_all[1]) and not np.array_equal(plain[2], want_all[2])


def test_fmrx_cli_single_stream_and_world_refusal(ctx, tmp_path):
    import csdr_amd
    assert os.path.exists(CSDR), "csdr_amd/csdr not built (make -C csdr_amd/csrc)"
    x = case_input(48000, 1, 7)[0]
    env = dict(os.environ, CSDR_AMD_BLOCK="4096")
    for rate in (48000, 11025):
        p = subprocess.run(["timeout", "-k", "5", "90", CSDR, "nfm_rx_cc_s16"] + ([str(rate)] if rate != 48000 else []), input=x.tobytes(), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, env=env, timeout=120)
        assert p.returncode == 0, p.stderr.decode()
        with csdr_amd.FmRx(ctx, 1, audio_rate=rate, max_samples_per_call=x.size) as o:
            want = o.process(x)[0][0]
        assert want.size >= 6 * 1024 and p.stdout == want.tobytes()
    p = subprocess.run(["timeout", "-k", "5", "90", CSDR, "fastddc_nfm_bank_s16", "2", "0.05", "HAMMING", "48000", "-", str(tmp_path / "a"), "0.1"], input=b"",
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, CSDR_AMD_WORLD="1"), timeout=120)
    assert p.returncode != 0 and "fastddc_nfm_bank_s16: runs on one GPU only: CSDR_AMD_WORLD is set" in p.stderr.decode()
    assert not os.path.exists(str(tmp_path / "a"))
