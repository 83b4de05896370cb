"""GPU checks of the passband per stream (csdr_amd_fftfilt_create_per_stream / set_stream_taps) and per SSB channel (csdr_amd_amssb_set_passband).

The gate is derived, not measured: a per-stream filter runs the shared filter's arithmetic on the shared filter's tables, row by row; only the address of the
table differs.  So stream s of a per-stream filter equals, word for word, stream s of a shared filter that has stream s's taps, in every kernel family, for every
cut into calls, and whichever workgroup a window falls to.

How a family is selected: the wave and team kernels take the calls with an even sample count, the 256- / 512-thread kernels k_fftfilt_lds<N> the odd ones and
everything under CSDR_AMD_FFTFILT_LDS_MODE=5.  An odd tap count makes the block fft_size - taps + 1 even, so every call of a 63- / 1041- / 4095-tap filter has an
even sample count: those reach k_fftfilt_lds<N> through MODE=5, and the odd-count route is taken with one tap fewer (62 / 1040 / 4094: the same windows)."""
import os
import subprocess
import numpy as np
import pytest

import amssb_model as mm
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "csdr_amd", "csdr")
f32, c64 = np.float32, np.complex64
BANDS = [(0.0, 0.1), (-0.1, 0.0), (-0.05, 0.2)]          # USB, LSB, asymmetric across 0


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def crand(rng, shape):
    return (rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)).astype(c64)


def bits(a):
    return np.ascontiguousarray(a, c64).view(np.uint64)


def same_bits(got, want, what):
    assert got.shape == want.shape, "%s: shape %r against %r" % (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, "%s: %d words differ, first at %r" % (what, len(bad), tuple(bad[0]))


# (kernel, taps, fft_size, CSDR_AMD_FFTFILT_LDS_MODE, window, windows in flight per CU as fw_launch / ft_launch / ffl_launch size their grids)
FAMILIES = [
    ("k_fftfilt_wave", 63, 256, "6", 4096, 8),
    ("k_fftfilt_team<2>", 1041, 2048, None, 8192, 4),
    ("k_fftfilt_team<4>", 4095, 8192, None, 16384, 2),
    ("k_fftfilt_lds<4096>", 63, 256, "5", 4096, 4),
    ("k_fftfilt_lds<8192>", 1041, 2048, "5", 8192, 1),
    ("k_fftfilt_lds<16384>", 4095, 8192, "5", 16384, 1),
    ("k_fftfilt_lds<4096>", 62, 256, None, 4096, 4),
    ("k_fftfilt_lds<8192>", 1040, 2048, None, 8192, 1),
    ("k_fftfilt_lds<16384>", 4094, 8192, None, 16384, 1),
]
FAMILY_IDS = ["%s-%d%s" % (f[0], f[1], "-mode" + f[3] if f[3] else "") for f in FAMILIES]


def _select(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("CSDR_AMD_FFTFILT_LDS_MODE", raising=False)
    else:
        monkeypatch.setenv("CSDR_AMD_FFTFILT_LDS_MODE", mode)      # read when the object is created
    monkeypatch.delenv("CSDR_AMD_FFTFILT_LDS_OFF", raising=False)
    monkeypatch.delenv("CSDR_AMD_FFTFILT_LDS_N", raising=False)


def _three(ctx, nt):
    """the three passbands at nt taps; an even count is the design of nt + 1 taps (the designer's lengths are odd, libcsdr.c:127-142) without its last tap"""
    return np.stack([ctx.firdes_bandpass_c(nt | 1, lo, hi)[:nt] for lo, hi in BANDS])


def _expect_kernel(kernels, calls, inp, name):
    """every call with the family's parity ran the family's kernel (an odd-count family: the odd calls)"""
    odd_family = inp % 2 == 1
    hit = [k for k, b in zip(kernels, calls) if not odd_family or (b * inp) % 2 == 1]
    assert hit and all(k == name for k in hit), (kernels, calls, name)


@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_per_stream_equals_shared_small(ctx, monkeypatch, family):
    """5 streams, stream s with filter s % 3, calls of 1, 2 and 5 blocks: word for word the rows of three shared-taps filters making the same calls"""
    name, nt, fft, mode, win, _ = family
    _select(monkeypatch, mode)
    S, calls = 5, [1, 2, 5]
    inp = fft - nt + 1
    taps = _three(ctx, nt)
    x = crand(np.random.default_rng(nt), (S, inp * sum(calls)))
    with ctx.fftfilt(fft, taps[[s % 3 for s in range(S)]], S, max(calls)) as f:
        assert f.per_stream() and f.window() == win
        y = f.process(x, calls)
        _expect_kernel(f.kernels, calls, inp, name)
    for k in range(3):
        with ctx.fftfilt(fft, taps[k], S, max(calls)) as f:
            assert not f.per_stream()
            want = f.process(x, calls)
            _expect_kernel(f.kernels, calls, inp, name)
        rows = [s for s in range(S) if s % 3 == k]
        same_bits(y[rows], want[rows], "%s, streams with filter %d" % (name, k))
    assert np.abs(y).max() > 0.01


@pytest.mark.parametrize("wps", [1, 3])
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_per_stream_equals_shared_full_grid(ctx, monkeypatch, family, wps):
    """n_streams x windows per stream >= 3 x the windows the launch keeps in flight, at 1 and 3 windows per stream: every workgroup walks several windows and
    crosses stream boundaries (what k_fftfilt_lds<8192>'s reload of its register-held spectrum exists for).  The input rows repeat with period 64 and the taps
    with period 3, so the expected rows come from three shared filters of 64 streams."""
    import torch
    name, nt, fft, mode, win, per_cu = family
    _select(monkeypatch, mode)
    inp = fft - nt + 1
    V = win - ((nt - 1 + 15) & ~15)                                     # new samples per window
    blocks = 1 if wps == 1 else 2 * V // inp + 1
    if (inp % 2) and not (blocks % 2):
        blocks += 1                                                     # (an odd-count family: an odd call)
    m = blocks * inp
    assert (m + V - 1) // V == wps
    in_flight = torch.cuda.get_device_properties(0).multi_processor_count * per_cu
    S = -(-3 * in_flight // wps)
    S += -S % 3 + 1                                                     # not a multiple of 3 or 64
    taps = _three(ctx, nt)
    x64 = crand(np.random.default_rng(1000 + nt + wps), (64, m))
    want = []
    for k in range(3):
        with ctx.fftfilt(fft, taps[k], 64, blocks) as f:
            want.append(f.process(x64, [blocks]))
            assert f.kernels == [name], f.kernels
    s_idx = np.arange(S)
    with ctx.fftfilt(fft, taps[s_idx % 3], S, blocks) as f:
        y = f.process(x64[s_idx % 64], [blocks])
        assert f.kernels == [name], f.kernels
    want = np.stack(want)[s_idx % 3, s_idx % 64]
    print("%s: %d streams x %d windows on %d windows in flight" % (name, S, wps, in_flight))
    same_bits(y, want, "%s at %d windows per stream" % (name, wps))


def test_per_stream_against_the_oracle(ctx, port, monkeypatch):
    """5 streams, five passbands: each stream against the oracle's bandpass_fir_fft_cc on that stream with that stream's taps"""
    from oracle import relrms
    _select(monkeypatch, None)
    S, nt, fft = 5, 255, 1024
    inp = fft - nt + 1
    bands = [(0.0, 0.1), (-0.1, 0.0), (0.01, 0.02), (-0.2, 0.2), (-0.3, 0.05)]
    taps = np.stack([port.firdes_bandpass_c(nt, lo, hi) for lo, hi in bands])
    x = crand(np.random.default_rng(77), (S, inp * 7))
    y = ctx.bandpass_fir_fft_cc(x, taps, fft, blocks_per_call=3)
    for s in range(S):
        e = relrms(y[s], port.bandpass_fir_fft_cc(x[s], taps[s], fft))
        print("stream %d, passband %r: %.3g" % (s, bands[s], e))
        assert e < TOL


def _retune_case(ctx):
    S, nt, fft = 5, 1041, 2048
    inp = fft - nt + 1
    a, b = ctx.firdes_bandpass_c(nt, 0.0, 0.1), ctx.firdes_bandpass_c(nt, -0.2, -0.05)
    x = crand(np.random.default_rng(78), (S, inp * 5))
    return S, fft, inp, a, b, x


def _two_calls(f, x, inp, between):
    y0 = f.process(x[:, :2 * inp], [2])
    between(f)
    return np.concatenate([y0, f.process(x[:, 2 * inp:], [3])], axis=1)


def test_retune_and_upgrade(ctx, monkeypatch):
    """set_stream_taps between two calls: that stream as a shared filter given set_taps at the same point, the others as a filter never retuned; the upgrade of a
    shared filter keeps the carried history; set_taps on a per-stream filter sets every row"""
    _select(monkeypatch, None)
    S, fft, inp, a, b, x = _retune_case(ctx)
    with ctx.fftfilt(fft, a, S, 3) as f:
        never = _two_calls(f, x, inp, lambda f: None)
    with ctx.fftfilt(fft, a, S, 3) as f:
        all_b = _two_calls(f, x, inp, lambda f: f.set_taps(b))
    assert not np.array_equal(bits(never[:, 2 * inp:]), bits(all_b[:, 2 * inp:]))
    with ctx.fftfilt(fft, a, S, 3) as f:
        got = _two_calls(f, x, inp, lambda f: f.set_stream_taps(2, b))
        assert f.per_stream()
    same_bits(got[2], all_b[2], "the retuned stream")
    same_bits(got[[0, 1, 3, 4]], never[[0, 1, 3, 4]], "the streams left alone")
    with ctx.fftfilt(fft, a, S, 3) as f:
        got = _two_calls(f, x, inp, lambda f: f.set_stream_taps(0, a))
        assert f.per_stream()
    same_bits(got, never, "upgraded in place with the same taps")
    with ctx.fftfilt(fft, np.stack([a, b, a, b, a]), S, 3) as f:
        got = _two_calls(f, x, inp, lambda f: f.set_taps(b))
        assert f.per_stream()
    same_bits(got[[1, 3], 2 * inp:], all_b[[1, 3], 2 * inp:], "set_taps on a per-stream filter, rows that had b")
    same_bits(got[[0, 2, 4]], all_b[[0, 2, 4]], "set_taps on a per-stream filter, rows that had a")


def _refused(ctx, call, word):
    import csdr_amd
    with pytest.raises(csdr_amd.CsdrAmdError) as e:
        call()
    assert word in str(e.value), str(e.value)


@pytest.mark.parametrize("case", ["one_pass", "8191_taps", "lds_off"])
def test_refusals(ctx, monkeypatch, case):
    """a wrong taps length, a stream out of range, a per-stream request on a filter that runs the full-size transform (by its length, or because the one-pass path
    is switched off): negative status, message set, and the next process gives what a filter nobody asked gives"""
    _select(monkeypatch, None)
    S = 3
    nt, fft = (8191, 16384) if case == "8191_taps" else (255, 1024)
    if case == "lds_off":
        monkeypatch.setenv("CSDR_AMD_FFTFILT_LDS_OFF", "1")
    inp = fft - nt + 1
    a, b = ctx.firdes_bandpass_c(nt, 0.0, 0.1), ctx.firdes_bandpass_c(nt, -0.1, 0.0)
    x = crand(np.random.default_rng(79), (S, inp * 4))
    with ctx.fftfilt(fft, a, S, 2) as f:
        want = np.concatenate([f.process(x[:, :2 * inp]), f.process(x[:, 2 * inp:])], axis=1)
        assert (f.kernels[0] != "") == (case == "one_pass")
    with ctx.fftfilt(fft, a, S, 2) as f:
        y0 = f.process(x[:, :2 * inp])
        _refused(ctx, lambda: f.set_stream_taps(1, b[:-1]), "taps_length")
        _refused(ctx, lambda: f.set_stream_taps(-1, b), "out of range")
        _refused(ctx, lambda: f.set_stream_taps(S, b), "out of range")
        if case != "one_pass":
            _refused(ctx, lambda: f.set_stream_taps(1, b), "one-pass")
            _refused(ctx, lambda: ctx.fftfilt(fft, np.stack([a, b, a]), S, 2), "one-pass")
        assert not f.per_stream()
        got = np.concatenate([y0, f.process(x[:, 2 * inp:])], axis=1)
    same_bits(got, want, "after the refusals")


# ---------------------------------------------------------------- the SSB bank
SSB_BANDS = [(0.0, 0.1), (-0.1, 0.0), (0.01, 0.02), (-0.2, 0.2)]


def _ssb_geometry(ctx):
    nt = ctx.firdes_filter_len(0.05)
    fft = 1 << (nt - 1).bit_length()
    if fft - nt < 200:
        fft *= 2
    return nt, fft


@pytest.mark.parametrize("u8", [False, True], ids=["cf32", "u8"])
def test_ssb_bank_passband_per_channel(ctx, u8):
    """4 channels, 4 passbands: row c of audio_s16 and pre_agc equals, by bits, row c of a 4-channel bank whose one passband is channel c's; unequal calls, one
    of them empty; CF32 input and the U8 front end"""
    nt, fft = _ssb_geometry(ctx)
    n_ch, B = 4, 256
    if u8:
        n, D = 1024 * 120, 50
        calls = [1024 * 70, 0, 1024 * 50]
        x = mm.am_test_signal(n, 21, 0.25 - 0.03 * np.arange(n_ch), n_ch)
        kw = dict(in_format="u8", shift_rate=(-(0.25 - 0.03 * np.arange(n_ch))).astype(f32), decimation=D,
                  ddc_taps=ctx.firdes_lowpass_f(ctx.firdes_filter_len(0.005), 0.5 / D), max_samples_per_call=max(calls))
    else:
        n = 6000
        calls = [2500, 0, 7, n - 2507]
        x = crand(np.random.default_rng(80), (n_ch, n)) * f32(0.3)
        kw = dict(max_samples_per_call=max(calls))
    taps = [ctx.firdes_bandpass_c(nt, lo, hi) for lo, hi in SSB_BANDS]
    with ctx.ssb_bank(n_ch, B, taps=taps[0], fft_size=fft, passbands=SSB_BANDS, **kw) as o:
        s16, pre, counts = o.process(x, calls=calls)
        assert [o.get_passband(c) for c in range(n_ch)] == [(float(f32(lo)), float(f32(hi))) for lo, hi in SSB_BANDS]
    assert s16.shape[1] >= 2 * B and counts[1] == 0
    for c in range(n_ch):
        with ctx.ssb_bank(n_ch, B, taps=taps[c], fft_size=fft, **kw) as o:
            w16, wpre, wcounts = o.process(x, calls=calls)
        assert wcounts == counts
        mm.assert_bits(s16[c], w16[c], "audio_s16 of channel %d" % c)
        mm.assert_bits(pre[c], wpre[c], "pre_agc of channel %d" % c)
    assert len({pre[c].tobytes() for c in range(n_ch)}) == n_ch


def test_ssb_bank_retune_and_readback(ctx):
    """set_passband between two calls: the channel as a bank whose channels were all given the same taps at the same call boundary, the others as a bank left
    alone; get_passband returns what was set, NaN for taps of the caller's own; reset and reset_channel keep the passbands; an AM object refuses"""
    import csdr_amd
    nt, fft = _ssb_geometry(ctx)
    n_ch, B, n = 4, 256, 6000
    calls = [2500, n - 2500]
    x = crand(np.random.default_rng(81), (n_ch, n)) * f32(0.3)
    a, b = ctx.firdes_bandpass_c(nt, 0.0, 0.1), ctx.firdes_bandpass_c(nt, -0.1, 0.0)
    kw = dict(taps=a, fft_size=fft, max_samples_per_call=max(calls))
    with ctx.ssb_bank(n_ch, B, **kw) as o:
        n16, npre, _ = o.process(x, calls=calls)
    with ctx.ssb_bank(n_ch, B, **kw) as o:
        a16, apre, _ = o.process(x, calls=calls, retunes={1: [(c, "taps", b) for c in range(n_ch)]})
        assert all(np.isnan(o.get_passband(c)).all() for c in range(n_ch))
    with ctx.ssb_bank(n_ch, B, **kw) as o:
        assert np.isnan(o.get_passband(2)).all()
        g16, gpre, _ = o.process(x, calls=calls, retunes={1: [(2, "bp", -0.1, 0.0)]})
        assert o.get_passband(2) == (float(f32(-0.1)), 0.0) and np.isnan(o.get_passband(1)).all()
        mm.assert_bits(g16[2], a16[2], "audio_s16 of the retuned channel")
        mm.assert_bits(gpre[2], apre[2], "pre_agc of the retuned channel")
        mm.assert_bits(g16[[0, 1, 3]], n16[[0, 1, 3]], "audio_s16 of the channels left alone")
        assert not np.array_equal(gpre[2], npre[2])
        # reset and reset_channel keep the passbands: the stream again from the start, channel 2 now LSB from its first sample
        o.reset(); o.reset_channel(2)
        assert o.get_passband(2) == (float(f32(-0.1)), 0.0)
        r16, rpre, _ = o.process(x, calls=calls)
    with ctx.ssb_bank(n_ch, B, taps=b, fft_size=fft, max_samples_per_call=max(calls)) as o:
        b16, bpre, _ = o.process(x, calls=calls)
    mm.assert_bits(rpre[2], bpre[2], "pre_agc of channel 2 after reset")
    mm.assert_bits(r16[[0, 1, 3]], n16[[0, 1, 3]], "audio_s16 of the other channels after reset")
    with ctx.am_bank(n_ch, B, max_samples_per_call=1024) as o:
        for call in (lambda: o.set_passband(0, 0.0, 0.1), lambda: o.set_channel_taps(0, np.zeros(0, c64)), lambda: o.get_passband(0)):
            with pytest.raises(csdr_amd.CsdrAmdError) as e:
                call()
            assert "SSB" in str(e.value)


# ---------------------------------------------------------------- the CLI
N_CLI = 65536 + 3 * 1024
RATES = "-0.25,-0.2"


def _cli(tmp, tag, args, u8, ok=True):
    outs = []
    for k in range(len(u8)):
        fi = tmp / ("in%d.u8" % k); fo = tmp / ("%s%d.s16" % (tag, k))
        if not fi.exists():
            u8[k].tofile(fi)
        outs.append(fo); args = args + [str(fi), str(fo)]
    env = dict(os.environ, CSDR_AMD_BANK_BLOCK="65536")
    p = subprocess.run([CLI] + args, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    if not ok:
        return p
    assert p.returncode == 0, p.stderr.decode()
    return [np.fromfile(o, np.int16) for o in outs], p.stderr


@pytest.fixture(scope="module")
def cli_plain(tmp_path_factory):
    """the two inputs and what the plain and the --lsb command make of them"""
    tmp = tmp_path_factory.mktemp("passbands_cli")
    u8 = [mm.am_test_signal(N_CLI, 820 + k, 0.25 - 0.05 * k)[0] for k in range(2)]
    usb, _ = _cli(tmp, "usb", ["ssb_bank_u8_s16", RATES], u8)
    lsb, _ = _cli(tmp, "lsb", ["ssb_bank_u8_s16", "--lsb", RATES], u8)
    assert usb[0].size >= 1024 and usb[1].tobytes() != lsb[1].tobytes()
    return tmp, u8, usb, lsb


def test_cli_passbands(cli_plain):
    """`--passbands 0:0.1,-0.1:0`: stream 0 as the plain command's, stream 1 as the --lsb command's, byte for byte; one pair serves all streams"""
    tmp, u8, usb, lsb = cli_plain
    got, _ = _cli(tmp, "pb", ["ssb_bank_u8_s16", "--passbands", "0:0.1,-0.1:0", RATES], u8)
    assert got[0].tobytes() == usb[0].tobytes() and got[1].tobytes() == lsb[1].tobytes()
    got, _ = _cli(tmp, "pb1", ["ssb_bank_u8_s16", "--passbands", "-0.1:0", RATES], u8)
    assert got[0].tobytes() == lsb[0].tobytes() and got[1].tobytes() == lsb[1].tobytes()


def test_cli_passband_control_line(cli_plain):
    """a line "1 bp -0.1 0" waiting in the --ctl fifo retunes stream 1 in front of the first pass, and stream 1 only"""
    tmp, u8, usb, lsb = cli_plain
    ctl = tmp / "ctl.fifo"; os.mkfifo(ctl)
    keep = os.open(ctl, os.O_RDWR)                      # keeps the fifo open for writing while the command runs
    os.write(keep, b"1 bp -0.1 0\n")
    try:
        got, err = _cli(tmp, "ctl", ["ssb_bank_u8_s16", "--ctl", str(ctl), RATES], u8)
    finally:
        os.close(keep)
    assert b"stream 1 passband reinitialized to -0.1 0" in err
    assert got[0].tobytes() == usb[0].tobytes() and got[1].tobytes() == lsb[1].tobytes()


@pytest.mark.parametrize("args", [["--passbands", "0,0.1"], ["--passbands", "0:0.1,-0.1:0,0:0.2"], ["--lsb", "--passbands", "0:0.1"],
                                  ["--passbands", "0:0.1", "--lsb"]], ids=["no_colon", "count", "lsb_first", "lsb_after"])
def test_cli_passbands_syntax(cli_plain, args):
    """malformed specs end as badsyntax does"""
    tmp, u8, _, _ = cli_plain
    p = _cli(tmp, "bad", ["ssb_bank_u8_s16"] + args + [RATES], u8, ok=False)
    assert p.returncode == 255 and p.stderr
