"""GPU checks of the AM / SSB receive chain object (amssb.hip): both kernels against the CPU run of the same functions bit for bit (channel counts, block
sizes, channels per wave, pitches, an unaligned base, with and without the pre-AGC tap), every cut into calls, the per-channel state calls, SSB behind its
filter, the U8 input through the owned front end against a separate front end, and the two CLI commands against the object byte for byte.  Nothing is compared
across agc_ff on unequal inputs except test 7's sanity figure."""
import os
import subprocess
import numpy as np
import pytest

import amssb_model as mm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "csdr_amd", "csdr")
f32, c64 = np.float32, np.complex64


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _inputs(mode, n_ch, n, block, seed):
    """[n_ch, n] complex: the kinds of amssb_model in turn, the last channel (of three or more) with Inf and NaN"""
    kinds = mm.INPUT_KINDS[:-1]
    x = np.empty((n_ch, n), c64)
    for c in range(n_ch):
        kind = mm.INPUT_KINDS[-1] if (n_ch >= 3 and c == n_ch - 1) else kinds[c % len(kinds)]
        x[c] = mm.complex_input(mode, kind, n, block, seed + 31 * c)
    return x


def _hook(P, x, states=None):
    """the expected (s16, pre_agc, states) from csdr_amd_debug_amssb_walk, channel by channel"""
    import csdr_amd
    nb = x.shape[1] // P.block
    s16 = np.empty((x.shape[0], nb * P.block), np.int16); pre = np.empty((x.shape[0], nb * P.block), f32)
    out_states = []
    for c in range(x.shape[0]):
        st = csdr_amd.AmSsbChan(0.0, 1.0) if states is None else csdr_amd.AmSsbChan(*states[c])
        s16[c], pre[c] = csdr_amd.amssb_debug_walk(P, x[c], st)
        out_states.append((st.last_dc, st.last_gain))
    return s16, pre, out_states


def _states(obj):
    return [(s.last_dc, s.last_gain) for s in (obj.get_channel(c) for c in range(obj.n_channels))]


def _same_states(got, want, what):
    assert mm.bits(np.array(got, f32)).tolist() == mm.bits(np.array(want, f32)).tolist(), what


def _name(mode, tiled):
    return "k_amssb_%s<%s>" % ("tiled" if tiled else "generic", mode.upper())


# (channels, block, lanes, force_generic, with_pre, extra in pitch, extra out pitch, bytes off alignment, blocks)
CF32_CASES = [
    (1, 64, 0, False, True, 0, 0, 0, 9),
    (3, 256, 4, False, False, 3, 1, 0, 7),
    (17, 1024, 16, False, True, 1, 3, 0, 5),
    (257, 64, 64, False, True, 0, 0, 0, 5),
    (257, 256, 1, False, True, 5, 7, 0, 5),
    (17, 1001, 0, False, True, 0, 0, 0, 5),
    (1, 16384, 0, False, True, 0, 0, 0, 3),
    (17, 256, 16, True, True, 3, 1, 0, 6),
    (3, 1024, 0, False, True, 1, 1, 4, 5),
    (257, 1024, 64, True, False, 0, 0, 0, 5),
    (3, 64, 64, False, True, 0, 0, 0, 8),
]


@pytest.mark.parametrize("mode", ["am", "ssb"])
@pytest.mark.parametrize("case", range(len(CF32_CASES)))
def test_cf32_vs_hook(ctx, mode, case):
    """4. the CF32 path against the hook, by bits: s16, pre_agc and the state"""
    import csdr_amd
    n_ch, B, lanes, generic, with_pre, ipx, opx, off, nb = CF32_CASES[case]
    agc = mm.AGC_ALT if case % 2 else mm.AGC_DEFAULT
    P = csdr_amd.amssb_params(mode, B, agc)
    n = nb * B
    x = _inputs(mode, n_ch, n, B, 10 * case)
    want16, wantpre, wst = _hook(P, x)
    with csdr_amd.AmSsb(ctx, P, n_ch, max_samples_per_call=n) as o:
        o.set_lanes(lanes)
        if generic:
            o.force_generic(True)
        s16, pre, counts = o.process(x, with_pre=with_pre, in_pitch=n + ipx, out_pitch=n + opx, in_offset=off)
        assert counts == [n]
        assert o.kernel_name() == _name(mode, not generic and B % 64 == 0 and off % 8 == 0)
        if lanes:
            assert o.lanes() == lanes
        mm.assert_bits(s16, want16, "s16")
        if with_pre:
            mm.assert_bits(pre, wantpre, "pre_agc")
        _same_states(_states(o) if n_ch <= 17 else [(s.last_dc, s.last_gain) for s in (o.get_channel(c) for c in (0, 63, 64, n_ch - 1))],
                     wst if n_ch <= 17 else [wst[c] for c in (0, 63, 64, n_ch - 1)], "state")


@pytest.mark.parametrize("mode", ["am", "ssb"])
@pytest.mark.parametrize("generic", [False, True])
def test_cuts(ctx, mode, generic):
    """5. one call, calls of [B / 3, 0, 1, 2 B + 5, rest] and one block per call: outputs and state equal by bits; the counts are the whole blocks that became
    available, 0 while less than a block has arrived; reset_channel, get_channel and set_channel"""
    import csdr_amd
    n_ch, B, nb = 5, 256, 7
    P = csdr_amd.amssb_params(mode, B, mm.AGC_ALT)
    n = nb * B
    x = _inputs(mode, n_ch, n, B, 77)
    want16, wantpre, wst = _hook(P, x)
    ragged = [B // 3, 0, 1, 2 * B + 5]; ragged.append(n - sum(ragged))
    for calls in ([n], ragged, [B] * nb):
        with csdr_amd.AmSsb(ctx, P, n_ch, max_samples_per_call=n) as o:
            if generic:
                o.force_generic(True)
            s16, pre, counts = o.process(x, calls=calls)
            have = np.cumsum(calls)
            assert counts == [int(h // B * B - (h - k) // B * B) for h, k in zip(have, calls)], (calls, counts)
            assert o.kernel_name() == _name(mode, not generic)
            mm.assert_bits(s16, want16, "s16 in calls %r" % (calls[:5],))
            mm.assert_bits(pre, wantpre, "pre_agc in calls %r" % (calls[:5],))
            _same_states(_states(o), wst, "state")
    assert ragged[0] < B and ragged[0] + 1 < B                              # (the first three calls give nothing)
    with csdr_amd.AmSsb(ctx, P, n_ch, max_samples_per_call=n) as o:
        if generic:
            o.force_generic(True)
        o.process(x)
        # one channel back to its start, the others carry on
        o.reset_channel(2)
        assert _states(o)[2] == (0.0, 1.0)
        st2 = list(wst); st2[2] = (0.0, 1.0)
        w16, wpre, wst2 = _hook(P, x, st2)
        s16, pre, _ = o.process(x)
        mm.assert_bits(s16, w16, "s16 after reset_channel"); mm.assert_bits(pre, wpre, "pre_agc after reset_channel")
        mm.assert_bits(s16[2], want16[2], "the reset channel starts over")
        _same_states(_states(o), wst2, "state after reset_channel")
        # set_channel / get_channel round trip, to the bit
        st = csdr_amd.AmSsbChan(float(f32(0.3125001)), float(f32(17.000002)))
        o.set_channel(4, st)
        back = o.get_channel(4)
        assert (back.last_dc, back.last_gain) == (st.last_dc, st.last_gain)
        st3 = list(wst2); st3[4] = (st.last_dc, st.last_gain)
        w16, _, wst3 = _hook(P, x[:, :3 * B], st3)
        s16, _, _ = o.process(x[:, :3 * B])
        mm.assert_bits(s16, w16, "s16 after set_channel")
        _same_states(_states(o), wst3, "state after set_channel")
        # reset: every channel, and nothing waiting
        o.process(x[:, :B // 2])
        o.reset()
        s16, _, counts = o.process(x)
        assert counts == [n]
        mm.assert_bits(s16, want16, "s16 after reset")


def _ssb_filter(port, lsb):
    nt = port.firdes_filter_len(0.05); fft = port.next_pow2(nt)
    if fft - nt < 200:
        fft *= 2
    return port.firdes_bandpass_c(nt, -0.1 if lsb else 0.0, 0.0 if lsb else 0.1), fft


@pytest.mark.parametrize("lsb", [False, True])
def test_ssb_with_filter(ctx, port, lsb):
    """6. SSB behind its filter: pre_agc against the oracle's bandpass_fir_fft_cc | realpart_cf within 1e-5 relative RMS; s16 against the hook run on the object's
    own pre_agc, by bits; the same in three ragged calls"""
    import csdr_amd
    import oracle
    n_ch, n, B = 3, 12000, 256
    taps, fft = _ssb_filter(port, lsb)
    rng = np.random.default_rng(60 + lsb)
    t = np.arange(n)
    x = np.stack([(0.3 * np.exp(2j * np.pi * (0.03 + 0.02 * c) * (-1 if lsb else 1) * t) * (1 + 0.5 * np.sin(2 * np.pi * t / (900.0 + 100 * c)))
                   + 0.05 * (rng.normal(size=n) + 1j * rng.normal(size=n))).astype(c64) for c in range(n_ch)])
    P = csdr_amd.amssb_params("ssb", B)
    inp = fft - taps.size + 1
    n_out = n // inp * inp // B * B
    assert n_out >= 5 * B
    for calls in ([n], [5000, 3, n - 5003]):
        with ctx.ssb_bank(n_ch, B, taps=taps, fft_size=fft, max_samples_per_call=n) as o:
            s16, pre, counts = o.process(x, calls=calls)
            assert sum(counts) == n_out and s16.shape == (n_ch, n_out) and o.kernel_name() == "k_amssb_tiled<SSB>"
            for c in range(n_ch):
                want = port.realpart_cf(port.bandpass_fir_fft_cc(x[c], taps, fft))[:n_out]
                e = oracle.relrms(pre[c], want)
                print("ssb%s calls %r channel %d: pre_agc against the oracle %.3g" % (" lsb" if lsb else "", calls, c, e))
                assert e <= 1e-5
                w16, wpre = csdr_amd.amssb_debug_walk(P, pre[c].astype(c64))
                mm.assert_bits(wpre, pre[c], "the hook's real part")
                mm.assert_bits(s16[c], w16, "s16 on the object's own pre_agc")


@pytest.mark.parametrize("n_ch", [3, 19])
@pytest.mark.parametrize("variant", ["one_rate", "rates", "set_rate"])
def test_u8_path(ctx, port, n_ch, variant):
    """7. U8 input through the owned front end: s16 and pre_agc equal, by bits, a CF32 object fed the output of a separate csdr_amd_ddc driven with the same calls;
    pre_agc against the oracle's stages within 1e-5 of the envelope's RMS; s16 against the full oracle chain as a sanity figure (relative RMS < 2e-2)"""
    import csdr_amd
    import oracle
    n, D, B = 1024 * 300, 50, 256
    calls = [1024 * 200, 1024 * 100]
    carriers = np.full(n_ch, 0.25) if variant == "one_rate" else 0.25 - 0.03 * np.arange(n_ch)
    u8 = mm.am_test_signal(n, 15, carriers, n_ch)
    taps = ctx.firdes_lowpass_f(ctx.firdes_filter_len(0.005), 0.5 / D)
    rates = -carriers.astype(f32)
    retunes = None
    if variant == "one_rate":
        create_rate = float(rates[0])
    else:
        create_rate = rates.copy()
        if variant == "set_rate":                                       # channel 1 starts elsewhere and is tuned in front of the second call
            create_rate[1] = 0.1
            retunes = {1: [(1, float(rates[1]))]}
    P = csdr_amd.amssb_params("am", B)
    with ctx.am_bank(n_ch, B, in_format="u8", shift_rate=create_rate, decimation=D, ddc_taps=taps, max_samples_per_call=max(calls)) as o:
        s16, pre, counts = o.process(u8, calls=calls, retunes=retunes)
        assert o.kernel_name() == "k_amssb_tiled<AM>" and o.front_end_kernel() != ""
        assert o.get_rate(1) == f32(rates[1])
    assert sum(counts) == 23 * B and all(k % B == 0 for k in counts)
    y = ctx.ddc_u8(u8, create_rate, D, taps, block=calls, retunes=retunes)
    with ctx.am_bank(n_ch, B, max_samples_per_call=y.shape[1]) as o:
        w16, wpre, _ = o.process(y)
    mm.assert_bits(s16, w16, "s16 against the CF32 object behind a separate front end")
    mm.assert_bits(pre, wpre, "pre_agc against the CF32 object behind a separate front end")
    for c in range(n_ch):
        if variant == "set_rate" and c == 1:
            continue
        sh, _ = port.shift_addition_cc(port.convert_u8_f(u8[c]).view(c64), float(rates[c]))
        dec = port.fir_decimate_cc(sh, D, taps)
        env = port.amdemod_cf(dec)
        want, _ = port.fastdcblock_ff(env, B)
        m = 23 * B
        assert want.size >= m
        e = mm.relrms_to(pre[c], want[:m], env[:m])
        full = port.convert_f_s16(port.limit_ff(port.agc_ff(want[:m], B)[0], 1.0))
        e16 = oracle.relrms(s16[c].astype(f32), full.astype(f32))
        print("u8 %s channel %d: pre_agc %.3g of the envelope's RMS, s16 against the full oracle chain %.3g" % (variant, c, e, e16))
        assert e <= 1e-5
        assert e16 < 2e-2


def _run_cli(tmp_path, args, sig, env_extra=None):
    outs = []
    for k in range(len(sig)):
        fi = tmp_path / ("in%d.u8" % k); fo = tmp_path / ("out%d.s16" % k)
        sig[k].tofile(fi); outs.append(fo); args = args + [str(fi), str(fo)]
    env = dict(os.environ, CSDR_AMD_BANK_BLOCK="65536", **(env_extra or {}))
    p = subprocess.run([CLI] + args, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    return [np.fromfile(o, np.int16) for o in outs], p.stderr


def _object_audio(ctx, port, cmd, lsb, u8, rates, calls, retunes=None):
    import csdr_amd
    taps = ctx.firdes_lowpass_f(ctx.firdes_filter_len(0.005), 0.5 / 50)
    kw = dict(in_format="u8", shift_rate=np.asarray(rates, f32), decimation=50, ddc_taps=taps, max_samples_per_call=65536)
    if cmd.startswith("am"):
        o = ctx.am_bank(len(u8), **kw)
    else:
        bp, fft = _ssb_filter(port, lsb)
        o = ctx.ssb_bank(len(u8), taps=bp, fft_size=fft, **kw)
    with o:
        s16, _, _ = o.process(np.stack(u8), calls=calls, with_pre=False, in_pitch=2 * 65536 * len(calls), retunes=retunes)
    return s16


@pytest.mark.parametrize("cmd,lsb", [("am_bank_u8_s16", False), ("ssb_bank_u8_s16", False), ("ssb_bank_u8_s16", True)])
def test_cli_banks(ctx, port, tmp_path, cmd, lsb):
    """8. `csdr am_bank_u8_s16` / `csdr ssb_bank_u8_s16 [--lsb]` on two input files against the Python object making the same calls, byte for byte"""
    n = 3 * 65536 + 5 * 1024
    u8 = [mm.am_test_signal(n, 800 + k, 0.25 - 0.05 * k)[0] for k in range(2)]
    rates = [-0.25, -0.2]
    got, _ = _run_cli(tmp_path, [cmd] + (["--lsb"] if lsb else []) + [",".join("%g" % r for r in rates)], u8)
    want = _object_audio(ctx, port, cmd, lsb, u8, rates, [65536] * 3 + [5 * 1024])
    assert want.shape[1] >= 3 * 1024
    for k in range(2):
        assert got[k].tobytes() == want[k].tobytes(), "stream %d: %d samples against %d" % (k, got[k].size, want.shape[1])


@pytest.mark.parametrize("cmd", ["am_bank_u8_s16", "ssb_bank_u8_s16"])
def test_cli_banks_control_channel(ctx, port, tmp_path, cmd):
    """`--ctl <fifo>`: a line "<stream> <rate>" that is in the fifo before the process starts is applied in front of the first pass (as
    tests/test_cli_gpu.py::test_cli_bank_rate_per_stream_and_control_channel does for the NFM bank): the object retuned in front of its first call, byte for byte"""
    n = 2 * 65536 + 3 * 1024
    rates = [-0.25, 0.3, -0.15]
    new1 = -0.2
    u8 = [mm.am_test_signal(n, 810 + k, -r)[0] for k, r in enumerate([rates[0], new1, rates[2]])]
    ctl = tmp_path / "ctl.fifo"; os.mkfifo(ctl)
    keep = os.open(ctl, os.O_RDWR)                      # keeps the fifo open for writing while the command runs
    os.write(keep, b"1 %g\n" % new1)
    try:
        got, err = _run_cli(tmp_path, [cmd, "--ctl", str(ctl), ",".join("%g" % r for r in rates)], u8)
    finally:
        os.close(keep)
    assert b"stream 1 reinitialized to -0.2" in err
    want = _object_audio(ctx, port, cmd, False, u8, rates, [65536] * 2 + [3 * 1024], retunes={0: [(1, new1)]})
    for k in range(3):
        assert got[k].size > 0 and got[k].tobytes() == want[k].tobytes(), "stream %d" % k
