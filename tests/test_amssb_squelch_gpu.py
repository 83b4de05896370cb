"""GPU checks of the squelch and S-meter inside the AM / SSB receive bank (csdr_amd_amssb_enable_squelch, amssb.hip): the gated tiled kernel, the gated generic
kernel and the composition csdr_amd.Squelch -> unsquelched AmSsb against each other and against the CPU walk on the model's gated stream, in every bit, for
every cut into calls; the powers against float64 and the flags exactly; the three ways of a block, each reached, with the state carried through the zero-run
shortcut; levels, resets and refusals; the owned front end and filter; the two CLI commands."""
import os
import subprocess
import numpy as np
import pytest

import amssb_model as mm
import amssb_squelch_model as qm
import squelch_model as sm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "csdr_amd", "csdr")
f32, c64 = np.float32, np.complex64
NB = qm.NB


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _name(mode, tiled, sq=True):
    return "k_amssb_%s%s<%s>" % ("tiled" if tiled else "generic", "_sq" if sq else "", mode.upper())


def _states(o):
    return [(s.last_dc, s.last_gain) for s in (o.get_channel(c) for c in range(o.n_channels))]


def _same_states(got, want, what):
    mm.assert_bits(np.array(got, f32), np.array(want, f32), what)


def _composed(ctx, P, x, d, levels, calls=None, levels_between=None, states=None):
    """csdr_amd.Squelch into a second buffer, then the unsquelched AmSsb -> (s16, pre_agc, powers, flags, states)"""
    import csdr_amd
    n_ch, n = x.shape
    with csdr_amd.Squelch(ctx, n_ch, P.block, d, levels, max_samples_per_call=max(n, 1)) as q:
        g, pw, fl = q.process(x, calls=calls, levels_between=levels_between)
    g, pw, fl = np.stack(g), np.stack(pw), np.stack(fl)
    with csdr_amd.AmSsb(ctx, P, n_ch, max_samples_per_call=max(g.shape[1], 1)) as o:
        for c, st in enumerate(states or []):
            o.set_channel(c, csdr_amd.AmSsbChan(*st))
        s16, pre, _ = o.process(g)
        assert "_sq" not in o.kernel_name()
        return s16, pre, pw, fl, _states(o)


def _walked(P, x, d, levels, changes=None, states=None):
    """csdr_amd_debug_amssb_walk on the model's gated stream, channel by channel"""
    import csdr_amd
    rows = [qm.expected(csdr_amd, P, x[c], d, float(levels[c]), None if changes is None else changes.get(c), None if states is None else states[c])
            for c in range(x.shape[0])]
    return tuple(np.stack([r[k] for r in rows]) for k in range(4)) + ([r[4] for r in rows],)


def _cuts(B, n):
    third = max(B // 3, 1)
    ragged = [B // 3, 0, 3 * B + 5]; ragged.append(n - sum(ragged))
    thirds = [third] * (n // third); thirds.append(n - sum(thirds))
    return {"one": [n], "ragged": ragged, "thirds": thirds, "zeros": [0, n // 2, 0, 0, n - n // 2, 0]}


def _run_gated(ctx, P, x, d, levels, lanes=0, generic=False, **kw):
    import csdr_amd
    n_ch, n = x.shape
    with csdr_amd.AmSsb(ctx, P, n_ch, max_samples_per_call=max(n, 1), squelch=True, use_every_nth=d, levels=levels) as o:
        o.set_lanes(lanes)
        o.force_generic(generic)
        out = o.process_squelched(x, **kw)
        return out + (_states(o), o.squelch_block_index())


def _check(got, want, what, counts_total=None):
    s16, pre, counts, pw, fl = got[:5]
    mm.assert_bits(s16, want[0], what + ": s16")
    mm.assert_bits(pre, want[1], what + ": pre_agc")
    mm.assert_bits(pw, want[2], what + ": powers")
    assert np.array_equal(fl, want[3]), what + ": flags"
    if counts_total is not None:
        assert sum(counts) == counts_total


SHAPES = [(n_ch, lanes) for n_ch in (1, 5, 17) for lanes in (0, 4, 16)]


@pytest.mark.parametrize("mode", ["am", "ssb"])
@pytest.mark.parametrize("n_ch,lanes", SHAPES)
def test_three_paths_and_the_walk(ctx, mode, n_ch, lanes):
    """the gated tiled kernel (B 64, 128), the gated generic kernel (the same B forced, B 100 and 2 by themselves) and Squelch -> AmSsb: s16, pre_agc, powers, flags,
    counts and states equal in every bit, for every cut, and equal to the CPU walk on the model's gated stream; the powers within (ceil(B / d) + 8) 2^-24 P of
    float64, the flags those of the float64 powers"""
    import csdr_amd
    for bi, B in enumerate((64, 128, 100, 2)):
        d = (1, 3)[(bi + SHAPES.index((n_ch, lanes))) % 2]
        P = csdr_amd.amssb_params(mode, B, mm.AGC_ALT if bi % 2 else mm.AGC_DEFAULT)
        x = qm.make_input(mode, n_ch, NB, B, extra=B // 2)
        n = x.shape[1]
        lv = qm.levels(n_ch)
        want = _composed(ctx, P, x, d, lv)
        walked = _walked(P, x, d, lv)
        for k in range(3):
            mm.assert_bits(want[k], walked[k], "B %d: the composition against the walk on the model's stream, output %d" % (B, k))
        assert np.array_equal(want[3], walked[3]), "flags"
        _same_states(want[4], walked[4], "states")
        for c in range(n_ch):
            assert np.array_equal(want[3][c], qm.flags64(x[c, :NB * B], B, d, float(lv[c]))), "flags against float64"
            for k in range(NB):
                p64 = sm.power64(x[c, k * B:(k + 1) * B], d)
                assert abs(float(want[2][c, k]) - p64) <= sm.bound(B, d, p64), "power of channel %d block %d" % (c, k)
        tiled = B % 64 == 0
        cuts = _cuts(B, n)
        for generic in ((False, True) if tiled else (False,)):
            for cut in (("one", "ragged", "thirds", "zeros") if lanes == 0 else ("one", ("ragged", "thirds", "zeros")[(bi + lanes // 8) % 3])):
                got = _run_gated(ctx, P, x, d, lv, lanes, generic, calls=cuts[cut])
                what = "%s B %d d %d %s %s" % (mode, B, d, "generic" if generic else "auto", cut)
                _check(got, want, what, NB * B)
                assert all(k % B == 0 for k in got[2])
                assert got[5] and set(got[5]) == {_name(mode, tiled and not generic)}, what
                _same_states(got[6], want[4], what + ": states")
                assert got[7] == NB


@pytest.mark.parametrize("mode", ["am", "ssb"])
@pytest.mark.parametrize("generic", [False, True])
def test_three_ways_are_reached(ctx, mode, generic):
    """an AM channel's first closed block is the ramp (non-zero pre_agc), the closed blocks behind it are +0.  Channels whose gain set_channel put to 1e6, NaN,
    +inf, 1 and 0.003 are closed for 20 blocks (1e6 at the defaults: the cycle of period 2; with alpha 0.99: period 3), then reopen, and their audio and
    state equal the reference walk's bits: the state came through the shortcut"""
    import csdr_amd
    B, n_ch = 64, 5
    x = qm.make_input(mode, n_ch, NB, B)
    lv = np.full(n_ch, qm.LEVEL, f32)
    P = csdr_amd.amssb_params(mode, B)
    got = _run_gated(ctx, P, x, 1, lv, 4, generic)
    _check(got, _walked(P, x, 1, lv), "the pattern input")
    seen = set()
    for c in range(n_ch):
        means = np.abs(x[c]).reshape(-1, B).mean(axis=1)
        for k, way in enumerate(qm.classify(mode, got[4][c], means)):
            blk = got[1][c, k * B:(k + 1) * B]
            seen.add(way)
            if way == "ramp":
                assert np.abs(blk).max() > 0.1 and blk[-1] != 0, "channel %d block %d is the ramp" % (c, k)
            if way == "zero":
                assert not blk.any() and not np.signbit(blk).any() and not got[0][c, k * B:(k + 1) * B].any(), "channel %d block %d is +0" % (c, k)
    assert seen == ({"open", "ramp", "zero"} if mode == "am" else {"open", "zero"})

    gains = (1e6, np.nan, np.inf, 1.0, 0.003)
    x = qm.make_input(mode, n_ch, 24, B, seed=3, quiet=False)
    for agc in (mm.AGC_DEFAULT, (200, 0.2, 0.01, 0.0001, 65536.0, 0, 0.99)):
        P = csdr_amd.amssb_params(mode, B, agc)
        states = [(0.0, g) for g in gains]
        changes = {c: {19: 0.0} for c in range(n_ch)}
        closed = np.full(n_ch, qm.ALL_CLOSED, f32)
        want = _walked(P, x, 1, closed, changes, states)
        assert not want[3][:, :20].any() and want[3][:, 20:].all()
        with csdr_amd.AmSsb(ctx, P, n_ch, max_samples_per_call=20 * B, squelch=True, levels=closed) as o:
            o.force_generic(generic)
            for c, st in enumerate(states):
                o.set_channel(c, csdr_amd.AmSsbChan(*st))
            got = o.process_squelched(x, calls=[20 * B, 4 * B], levels_between={1: [(-1, 0.0)]})
            _check(got, want, "%s alpha %g" % (mode, agc[6]), 24 * B)
            assert set(got[5]) == {_name(mode, not generic)}
            _same_states(_states(o), want[4], "states behind the reopening")
        zero = got[1][:, :20 * B]
        assert not zero.any() and not np.signbit(zero).any() and not got[0][:, :20 * B].any(), "zero blocks are +0"
        assert got[0][0, 20 * B:].any() and got[0][3, 20 * B:].any(), "the reopened channels have audio"
        # the gain that met the reopening is the plain iteration's: 20 blocks of B - 1 steps each (agc_ff's call begins with last_gain as it is)
        g = f32(1e6)
        for _ in range(20):
            g = qm.iterate(agc[6], agc[4], g, B - 1)
        st = csdr_amd.AmSsbChan(0.0, float(g))
        w16, _ = csdr_amd.amssb_debug_walk(P, x[0, 20 * B:], st)
        mm.assert_bits(got[0][0, 20 * B:], w16, "audio behind 20 zero blocks, from the plainly iterated gain")


@pytest.mark.parametrize("mode", ["am", "ssb"])
def test_levels_resets_and_refusals(ctx, mode):
    """level 0 everywhere is the unsquelched object; an all-closed bank gives zeros; level changes with a partial block held and with none against
    csdr_amd.Squelch at the same call boundaries; the kernels alternating call by call; reset, reset_channel; the refusals"""
    import csdr_amd
    B, n_ch, d = 64, 5, 1
    P = csdr_amd.amssb_params(mode, B, mm.AGC_ALT)
    x = qm.make_input(mode, n_ch, NB, B)
    n = x.shape[1]
    with csdr_amd.AmSsb(ctx, P, n_ch, max_samples_per_call=n) as o:
        plain16, plainpre, _ = o.process(x)
        assert o.kernel_name() == _name(mode, True, sq=False)
        # the squelch calls on an object without one: each -3, and the object goes on as before
        for call in (lambda: o.set_squelch_level(0, 1.0), lambda: o.get_squelch_level(0), lambda: o.squelch_block_index(),
                     lambda: o.process_squelched_dev(None, 0, 0, None, None, 0)):
            with pytest.raises(csdr_amd.CsdrAmdError):
                call()
        # enable_squelch on an object that has taken samples: -3; after a reset it is accepted
        assert ctx.L.csdr_amd_amssb_enable_squelch(o.h, 1, None) == -3
        o.reset()
        assert ctx.L.csdr_amd_amssb_enable_squelch(o.h, 1, None) == 0
        got = o.process_squelched(x)
        assert got[5] == [_name(mode, True)]
        mm.assert_bits(got[0], plain16, "level 0: s16 of the unsquelched object"); mm.assert_bits(got[1], plainpre, "level 0: pre_agc")
        assert got[4].all()
    for out_pitch in (None, n + 3):                     # (rows that 16-byte stores can and cannot serve)
        got = _run_gated(ctx, P, x, d, np.full(n_ch, qm.ALL_CLOSED, f32), out_pitch=out_pitch)
        assert not got[0].any() and not got[4].any()
        mm.assert_bits(got[1], _walked(P, x, d, np.full(n_ch, qm.ALL_CLOSED, f32))[1], "pre_agc of an all-closed bank")
    # level changes: in front of call 1 a partial block is held (its level stays the old one), in front of call 2 none is
    calls = [2 * B + B // 2, 3 * B + B // 2, 4 * B, n - 10 * B]
    between = {1: [(0, qm.ALL_CLOSED), (3, 0.0)], 2: [(0, qm.LEVEL), (4, qm.ALL_CLOSED)], 3: [(-1, qm.LEVEL)]}
    lv = qm.levels(n_ch)
    sq_between = {k: [(c, v) for ch, v in lst for c in (range(n_ch) if ch < 0 else [ch])] for k, lst in between.items()}
    want = _composed(ctx, P, x, d, lv, calls=calls, levels_between=sq_between)
    _check(_run_gated(ctx, P, x, d, lv, calls=calls, levels_between=between), want, "level changes", NB * B)
    got = _run_gated(ctx, P, x, d, lv, calls=calls, levels_between=between, generic_calls=(1, 3))
    _check(got, want, "level changes, alternating kernels", NB * B)
    assert got[5] == [_name(mode, True), _name(mode, False), _name(mode, True), _name(mode, False)]
    # reset keeps the levels and clears the block index and the held samples; reset_channel is the two state words
    want = _composed(ctx, P, x, d, lv)
    with csdr_amd.AmSsb(ctx, P, n_ch, max_samples_per_call=n, squelch=True, use_every_nth=d, levels=lv) as o:
        o.process_squelched(x[:, :5 * B + 7])
        assert o.squelch_block_index() == 5
        o.reset()
        assert o.squelch_block_index() == 0 and [o.get_squelch_level(c) for c in range(n_ch)] == [float(v) for v in lv]
        _check(o.process_squelched(x), want, "after reset", NB * B)
        o.reset()
        o.process_squelched(x[:, :4 * B])
        o.reset_channel(3)
        got = o.process_squelched(x[:, 4 * B:])
        assert o.squelch_block_index() == NB
        w3 = qm.expected(csdr_amd, P, x[3, 4 * B:], d, float(lv[3]))
        mm.assert_bits(got[0][3], w3[0], "the reset channel"); mm.assert_bits(got[0][0], want[0][0, 4 * B:], "another channel")
        # the refusals: each -3, nothing changed
        o.reset()
        o.process_squelched(x[:, :B + 9])
        before = (_states(o), o.squelch_block_index(), [o.get_squelch_level(c) for c in range(n_ch)])
        for call in (lambda: o.set_squelch_level(n_ch, 1.0), lambda: o.set_squelch_level(-2, 1.0), lambda: o.get_squelch_level(-1), lambda: o.get_squelch_level(n_ch)):
            with pytest.raises(csdr_amd.CsdrAmdError):
                call()
        assert ctx.L.csdr_amd_amssb_enable_squelch(o.h, 1, None) == -3
        di = ctx.upload(np.ascontiguousarray(x[:, B + 9:]))
        ds, dp, dg = ctx.alloc(2 * n * n_ch + 256), ctx.alloc(4 * n_ch * 64), ctx.alloc(n_ch * 64)
        with pytest.raises(csdr_amd.CsdrAmdError):      # power_pitch below the call's blocks
            o.process_squelched_dev(di.ptr, n - B - 9, n - B - 9, ds.ptr, None, n, dp.ptr, NB - 2, dg.ptr)
        assert (_states(o), o.squelch_block_index(), [o.get_squelch_level(c) for c in range(n_ch)]) == before
        _check(o.process_squelched(x[:, B + 9:]), tuple(w[:, B:] if k < 2 else w[:, 1:] for k, w in enumerate(want[:4])), "behind the refusals")


def _ssb_filter(ctx, lsb=False):
    nt = ctx.firdes_filter_len(0.05)
    fft = 1 << (nt - 1).bit_length()
    if fft - nt < 200:
        fft *= 2
    return ctx.firdes_bandpass_c(nt, -0.1 if lsb else 0.0, 0.0 if lsb else 0.1), fft


def test_u8_front_end(ctx):
    """the U8 form at constant levels against a separate front end -> Squelch -> the CF32 object driven with the same calls, in every bit"""
    import csdr_amd
    n, D, B, n_ch, d = 1024 * 120, 50, 256, 3, 3
    calls = [1024 * 70, 1024 * 50]
    carriers = 0.25 - 0.03 * np.arange(n_ch)
    u8 = mm.am_test_signal(n, 15, carriers, n_ch)
    u8[2, :] = 0x80 + ((u8[2, :].astype(np.int16) - 0x80) // 16).astype(np.int16)      # a weak channel
    taps = ctx.firdes_lowpass_f(ctx.firdes_filter_len(0.005), 0.5 / D)
    rates = -carriers.astype(f32)
    P = csdr_amd.amssb_params("am", B)
    y = ctx.ddc_u8(u8, rates.copy(), D, taps, block=calls)
    pw = [sm.power64(y[c, k * B:(k + 1) * B], d) for c in range(n_ch) for k in range(y.shape[1] // B)]
    lv = np.array([0.0, 1e3, np.sqrt(min(pw[:9]) * max(pw[-9:]))], f32)      # open, closed, and between the strong channel's power and the weak one's
    assert all(not sm.undecidable(B, d, p, float(lv[2])) for p in pw)
    with ctx.am_bank(n_ch, B, in_format="u8", shift_rate=rates.copy(), decimation=D, ddc_taps=taps, max_samples_per_call=max(calls), squelch=True, use_every_nth=d,
                     levels=lv) as o:
        got = o.process_squelched(u8, calls=calls)
        assert set(got[5]) == {"k_amssb_tiled_sq<AM>"} and o.front_end_kernel() != ""
    m = y.shape[1] // B * B
    want = _composed(ctx, P, y[:, :m], d, lv)
    _check(got, want, "u8", m)
    assert got[4][0].all() and not got[4][1].any() and not got[4][2].any()


def test_ssb_owned_filter(ctx):
    """the SSB form with an owned filter at constant levels against FftFilt -> Squelch -> the CF32 object: flags exact, pre_agc within 1e-5 relative RMS (the
    gate of the unsquelched object's own filter test), s16 against the walk on the object's own pre_agc in every bit"""
    import csdr_amd
    import oracle
    n_ch, n, B, d = 3, 12000, 256, 1
    taps, fft = _ssb_filter(ctx)
    rng = np.random.default_rng(61)
    t = np.arange(n)
    amp = (0.3, 0.3, 0.003)
    x = np.stack([(amp[c] * np.exp(2j * np.pi * (0.03 + 0.02 * c) * t) * (1 + 0.5 * np.sin(2 * np.pi * t / (900.0 + 100 * c)))
                   + amp[c] / 6 * (rng.normal(size=n) + 1j * rng.normal(size=n))).astype(c64) for c in range(n_ch)])
    lv = np.array([0.01, 10.0, 0.01], f32)
    P = csdr_amd.amssb_params("ssb", B)
    inp = fft - taps.size + 1
    with csdr_amd.FftFilt(ctx, fft, taps, n_ch, n // inp) as f:
        y = f.process(x)
    m = y.shape[1] // B * B
    want = _composed(ctx, P, y[:, :m], d, lv)
    for c in range(n_ch):
        assert qm.undecidable_blocks(y[c, :m], B, d, float(lv[c])) == []
    for calls in ([n], [5000, 3, n - 5003]):
        with ctx.ssb_bank(n_ch, B, taps=taps, fft_size=fft, max_samples_per_call=n, squelch=True, use_every_nth=d, levels=lv) as o:
            s16, pre, counts, pw, fl, names = o.process_squelched(x, calls=calls)
        assert sum(counts) == m and set(names) == {"k_amssb_tiled_sq<SSB>"}
        assert np.array_equal(fl, want[3]) and fl[0].all() and not fl[1:].any()
        for c in range(n_ch):
            e = oracle.relrms(pre[c], want[1][c]) if want[1][c].any() else float(np.abs(pre[c]).max())
            assert e <= 1e-5, "pre_agc of channel %d: %g" % (c, e)
            w16, _ = csdr_amd.amssb_debug_walk(P, pre[c].astype(c64))
            mm.assert_bits(s16[c], w16, "s16 on the object's own pre_agc")
            for k in range(m // B):
                p64 = sm.power64(y[c, k * B:(k + 1) * B], d)
                assert abs(float(pw[c, k]) - p64) <= sm.bound(B, d, p64) + 4e-5 * p64      # (the filter's own 1e-5 relative RMS, squared, with room)


def _run_cli(tmp_path, args, sig, ctl_lines=None):
    outs = []
    keep = None
    if ctl_lines is not None:
        ctl = tmp_path / "ctl.fifo"; os.mkfifo(ctl)
        keep = os.open(ctl, os.O_RDWR)                  # keeps the fifo open for writing while the command runs
        os.write(keep, ctl_lines)
        args = args[:-1] + ["--ctl", str(ctl)] + args[-1:]
    for k in range(len(sig)):
        fi = tmp_path / ("in%d.u8" % k); fo = tmp_path / ("out%d.s16" % k)
        sig[k].tofile(fi); outs.append(fo); args = args + [str(fi), str(fo)]
    env = dict(os.environ, CSDR_AMD_BANK_BLOCK="65536")
    try:
        p = subprocess.run([CLI] + args, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    finally:
        if keep is not None:
            os.close(keep)
    assert p.returncode == 0, p.stderr.decode()
    return [np.fromfile(o, np.int16) for o in outs], p.stderr


def _bank(ctx, cmd, n_ch, rates, **kw):
    taps = ctx.firdes_lowpass_f(ctx.firdes_filter_len(0.005), 0.5 / 50)
    kw = dict(in_format="u8", shift_rate=np.asarray(rates, f32), decimation=50, ddc_taps=taps, max_samples_per_call=65536, **kw)
    if cmd.startswith("am"):
        return ctx.am_bank(n_ch, **kw)
    bp, fft = _ssb_filter(ctx)
    return ctx.ssb_bank(n_ch, taps=bp, fft_size=fft, **kw)


@pytest.mark.parametrize("cmd", ["am_bank_u8_s16", "ssb_bank_u8_s16"])
def test_cli(ctx, tmp_path, cmd):
    """`csdr <cmd> --squelch 1 1 <smeter>` with a control line "1 squelch <level>" against the Python object making the same calls: the audio byte for byte and
    the report lines; the command without --squelch against the unsquelched object"""
    n = 3 * 65536 + 5 * 1024
    u8 = [mm.am_test_signal(n, 800 + k, 0.25 - 0.05 * k)[0] for k in range(2)]
    rates = [-0.25, -0.2]
    calls = [65536] * 3 + [5 * 1024]
    smeter = tmp_path / "smeter.txt"
    got, err = _run_cli(tmp_path, [cmd, "--squelch", "1", "1", str(smeter), ",".join("%g" % r for r in rates)], u8, ctl_lines=b"1 squelch 1000\n")
    assert b"stream 1 squelch level is 1000" in err
    with _bank(ctx, cmd, 2, rates, squelch=True, use_every_nth=1) as o:
        s16, _, counts, pw, fl, names = o.process_squelched(np.stack(u8), calls=calls, with_pre=False, in_pitch=2 * 65536 * len(calls), levels_between={0: [(1, 1000.0)]})
    assert s16.shape[1] >= 3 * 1024 and fl[0].all() and not fl[1].any() and not s16[1].any() and s16[0].any()
    for k in range(2):
        assert got[k].tobytes() == s16[k].tobytes(), "stream %d: %d samples against %d" % (k, got[k].size, s16.shape[1])
    lines = "".join("%d %g\n" % (ch, pw[ch, k]) for k in sm.report_replay(1, pw.shape[1]) for ch in range(2))
    assert lines and smeter.read_text() == lines
    plain, _ = _run_cli(tmp_path, [cmd, ",".join("%g" % r for r in rates)], u8)
    with _bank(ctx, cmd, 2, rates) as o:
        w16, _, _ = o.process(np.stack(u8), calls=calls, with_pre=False, in_pitch=2 * 65536 * len(calls))
    for k in range(2):
        assert plain[k].tobytes() == w16[k].tobytes(), "without --squelch: stream %d" % k
