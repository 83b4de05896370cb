"""The squelched WFM receive bank on the GPU (csdr_amd_wfmrx_create_squelched / csdr_amd.WfmRx(squelch_block=...)): the fused path, the generic path and the
composition csdr_amd.Squelch -> csdr_amd.WfmRx in every bit, under every cut of the stream into calls; all of them against the oracle's chain on the model's
gated stream; the levels, the resets, the refusals, behind the channelizer and the two commands.  The shapes are the smallest at which a path can still go
wrong: one channel, a partly filled group of the front kernel's 8 channels, two groups plus one channel (which also crosses the tail's 16); 7 windows; squelch
blocks of 1024 (the window), of 300 (blocks that straddle output tiles, windows and calls; a boundary between two staged quads) and of 301 (a boundary inside
a quad, held counts of either parity)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import squelch_model as sm
import wfmrx_model as wm
import wfmrx_squelch_model as wsm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
FUSED, GENERIC = "k_wfmrx_front_sq", "k_fracdec"
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    assert c.arch().startswith("gfx950")
    yield c
    c.close()


_inputs, _expected = {}, {}


def case_input(n_ch, seed=0, n=wsm.N):
    key = (n_ch, seed, n)
    if key not in _inputs:
        x = wsm.make_input(n_ch, n, seed)
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]


def case_expected(port, n_ch, c, B, d, rate=5, P=12):
    """the oracle's chain on the gated stream of channel c of case_input(n_ch) at its level, computed once"""
    key = (n_ch, c, B, d, rate, P)
    if key not in _expected:
        _expected[key] = wsm.expected(port, case_input(n_ch)[c], B, d, wsm.levels(n_ch)[c], rate, P)
    return _expected[key]


def cut(n, calls):
    calls = [n] if calls is None else list(calls)
    if sum(calls) < n:
        calls.append(n - sum(calls))
    return calls


def run(ctx, x, B, d, lv, calls=None, generic=False, kernel=None, obj=None, rate=5, P=12, taps=None, levels_between=None, **kw):
    """x [n_channels, n] through one squelched object in calls of `calls` samples (the rest in one more); generic: a path for all calls, or one per call;
    levels_between: {call index: [(channel, level), ...]} applied in front of that call -> (s16, float audio, per-call audio counts, powers, flags).
    Every call's counts are checked against the two plans and max_output, its kernel_name against `kernel` (default: the path asked for)."""
    import csdr_amd
    x = np.atleast_2d(x)
    calls = cut(x.shape[1], calls)
    o = obj or csdr_amd.WfmRx(ctx, x.shape[0], rate=rate, num_poly_points=P, prefilter_taps=taps, max_samples_per_call=max(max(calls), 1), squelch_block=B, use_every_nth=d,
                              levels=lv)
    nt = 0 if taps is None else len(taps)
    try:
        pcm, af, counts, pws, fls, at = [], [], [], [], [], 0
        for i, k in enumerate(calls):
            g = generic[i % len(generic)] if isinstance(generic, (list, tuple)) else generic
            o.force_generic(g)
            for ch, level in (levels_between or {}).get(i, ()):
                o.set_squelch_level(ch, level)
            assert csdr_amd.wfmrx_squelch_plan(o.squelch_held(), k, B) == wsm.squelch_plan(o.squelch_held(), k, B)
            want = wsm.plan(rate, P, nt, wm.W, o.where(), o.held(), o.squelch_held(), k, B)
            blocks_before = o.squelch_block_index()
            s16, f, got, pw, fl = o.process_squelched(x[:, at:at + k], with_float=True, **kw)
            assert (got, o.where(), o.held(), o.squelch_held(), pw.shape[1]) == want and fl.shape == pw.shape and got <= o.max_output(k) == o.max_out(k)
            assert o.squelch_block_index() == blocks_before + want[4]
            if k:
                assert o.kernel_name() == (kernel or (GENERIC if g else FUSED))
            pcm.append(s16); af.append(f); counts.append(got); pws.append(pw); fls.append(fl); at += k
        return np.concatenate(pcm, axis=1), np.concatenate(af, axis=1), counts, np.concatenate(pws, axis=1), np.concatenate(fls, axis=1)
    finally:
        if obj is None:
            o.close()


def composed(ctx, x, B, d, lv, calls=None, levels_between=None, rate=5, P=12, taps=None, generic=False):
    """csdr_amd.Squelch into a second row buffer, csdr_amd.WfmRx over it, call by call -> run()'s tuple"""
    import csdr_amd
    x = np.atleast_2d(x)
    s = x.shape[0]
    calls = cut(x.shape[1], calls)
    pcm, af, counts, pws, fls, at = [], [], [], [], [], 0
    with csdr_amd.Squelch(ctx, s, B, d, lv, max_samples_per_call=max(max(calls), 1)) as sq, \
            csdr_amd.WfmRx(ctx, s, rate=rate, num_poly_points=P, prefilter_taps=taps, max_samples_per_call=max(calls) + B) as rx:
        rx.force_generic(generic)
        for i, k in enumerate(calls):
            for ch, level in (levels_between or {}).get(i, ()):
                sq.set_level(ch, level)
            if k:
                g, pw, fl = sq.process(x[:, at:at + k])
                g, pw, fl = np.stack(g), np.stack(pw), np.stack(fl)
            else:
                g, pw, fl = np.zeros((s, 0), np.complex64), np.zeros((s, 0), f32), np.zeros((s, 0), np.uint8)
            if g.shape[1]:
                s16, f, got = rx.process(g, with_float=True)
            else:
                s16, f, got = np.zeros((s, 0), np.int16), np.zeros((s, 0), f32), 0
            pcm.append(s16); af.append(f); counts.append(got); pws.append(pw); fls.append(fl); at += k
    return np.concatenate(pcm, axis=1), np.concatenate(af, axis=1), counts, np.concatenate(pws, axis=1), np.concatenate(fls, axis=1)


def same_bits(a, b, counts=True):
    return (a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and (a[2] == b[2] or not counts)
            and a[3].shape == b[3].shape and np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32)) and np.array_equal(a[4], b[4]))


def short_calls(B):
    """calls of a third of a block: two in three complete no block"""
    return [B // 3] * 7


def n_out_of(B, rate=5, P=12):
    return wm.plan(rate, P, 0, wm.W, wm.fresh_where(P), 0, wsm.N // B * B)[0]


# ---------------------------------------------------------------- 1. fused = generic = composed, in every bit
@pytest.mark.parametrize("n_ch,B,d", wsm.SHAPES + [(17, 301, 1)])
def test_wfmrx_squelch_paths_and_composition_same_bits(ctx, n_ch, B, d):
    x, lv = case_input(n_ch), wsm.levels(n_ch)
    for calls in (None, wsm.RAGGED, short_calls(B)):
        a, b, c = run(ctx, x, B, d, lv, calls), run(ctx, x, B, d, lv, calls, generic=True), composed(ctx, x, B, d, lv, calls)
        assert sum(a[2]) == n_out_of(B) and a[3].shape == (n_ch, wsm.N // B), calls
        assert same_bits(a, b) and same_bits(a, c), calls
        if calls is not None and calls[0] < B:
            assert a[2][0] == 0 and a[3].shape[1] > 0
    assert 0 < a[4][0].sum() < a[4][0].size
    if n_ch > 5:
        assert not a[4][4].any() and a[4][5].all() and not a[4][2].any()


def test_wfmrx_squelch_closed_block_follows_an_open_one_inside_a_quad(ctx):
    """B = 301: block boundaries at every residue mod 4 of the staged row, so quads of four staged samples hold the end of an open block and the start of a
    closed one (and the reverse); B = 300: the boundary falls between two quads and only the demodulator's previous sample comes from the other block;
    B = 1024 = the window: a closed block (block 1) ends exactly on a window boundary"""
    x, lv = case_input(17), wsm.levels(17)
    for B in (300, 301, 1024):
        a = run(ctx, x, B, 1, lv)
        assert same_bits(a, composed(ctx, x, B, 1, lv))
        fl = a[4][0].astype(int)
        falls = [k for k in range(1, fl.size) if fl[k - 1] == 1 and fl[k] == 0]
        rises = [k for k in range(1, fl.size) if fl[k - 1] == 0 and fl[k] == 1]
        assert falls and rises
        if B == 301:
            assert {(k * B) % 4 for k in falls + rises} - {0}
        if B == 1024:
            assert falls[0] == 1 and rises[0] == 2 and B == wm.W


# ---------------------------------------------------------------- 2. against the oracle
def check_against_oracle(got, want, x_row, B, d, what):
    pcm, af, pw, fl = got
    want_s16, want_af, want_pw, want_fl = want
    assert np.array_equal(fl, want_fl), what
    for k in range(want_pw.size):
        P = sm.power64(x_row[k * B:(k + 1) * B], d)
        assert abs(float(pw[k]) - P) <= sm.bound(B, d, P), (what, k)
    if not want_fl.any():                                               # every block closed: silence, exactly
        assert not want_s16.any() and not pcm.any() and not af.any() and af.size == want_af.size > 0
    else:
        wm.assert_gates(pcm, af, want_s16, want_af, what=what)


@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
@pytest.mark.parametrize("n_ch,B,d", [(1, 1024, 1), (5, 300, 3), (17, 1024, 3), (17, 300, 1), (17, 301, 1)])
def test_wfmrx_squelch_against_oracle(ctx, port, n_ch, B, d, generic):
    x, lv = case_input(n_ch), wsm.levels(n_ch)
    pcm, af, counts, pw, fl = run(ctx, x, B, d, lv, generic=generic)
    assert counts == [n_out_of(B)]
    for c in range(n_ch):
        check_against_oracle((pcm[c], af[c], pw[c], fl[c]), case_expected(port, n_ch, c, B, d), x[c], B, d,
                             "%s ch %d (%s) B %d d %d" % ("generic" if generic else "fused", c, wm.KINDS[c % 4], B, d))


@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
@pytest.mark.parametrize("rate,P", [(2.5, 12), (5.2083335, 12), (3.3, 12), (5, 4)])
def test_wfmrx_squelch_against_oracle_rates_and_orders(ctx, port, rate, P, generic):
    n_ch, B, d = 5, 300, 1
    x, lv = case_input(n_ch), wsm.levels(n_ch)
    pcm, af, counts, pw, fl = run(ctx, x, B, d, lv, generic=generic, rate=rate, P=P)
    assert counts == [n_out_of(B, rate, P)]
    for c in range(n_ch):
        check_against_oracle((pcm[c], af[c], pw[c], fl[c]), case_expected(port, n_ch, c, B, d, rate, P), x[c], B, d,
                             "%s ch %d (%s) @ %g / %d" % ("generic" if generic else "fused", c, wm.KINDS[c % 4], rate, P))


# ---------------------------------------------------------------- 3. level 0 everywhere: the unsquelched bank on the first m samples
@pytest.mark.parametrize("B", [1024, 300])
def test_wfmrx_squelch_level_zero_equals_unsquelched(ctx, B):
    import csdr_amd
    x = case_input(17)
    m = wsm.N // B * B
    with csdr_amd.WfmRx(ctx, 17, max_samples_per_call=m) as o:
        want = o.process(x[:, :m], with_float=True)
        assert o.kernel_name() == "k_wfmrx_front"
    for generic in (False, True):
        got = run(ctx, x, B, 1, None, wsm.RAGGED, generic=generic)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and sum(got[2]) == want[2]
        assert got[4].all()


# ---------------------------------------------------------------- 4. set_squelch_level between calls
@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
def test_wfmrx_squelch_level_changes_between_calls(ctx, generic):
    """B = 1024.  In front of call 1, with 500 samples of block 0 held, channel 0 goes to ALL_CLOSED and channel 4 (all closed so far) to 0: block 0 stays under
    the levels it started with, block 1 and later have the new ones.  In front of call 3, with nothing held (3072 samples in), channel 0 returns to LEVEL:
    block 3 has it, and block 2, open at LEVEL, was closed.  The model's `changes` say the same: {0: new} is read behind block 0, {2: new} behind block 2."""
    import csdr_amd
    B, x, lv = 1024, case_input(17), wsm.levels(17)
    calls = [500, 1000, 1572, 2000]
    between = {1: [(0, wsm.ALL_CLOSED), (4, 0.0)], 3: [(0, wsm.LEVEL)]}
    got = run(ctx, x, B, 1, lv, calls, generic=generic, levels_between=between)
    assert same_bits(got, composed(ctx, x, B, 1, lv, calls, levels_between=between))
    want0 = wsm.gated(x[0], B, 1, wsm.LEVEL, {0: wsm.ALL_CLOSED, 2: wsm.LEVEL})[2]
    want4 = wsm.gated(x[4], B, 1, wsm.ALL_CLOSED, {0: 0.0})[2]
    assert np.array_equal(got[4][0], want0) and np.array_equal(got[4][4], want4)
    assert list(want0[:4]) == [1, 0, 0, 1] and list(want4[:3]) == [0, 1, 1]
    with csdr_amd.WfmRx(ctx, 3, squelch_block=B, levels=[0.5, 0.25, 0.125]) as o:
        assert [o.get_squelch_level(c) for c in range(3)] == [0.5, 0.25, 0.125]
        o.set_squelch_level(-1, 2.0)
        assert [o.get_squelch_level(c) for c in range(3)] == [2.0, 2.0, 2.0]
        o.set_squelch_level(1, 0.0)
        assert [o.get_squelch_level(c) for c in range(3)] == [2.0, 0.0, 2.0]
        for bad in (3, -2):
            with pytest.raises(csdr_amd.CsdrAmdError, match="wfmrx: channel out of range"):
                o.set_squelch_level(bad, 1.0)


# ---------------------------------------------------------------- 5. paths alternating call by call
@pytest.mark.parametrize("B,d", [(300, 1), (1024, 3), (301, 1)])
def test_wfmrx_squelch_paths_alternate_within_a_stream(ctx, B, d):
    """the held squelch samples and the held demodulated floats move between the two paths' buffers"""
    x, lv = case_input(17), wsm.levels(17)
    calls = [341, 100, 1500, 900, 150, 2100, 64]
    ref = run(ctx, x, B, d, lv, calls, generic=True)
    for order in ([False, True], [True, False]):
        assert same_bits(run(ctx, x, B, d, lv, calls, generic=order), ref), order


# ---------------------------------------------------------------- 6. reset_channel, reset
@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
def test_wfmrx_squelch_reset_channel_and_reset(ctx, generic):
    """B = 64, first call 39 blocks + 4: two windows out, then the decimator holds some hundred floats and the squelch 4 samples.  reset_channel(1) leaves
    channel 1 with zeros in all of them and no history, 4 samples into a squelch block: so is a fresh channel fed `first` zero samples.  (A zero block is
    silence open or closed; the block under way, 4 zeros and 60 samples, is judged in both.)"""
    import csdr_amd
    B, first = 64, 39 * 64 + 4
    x = case_input(3, seed=3)
    lv = np.array([wsm.LEVEL, wsm.LEVEL, 0.0], f32)
    undisturbed = run(ctx, x, B, 1, lv, [first], generic=generic)
    with csdr_amd.WfmRx(ctx, 3, max_samples_per_call=x.shape[1], squelch_block=B, levels=lv) as o:
        a = run(ctx, x[:, :first], B, 1, lv, obj=o, generic=generic)
        assert a[2] == [404] and 0 < o.held() < wm.W and o.squelch_held() == 4 and o.squelch_block_index() == 39
        state = (o.held(), o.where(), o.squelch_held(), o.squelch_block_index())
        o.reset_channel(1)
        assert (o.held(), o.where(), o.squelch_held(), o.squelch_block_index()) == state
        b = run(ctx, x[:, first:], B, 1, lv, obj=o, generic=generic)
        fresh = run(ctx, np.concatenate([np.zeros((1, first), np.complex64), x[1:2, first:]], axis=1), B, 1, lv[1:2], [first], generic=generic)
        assert fresh[2] == a[2] + b[2] and not fresh[0][0, :404].any()
        assert np.array_equal(b[0][1], fresh[0][0, 404:]) and np.array_equal(b[1][1].view(np.uint32), fresh[1][0, 404:].view(np.uint32))
        assert np.array_equal(b[3][1].view(np.uint32), fresh[3][0][39:].view(np.uint32)) and np.array_equal(b[4][1], fresh[4][0][39:])
        for c in (0, 2):
            for j in (0, 1, 3, 4):
                assert np.array_equal(np.concatenate([a[j][c], b[j][c]]), undisturbed[j][c]), (c, j)
        o.reset()
        assert (o.held(), o.where(), o.squelch_held(), o.squelch_block_index()) == (0, 5.0, 0, 0) and o.get_squelch_level(1) == float(f32(wsm.LEVEL))
        assert same_bits(run(ctx, x, B, 1, lv, [first], obj=o, generic=generic), undisturbed)


# ---------------------------------------------------------------- 7. a long closed tail behind an open block
def test_wfmrx_squelch_long_closed_tail(ctx, port):
    """one fm channel whose samples from 1024 on are scaled by 0.05, B = 1024 at LEVEL: one open block, then 6144 closed samples, through which the de-emphasis
    state decays into the smallest floats.  The two paths and the composition agree in every bit there; against the oracle the gates only (its host build
    flushes subnormals to zero, the GPU's float path is not asked to)."""
    x = wm.make_input(1, wsm.N).copy()
    x[:, 1024:] *= f32(0.05)
    a, b, c = run(ctx, x, 1024, 1, [wsm.LEVEL]), run(ctx, x, 1024, 1, [wsm.LEVEL], generic=True), composed(ctx, x, 1024, 1, [wsm.LEVEL])
    assert same_bits(a, b) and same_bits(a, c)
    assert "".join(str(v) for v in a[4][0]) == "1000000"
    want_s16, want_af, _, want_fl = wsm.expected(port, x[0], 1024, 1, wsm.LEVEL)
    assert np.array_equal(a[4][0], want_fl) and np.abs(want_af[-200:]).max() < 1e-30
    wm.assert_gates(a[0][0], a[1][0], want_s16, want_af, what="long closed tail")
    assert not a[0][0, -1000:].any()


# ---------------------------------------------------------------- 8. shapes that leave the fused path
def test_wfmrx_squelch_shapes_that_leave_the_fused_kernel(ctx):
    B, x, lv = 300, case_input(5), wsm.levels(5)
    n = x.shape[1]
    ref = composed(ctx, x, B, 1, lv, wsm.RAGGED)                                                          # the composition itself, not the object's generic run
    assert same_bits(run(ctx, x, B, 1, lv, wsm.RAGGED, generic=True), ref)
    odd, even = n | 1, (n + 3) & ~1
    assert same_bits(run(ctx, x, B, 1, lv, wsm.RAGGED, kernel=GENERIC, in_pitch=odd), ref)               # rows off 16-byte boundaries
    assert same_bits(run(ctx, x, B, 1, lv, wsm.RAGGED, kernel=GENERIC, in_offset=8), ref)                 # the base 8 bytes off
    assert same_bits(run(ctx, x, B, 1, lv, wsm.RAGGED, kernel=FUSED, in_pitch=even, in_offset=16), ref)  # (an even pitch on an aligned base stays)
    p18 = run(ctx, x, B, 1, lv, wsm.RAGGED, kernel=GENERIC, P=18)                                         # more points than the front kernel has
    assert same_bits(p18, composed(ctx, x, B, 1, lv, wsm.RAGGED, P=18)) and sum(p18[2]) > 1000
    rate = 5.2083335
    taps = wm.prefilter_taps(rate)
    pre = run(ctx, x, B, 1, lv, wsm.RAGGED, kernel=GENERIC, rate=rate, taps=taps)                         # a prefilter
    assert same_bits(pre, composed(ctx, x, B, 1, lv, wsm.RAGGED, rate=rate, taps=taps)) and sum(pre[2]) > 1000


def test_wfmrx_squelch_plain_process_is_the_same_call(ctx):
    import csdr_amd
    B, x, lv = 300, case_input(17), wsm.levels(17)
    ref = run(ctx, x, B, 1, lv, wsm.RAGGED)
    for generic in (False, True):
        with csdr_amd.WfmRx(ctx, 17, max_samples_per_call=x.shape[1], squelch_block=B, levels=lv) as o:
            o.force_generic(generic)
            parts, at = [], 0
            for k in cut(x.shape[1], wsm.RAGGED):
                parts.append(o.process(x[:, at:at + k], with_float=True)); at += k
            assert o.kernel_name() == (GENERIC if generic else FUSED) and o.squelch_block_index() == wsm.N // B
            assert [p[2] for p in parts] == ref[2] and np.array_equal(np.concatenate([p[0] for p in parts], axis=1), ref[0])
            assert np.array_equal(np.concatenate([p[1] for p in parts], axis=1).view(np.uint32), ref[1].view(np.uint32))


# ---------------------------------------------------------------- 9. every CU busy
def test_wfmrx_squelch_paths_same_bits_with_every_cu_busy(ctx, port):
    """1024 channels x 8 blocks of 1024 and 108 samples, rows tiled from 16, as tests/test_wfmrx_gpu.py's: 128 channel groups x 7 output tiles of the gated front
    kernel, 2048 workgroups of the power kernel"""
    n = 8300
    rows, lv16 = case_input(16, seed=5, n=n), wsm.levels(16)
    x, lv = np.tile(rows, (64, 1)), np.tile(lv16, 64)
    a, b = run(ctx, x, 1024, 1, lv), run(ctx, x, 1024, 1, lv, generic=True)
    assert a[2] == [wm.plan(5, 12, 0, wm.W, 5.0, 0, 8192)[0]] and a[3].shape == (1024, 8) and same_bits(a, b)
    assert np.array_equal(a[0][:16], a[0][1008:]) and not np.array_equal(a[0][0], a[0][1]) and 0 < a[4][0].sum() < a[4][0].size
    for c in (0, 1, 3, 4, 5, 7, 520, 1023):
        want = wsm.expected(port, x[c], 1024, 1, lv[c])
        check_against_oracle((a[0][c], a[1][c], a[3][c], a[4][c]), want, x[c], 1024, 1, "busy ch %d" % c)


# ---------------------------------------------------------------- 10. the refusals
def test_wfmrx_squelch_refusals(ctx):
    import csdr_amd
    L = ctx.L
    for B, d, msg in ((0, 1, "wfmrx: squelch_block should be 1 .. 65536"), (65537, 1, "wfmrx: squelch_block"), (-1, 1, "wfmrx: squelch_block"), (1024, 0, "wfmrx: use_every_nth"),
                      (1024, -3, "wfmrx: use_every_nth")):
        assert L.csdr_amd_wfmrx_create_squelched(ctx.h, 2, 5.0, 12, None, 0, 1024, 50e-6, 48000, 4096, B, d, None) is None and msg in ctx.err()
    assert L.csdr_amd_wfmrx_create_squelched(ctx.h, 2, 1.0, 12, None, 0, 1024, 50e-6, 48000, 4096, 1024, 1, None) is None and "wfmrx: rate should be > 1" in ctx.err()
    with pytest.raises(csdr_amd.CsdrAmdError, match="wfmrx: use_every_nth"):
        csdr_amd.WfmRx(ctx, 2, squelch_block=1024, use_every_nth=0)
    with pytest.raises(csdr_amd.CsdrAmdError, match="wfmrx: squelch_block"):
        csdr_amd.WfmRx(ctx, 2, squelch_block=1 << 17)
    x = wsm.make_input(2, 4096)
    di, ds, dp, dg = ctx.upload(x), ctx.alloc(2 * 2 * 4096 + 256), ctx.alloc(4 * 2 * 16), ctx.alloc(2 * 16)
    with ctx.wfm_rx(2, max_samples_per_call=3000, squelch_block=300, levels=[wsm.LEVEL, 0.0]) as o:
        assert o.process_squelched_dev(di.ptr, 4096, 100, ds.ptr, None, 4096, dp.ptr, 0, dg.ptr) == (0, 0) and o.squelch_held() == 100     # (no block: no pitch needed)
        state = (o.held(), o.where(), o.squelch_held(), o.squelch_block_index())
        for power, flags in ((dp.ptr, None), (None, dg.ptr), (dp.ptr, dg.ptr)):
            assert L.csdr_amd_wfmrx_process_squelched(o.h, di.at(800), 4096, 2900, ds.ptr, None, 4096, power, 9, flags, None) == -3
            assert "wfmrx: power_pitch 9 below the 10 squelch blocks of this call" in ctx.err()
        assert L.csdr_amd_wfmrx_process_squelched(o.h, di.at(800), 4096, 3001, ds.ptr, None, 4096, None, 0, None, None) == -3 and "wfmrx: n_in should be 0 .. " in ctx.err()
        assert L.csdr_amd_wfmrx_process_squelched(o.h, di.at(800), 4096, 2900, ds.ptr, None, 403, None, 0, None, None) == -3 and "wfmrx: out_pitch 403 smaller than the 404" in ctx.err()
        assert (o.held(), o.where(), o.squelch_held(), o.squelch_block_index()) == state                           # a refused call changes nothing
        assert o.process_squelched_dev(di.at(800), 4096, 2900, ds.ptr, None, 4096, dp.ptr, 10, dg.ptr) == (404, 10) and o.squelch_held() == 0
        assert o.max_output(3000) == (1024 + 3000 + 299) // 5 + 2 and o.max_output(0) == 0
    with ctx.wfm_rx(2, max_samples_per_call=3000) as o:                  # an object without a squelch
        state = (o.held(), o.where())
        assert L.csdr_amd_wfmrx_process_squelched(o.h, di.ptr, 4096, 3000, ds.ptr, None, 4096, None, 0, None, None) == -3 and "created without a squelch" in ctx.err()
        assert L.csdr_amd_wfmrx_set_squelch_level(o.h, 0, 1.0) == -3 and "created without a squelch" in ctx.err()
        assert L.csdr_amd_wfmrx_squelch_held(o.h) == -3 and L.csdr_amd_wfmrx_squelch_block_index(o.h) == -3
        for call in (lambda: o.process_squelched(x[:, :3000]), lambda: o.set_squelch_level(0, 1.0), lambda: o.get_squelch_level(0), o.squelch_held, o.squelch_block_index):
            with pytest.raises(csdr_amd.CsdrAmdError, match="created without a squelch"):
                call()
        assert (o.held(), o.where()) == state and o.process_dev(di.ptr, 4096, 3000, ds.ptr, None, 404) == 404 and o.max_output(3000) == (1024 + 3000) // 5 + 2


# ---------------------------------------------------------------- 11. behind the channelizer
def test_wfmrx_squelch_behind_the_channelizer(ctx, port):
    """a squelched WfmRx on ctx.fastddc_bank rows at the smallest channelizer geometry (transition_bw 0.05, decimation 2), call by call with the bank's counts;
    in front of the second call channel 1 goes to ALL_CLOSED with part of a block held.  Against the oracle chain on the model's gated stream of the bank's
    own rows, with the level change where the model reads it: behind the block under way."""
    D, tbw, rates, B = 2, 0.05, [0.1, 0.104, 0.097], 300
    ddc, _ = ctx.fastddc_init(tbw, D, 0.0)
    x = wsm.bank_input(16 * ddc.input_size)
    audio, powers, flags, y, counts = wsm.bank_composition(ctx, x, tbw, D, rates, 4, 5, B, 1, levels_between={1: [(1, wsm.ALL_CLOSED)]})
    assert len(counts) == 4 and sum(counts) >= 6 * wm.W and counts[0] % B
    got, fl = np.concatenate(audio, axis=1), np.concatenate(flags, axis=1)
    under_way = counts[0] // B                                           # the block that is under way at the level change keeps level 0
    for c in range(3):
        changes = {under_way: wsm.ALL_CLOSED} if c == 1 else None
        want_s16, want_af, want_pw, want_fl = wsm.expected(port, y[c][:sum(counts)], B, 1, 0.0, changes=changes)
        assert np.array_equal(fl[c], want_fl) and fl[c][:under_way + 1].all() and (c != 1) == bool(fl[c][under_way + 1:].all())
        d = np.abs(got[c].astype(np.int32) - want_s16.astype(np.int32))
        print("bank ch %d: %d samples, s16 max diff %d, differing %.4f %%" % (c, want_s16.size, d.max(), 100 * (d > 0).mean()))
        assert got[c].shape == want_s16.shape and want_s16.size > 1000 and np.abs(want_s16).max() > 1000
        assert d.max() <= 1 and (d > 0).mean() < wm.S16_FRACTION
    assert not fl[1][under_way + 1:].any() and not got[1][-256:].any()


# ---------------------------------------------------------------- 12. the two commands
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


def test_wfmrx_squelch_cli_bank_equals_python_composition(ctx, tmp_path):
    """`csdr fastddc_wfm_bank_s16 --squelch 300 1 1 <smeter>` on 3 channels at the smallest channelizer geometry against ctx.fastddc_bank -> the squelched WfmRx
    with the same blocks per call (wfmrx_squelch_model.bank_composition), which runs in a process of its own without torch (tests/test_wfmrx_gpu.py's bank test
    says why).  Channel 0's audio goes to a fifo: once the first batch's bytes have arrived the command waits for input, and the level line written then is
    applied in front of the second batch, as it is in the composition, with part of a block held: that block stays open, the later ones of channel 1 close.
    The audio files byte for byte, the S-meter lines against report_replay over the composition's powers."""
    import math
    assert os.path.exists(CSDR), "csdr_amd/csrc not built (make -C csdr_amd/csrc)"
    D, tbw, rates, B, every = 2, 0.05, [0.1, 0.104, 0.097], 300, 1
    ddc, _ = ctx.fastddc_init(tbw, D, 0.0)
    inp = ddc.input_size
    per = 1024 // math.gcd(inp, 1024)
    x = wsm.bank_input(2 * per * inp)
    env = {k: v for k, v in os.environ.items() if k != "CSDR_AMD_WORLD"}
    np.savez(str(tmp_path / "in.npz"), x=x, tbw=tbw, decimation=D, rates=rates, per=per, frac_rate=5.0, B=B, d=1, level_channel=1, level=wsm.ALL_CLOSED)
    c = subprocess.run(["timeout", "-k", "5", "120", sys.executable, os.path.join(ROOT, "tests", "wfmrx_squelch_model.py"), str(tmp_path / "in.npz"), str(tmp_path / "want.npz")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, CSDR_AMD_NO_TORCH_PRELOAD="1"), timeout=150)
    assert c.returncode == 0, c.stderr.decode()
    w = np.load(str(tmp_path / "want.npz"))
    want = [w["first"], w["second"]]
    assert not w["torch_loaded"]
    assert want[0].shape[1] > 0 and want[1].shape[1] > 0 and want[0].shape[1] + want[1].shape[1] >= 1000
    outs = [str(tmp_path / ("audio%d" % k)) for k in range(3)]
    ctl, smeter = str(tmp_path / "ctl"), str(tmp_path / "smeter")
    os.mkfifo(outs[0]); os.mkfifo(ctl)
    fo, fc = os.open(outs[0], os.O_RDWR | os.O_NONBLOCK), os.open(ctl, os.O_RDWR | os.O_NONBLOCK)
    args = ["timeout", "-k", "5", "90", CSDR, "fastddc_wfm_bank_s16", "--squelch", B, 1, every, smeter, D, tbw, "HAMMING", 5, 48000, "50e-6", ctl]
    for path, r in zip(outs, rates):
        args += [path, r]
    p = subprocess.Popen([str(a) for a in args], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, CSDR_AMD_BLOCK=str(per * inp)))
    try:
        p.stdin.write(x[:per * inp].tobytes()); p.stdin.flush()
        first = read_exactly(fo, 2 * want[0].shape[1])
        os.write(fc, ("1 squelch %g\n" % wsm.ALL_CLOSED).encode())
        p.stdin.write(x[per * inp:].tobytes()); p.stdin.close()
        second = read_exactly(fo, 2 * want[1].shape[1])
        assert p.wait(timeout=60) == 0, p.stderr.read().decode()
        err = p.stderr.read().decode()
    finally:
        if p.poll() is None:
            p.kill(); p.wait(timeout=10)
        os.close(fo); os.close(fc)
    assert "channel 1 squelch level is 10" in err
    want_all = np.concatenate(want, axis=1)
    assert first + second == want_all[0].tobytes()
    for k in (1, 2):
        assert open(outs[k], "rb").read() == want_all[k].tobytes(), k
    powers, flags = w["powers"], w["flags"]
    assert powers.shape[0] == 3 and powers.shape[1] >= 20 and open(smeter).read() == wsm.smeter_lines(powers, every)
    # the level line did something: channel 1 falls silent, the others are what they are without it
    plain = w["plain"]
    assert flags[0].all() and flags[2].all() and flags[1][0] == 1 and flags[1][-1] == 0
    assert np.array_equal(plain[0], want_all[0]) and np.array_equal(plain[2], want_all[2]) and not np.array_equal(plain[1], want_all[1])
    assert plain[1][-64:].any() and not want_all[1][-64:].any()


def single_stream_pipeline(tmp_path, tag, row, level_text, env):
    """`csdr squelch_and_smeter_cc --fifo <ctl> --outfifo <rep> 1 1 | csdr wfm_rx_cc_s16 5` on one channel's complexf row, the level waiting in the fifo
    -> (audio bytes, report text)"""
    ctl, rep = str(tmp_path / ("ctl_" + tag)), str(tmp_path / ("rep_" + tag))
    os.mkfifo(ctl); os.mkfifo(rep)
    fc, fr = os.open(ctl, os.O_RDWR), os.open(rep, os.O_RDONLY | os.O_NONBLOCK)
    try:
        os.write(fc, (level_text + "\n").encode())
        line = "%s squelch_and_smeter_cc --fifo %s --outfifo %s 1 1 | %s wfm_rx_cc_s16 5" % (CSDR, ctl, rep, CSDR)
        p = subprocess.run(["timeout", "-k", "5", "90", "sh", "-c", line], input=row.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
        assert p.returncode == 0, p.stderr.decode()
        data = b""
        try:
            while True:
                b = os.read(fr, 65536)
                if not b:
                    break
                data += b
        except BlockingIOError:
            pass
        return p.stdout, data.decode()
    finally:
        os.close(fc); os.close(fr)


def test_wfmrx_squelch_cli_bank_equals_single_stream_pipeline(ctx, tmp_path):
    """`csdr fastddc_wfm_bank_s16 --squelch 1024 1 1 <smeter>` against the reference's own topology per channel: the channel's row, as `csdr fastddc_bank_cc`
    of the same binary writes it for the same input and batches, through `csdr squelch_and_smeter_cc ... 1 1 | csdr wfm_rx_cc_s16 5` (block = the buffer size,
    1024).  The second half of the wide input is scaled by 0.05; channel 1 gets a level between its loud and its quiet block powers through the control channel
    before the first batch (the line waits in the fifo), channels 0 and 2 stay at 0.  Per channel: the audio bytes equal the bank command's file, and the
    pipeline's "%g" report lines equal the power column of that channel's "<channel> %g" lines."""
    import math
    assert os.path.exists(CSDR), "csdr_amd/csdr not built (make -C csdr_amd/csrc)"
    D, tbw, rates, B = 2, 0.05, [0.1, 0.104, 0.097], 1024
    ddc, _ = ctx.fastddc_init(tbw, D, 0.0)
    inp = ddc.input_size
    per = 1024 // math.gcd(inp, 1024)
    x = wsm.bank_input(2 * per * inp).copy()
    x[per * inp:] *= f32(0.05)
    env = {k: v for k, v in os.environ.items() if k not in ("CSDR_AMD_WORLD", "CSDR_DYNAMIC_BUFSIZE_ON", "CSDR_FIXED_BUFSIZE")}
    bank_env = dict(env, CSDR_AMD_BLOCK=str(per * inp))
    rows_at = [str(tmp_path / ("row%d" % k)) for k in range(3)]
    args = [CSDR, "fastddc_bank_cc", D, tbw, "HAMMING", "-"]
    for path, r in zip(rows_at, rates):
        args += [path, r]
    p = subprocess.run(["timeout", "-k", "5", "90"] + [str(a) for a in args], input=x.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=bank_env, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    rows = [np.fromfile(path, np.complex64) for path in rows_at]
    assert all(r.size == rows[0].size for r in rows) and rows[0].size >= 6 * B
    nb = rows[0].size // B
    P1 = [sm.power64(rows[1][k * B:(k + 1) * B]) for k in range(nb)]
    level = float(f32(math.sqrt(max(P1) * min(P1))))                     # between the loud and the quiet blocks; the block that holds the step is judged too
    assert min(P1) > 0 and max(P1) / min(P1) > 100 and wsm.undecidable_blocks(rows[1], B, 1, level) == []
    want_open = [pw >= level for pw in P1]
    assert want_open[0] and not want_open[-1]
    level_text = "%.9g" % level
    outs = [str(tmp_path / ("audio%d" % k)) for k in range(3)]
    ctl, smeter = str(tmp_path / "ctl"), str(tmp_path / "smeter")
    os.mkfifo(ctl)
    fc = os.open(ctl, os.O_RDWR | os.O_NONBLOCK)
    try:
        os.write(fc, ("1 squelch %s\n" % level_text).encode())
        args = [CSDR, "fastddc_wfm_bank_s16", "--squelch", B, 1, 1, smeter, D, tbw, "HAMMING", 5, 48000, "50e-6", ctl]
        for path, r in zip(outs, rates):
            args += [path, r]
        p = subprocess.run(["timeout", "-k", "5", "90"] + [str(a) for a in args], input=x.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=bank_env, timeout=120)
    finally:
        os.close(fc)
    assert p.returncode == 0, p.stderr.decode()
    assert "channel 1 squelch level is" in p.stderr.decode()
    lines = [ln.split() for ln in open(smeter).read().splitlines()]
    assert lines and all(len(ln) == 2 for ln in lines)
    pipe_env = dict(env, CSDR_AMD_BLOCK="4096")
    for k in range(3):
        audio, reports = single_stream_pipeline(tmp_path, str(k), rows[k], level_text if k == 1 else "0", pipe_env)
        got = open(outs[k], "rb").read()
        assert len(audio) == 2 * wm.plan(5, 12, 0, wm.W, 5.0, 0, nb * B)[0] > 2000 and got == audio, k
        mine = [ln[1] for ln in lines if ln[0] == str(k)]
        assert mine == reports.split() and len(mine) == len(sm.report_replay(1, nb)) >= 2, k
    a1 = np.frombuffer(open(outs[1], "rb").read(), np.int16)
    a0 = np.frombuffer(open(outs[0], "rb").read(), np.int16)
    assert np.abs(a1).max() > 1000 and not a1[-64:].any() and a0[-64:].any()      # channel 1 closed behind the step, channel 0 did not


def test_wfmrx_squelch_cli_single_stream(ctx, tmp_path):
    """`csdr wfm_rx_cc_s16 5 48000 --squelch --fifo <ctl> --outfifo <path> 1 1` with the level waiting in the fifo against `csdr squelch_and_smeter_cc --fifo
    <ctl> --outfifo <path> 1 1 | csdr wfm_rx_cc_s16 5` of the same binary: the same audio bytes and the same report lines; and against the Python object.  The
    --squelch group follows a prefix of the optional arguments here and the rate alone in a third run."""
    import csdr_amd
    assert os.path.exists(CSDR), "csdr_amd/csdr not built (make -C csdr_amd/csrc)"
    x = case_input(1)[0]
    env = {k: v for k, v in os.environ.items() if k not in ("CSDR_DYNAMIC_BUFSIZE_ON", "CSDR_FIXED_BUFSIZE")}
    env["CSDR_AMD_BLOCK"] = "4096"
    ctl, rep = str(tmp_path / "ctl"), str(tmp_path / "rep")
    os.mkfifo(ctl); os.mkfifo(rep)
    fc, fr = os.open(ctl, os.O_RDWR), os.open(rep, os.O_RDONLY | os.O_NONBLOCK)

    def reports():
        data = b""
        try:
            while True:
                b = os.read(fr, 65536)
                if not b:
                    break
                data += b
        except BlockingIOError:
            pass
        return data.decode()

    sq = "--fifo %s --outfifo %s 1 1" % (ctl, rep)
    got = []
    try:
        for line in ("%s wfm_rx_cc_s16 5 48000 --squelch %s" % (CSDR, sq), "%s squelch_and_smeter_cc %s | %s wfm_rx_cc_s16 5" % (CSDR, sq, CSDR),
                     "%s wfm_rx_cc_s16 5 --squelch %s" % (CSDR, sq)):
            os.write(fc, ("%g\n" % wsm.LEVEL).encode())
            p = subprocess.run(["timeout", "-k", "5", "90", "sh", "-c", line], input=x.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
            assert p.returncode == 0, p.stderr.decode()
            got.append((p.stdout, reports()))
    finally:
        os.close(fc); os.close(fr)
    assert got[0] == got[1] == got[2]
    with csdr_amd.WfmRx(ctx, 1, max_samples_per_call=x.size, squelch_block=1024, levels=wsm.LEVEL) as o:
        s16, count, pw, fl = o.process_squelched(x)
    assert count == n_out_of(1024) and 0 < fl.sum() < fl.size and got[0][0] == s16[0].tobytes()
    assert got[0][1] == "".join("%g\n" % pw[0, k] for k in sm.report_replay(1, pw.shape[1])) and len(got[0][1].split()) == 2
    p = subprocess.run(["timeout", "-k", "5", "90", CSDR, "wfm_rx_cc_s16", "5", "--squelch"], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode != 0 and "need required parameter (--fifo <fifo>)" in p.stderr.decode()
