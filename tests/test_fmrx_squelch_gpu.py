"""The squelched FM receive bank on the GPU (csdr_amd_fmrx_create_squelched / csdr_amd.FmRx(squelch_block=...)): the fused path, the generic path and the
composition csdr_amd.Squelch -> csdr_amd.FmRx in every bit, under every cut of the stream into calls; all of them against the oracle's chain on the model's
gated stream; the levels, the resets, the refusals and the two commands.  The shapes are the smallest at which a path can still go wrong: one channel, a
partly filled 16-row group, two groups plus one channel; 7 AGC blocks; squelch blocks of 1024 (the span) and of 300 (blocks that straddle spans, staging passes
and calls), and 301 (an odd block: quads of four staged samples that straddle two blocks, held counts of either parity)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fmrx_model as fm
import fmrx_squelch_model as fsm
import squelch_model as sm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
FUSED, GENERIC = "k_fmrx_front_sq", "k_nfm_deemph_mfma"
RATE = 48000
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    assert c.arch().startswith("gfx950")
    yield c
    c.close()


_inputs = {}


def case_input(n_ch, seed=0, n=fsm.N):
    key = (n_ch, seed, n)
    if key not in _inputs:
        x = fsm.make_input(n_ch, n, seed)
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]


def cut(n, calls):
    calls = [n] if calls is None else list(calls)
    if sum(calls) < n:
        calls.append(n - sum(calls))
    return calls


def run(ctx, x, B, d, lv, calls=None, generic=False, kernel=None, obj=None, block=1024, levels_between=None, **kw):
    """x [n_channels, n] through one squelched object in calls of `calls` samples (the rest in one more); generic: a path for all calls, or one per call;
    levels_between: {call index: [(channel, level), ...]} applied in front of that call -> (s16, float audio, per-call audio counts, powers, flags).
    Every call's counts are checked against the two plans and max_output, its kernel_name against `kernel` (default: the path asked for)."""
    import csdr_amd
    x = np.atleast_2d(x)
    calls = cut(x.shape[1], calls)
    o = obj or csdr_amd.FmRx(ctx, x.shape[0], audio_rate=RATE, agc_block=block, max_samples_per_call=max(max(calls), 1), squelch_block=B, use_every_nth=d, levels=lv)
    try:
        pcm, af, counts, pws, fls, at = [], [], [], [], [], 0
        for i, k in enumerate(calls):
            g = generic[i % len(generic)] if isinstance(generic, (list, tuple)) else generic
            o.force_generic(g)
            for ch, level in (levels_between or {}).get(i, ()):
                o.set_squelch_level(ch, level)
            assert csdr_amd.fmrx_squelch_plan(o.squelch_held(), k, B) == fsm.squelch_plan(o.squelch_held(), k, B)
            want = fsm.plan(o.fill(), o.squelch_held(), k, o.taps_length, block, B)
            blocks_before = o.squelch_block_index()
            s16, f, got, pw, fl = o.process_squelched(x[:, at:at + k], with_float=True, **kw)
            assert (got, o.fill(), o.squelch_held(), pw.shape[1]) == want and fl.shape == pw.shape and got <= o.max_output(k)
            assert o.squelch_block_index() == blocks_before + want[3]
            if k:
                assert o.kernel_name() == (kernel or (GENERIC if g else FUSED))
            pcm.append(s16); af.append(f); counts.append(got); pws.append(pw); fls.append(fl); at += k
        return np.concatenate(pcm, axis=1), np.concatenate(af, axis=1), counts, np.concatenate(pws, axis=1), np.concatenate(fls, axis=1)
    finally:
        if obj is None:
            o.close()


def composed(ctx, x, B, d, lv, calls=None, levels_between=None, block=1024):
    """csdr_amd.Squelch into a second row buffer, csdr_amd.FmRx over it, call by call -> run()'s tuple"""
    import csdr_amd
    x = np.atleast_2d(x)
    s = x.shape[0]
    calls = cut(x.shape[1], calls)
    pcm, af, counts, pws, fls, at = [], [], [], [], [], 0
    with csdr_amd.Squelch(ctx, s, B, d, lv, max_samples_per_call=max(max(calls), 1)) as sq, \
            csdr_amd.FmRx(ctx, s, audio_rate=RATE, agc_block=block, max_samples_per_call=max(calls) + B) as rx:
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


def ragged(B):
    """341, then three spans + 5, then the rest"""
    return [341, 3 * 1024 + 5]


def short_calls(B):
    """calls of a third of a block: two in three complete no block"""
    return [B // 3] * 7


# ---------------------------------------------------------------- 1. fused = generic = composed, in every bit
@pytest.mark.parametrize("n_ch,B,d", fsm.SHAPES + [(17, 301, 1)])
def test_fmrx_squelch_paths_and_composition_same_bits(ctx, n_ch, B, d):
    x, lv = case_input(n_ch), fsm.levels(n_ch)
    for calls in (None, ragged(B), short_calls(B)):
        a, b, c = run(ctx, x, B, d, lv, calls), run(ctx, x, B, d, lv, calls, generic=True), composed(ctx, x, B, d, lv, calls)
        assert sum(a[2]) == 7 * 1024 and a[3].shape == (n_ch, fsm.N // B), calls
        assert same_bits(a, b) and same_bits(a, c), calls
        if calls is not None and calls[0] < B:
            assert a[2][0] == 0 and a[3].shape[1] > 0
    if n_ch > 2:
        assert a[4][1].all() and not a[4][2].any() and 0 < a[4][0].sum() < a[4][0].size


def test_fmrx_squelch_closed_block_follows_an_open_one_inside_a_quad(ctx):
    """B = 301: block boundaries at every residue mod 4 of the staged row, so quads of four staged samples hold the end of an open block and the start of a
    closed one (and the reverse); B = 300: the boundary falls between two quads and only the demodulator's previous sample comes from the other block"""
    x, lv = case_input(17), fsm.levels(17)
    for B in (300, 301):
        a = run(ctx, x, B, 1, lv)
        assert same_bits(a, composed(ctx, x, B, 1, lv))
        fl = a[4][0].astype(int)
        falls = [k for k in range(1, fl.size) if fl[k - 1] == 1 and fl[k] == 0]
        rises = [k for k in range(1, fl.size) if fl[k - 1] == 0 and fl[k] == 1]
        assert falls and rises
        if B == 301:
            assert {(k * B) % 4 for k in falls + rises} - {0}


# ---------------------------------------------------------------- 2. against the oracle
@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
@pytest.mark.parametrize("n_ch,B,d", [(1, 1024, 1), (17, 300, 3), (33, 1024, 3), (17, 300, 1)])
def test_fmrx_squelch_against_oracle(ctx, port, n_ch, B, d, generic):
    x, lv, taps = case_input(n_ch), fsm.levels(n_ch), fm.taps_of(RATE)
    pcm, af, counts, pw, fl = run(ctx, x, B, d, lv, generic=generic)
    assert counts == [7 * 1024]
    for c in range(n_ch):
        want_s16, want_af, want_pw, want_fl = fsm.expected(port, x[c], B, d, lv[c], taps)
        assert np.array_equal(fl[c], want_fl), c
        for k in range(want_pw.size):
            P = sm.power64(x[c, k * B:(k + 1) * B], d)
            assert abs(float(pw[c, k]) - P) <= sm.bound(B, d, P), (c, k)
        if not want_fl.any():                                           # every block closed: silence, exactly
            assert not want_s16.any() and not pcm[c].any() and not af[c].any() and af[c].size == 7 * 1024
        else:
            fm.assert_gates(pcm[c], af[c], want_s16, want_af, what="%s ch %d (%s) B %d d %d" % ("generic" if generic else "fused", c, fm.KINDS[c % 4], B, d))


# ---------------------------------------------------------------- 3. level 0 everywhere: the unsquelched bank on the first m samples
@pytest.mark.parametrize("B", [1024, 300])
def test_fmrx_squelch_level_zero_equals_unsquelched(ctx, B):
    import csdr_amd
    x = case_input(17)
    m = fsm.N // B * B
    with csdr_amd.FmRx(ctx, 17, max_samples_per_call=m) as o:
        want = o.process(x[:, :m], with_float=True)
        assert o.kernel_name() == "k_fmrx_front"
    for generic in (False, True):
        got = run(ctx, x, B, 1, None, ragged(B), generic=generic)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and sum(got[2]) == want[2]
        assert got[4].all()


# ---------------------------------------------------------------- 4. set_squelch_level between calls
@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
def test_fmrx_squelch_level_changes_between_calls(ctx, generic):
    """B = 1024.  In front of call 1, with 500 samples of block 0 held, channel 0 goes to ALL_CLOSED and channel 2 (all closed so far) to 0: block 0 stays under
    the levels it started with, block 1 and later have the new ones.  In front of call 3, with nothing held (2048 samples in), channel 0 returns to LEVEL:
    block 2 has it.  The model's `changes` say the same: {0: new} is read behind block 0, {1: new} behind block 1."""
    import csdr_amd
    B, x, lv = 1024, case_input(17), fsm.levels(17)
    calls = [500, 1000, 548, 2000]
    between = {1: [(0, fsm.ALL_CLOSED), (2, 0.0)], 3: [(0, fsm.LEVEL)]}
    got = run(ctx, x, B, 1, lv, calls, generic=generic, levels_between=between)
    assert same_bits(got, composed(ctx, x, B, 1, lv, calls, levels_between=between))
    want0 = fsm.gated(x[0], B, 1, fsm.LEVEL, {0: fsm.ALL_CLOSED, 1: fsm.LEVEL})[2]
    want2 = fsm.gated(x[2], B, 1, fsm.ALL_CLOSED, {0: 0.0})[2]
    assert np.array_equal(got[4][0], want0) and np.array_equal(got[4][2], want2)
    assert want0[0] == 1 and want0[1] == 0 and list(want2[:3]) == [0, 1, 1]
    with csdr_amd.FmRx(ctx, 3, squelch_block=B, levels=[0.5, 0.25, 0.125]) as o:
        assert [o.get_squelch_level(c) for c in range(3)] == [0.5, 0.25, 0.125]
        o.set_squelch_level(-1, 2.0)
        assert [o.get_squelch_level(c) for c in range(3)] == [2.0, 2.0, 2.0]
        o.set_squelch_level(1, 0.0)
        assert [o.get_squelch_level(c) for c in range(3)] == [2.0, 0.0, 2.0]
        for bad in (3, -2):
            with pytest.raises(csdr_amd.CsdrAmdError, match="fmrx: channel out of range"):
                o.set_squelch_level(bad, 1.0)


# ---------------------------------------------------------------- 5. paths alternating call by call
@pytest.mark.parametrize("B,d", [(300, 1), (1024, 3), (301, 1)])
def test_fmrx_squelch_paths_alternate_within_a_stream(ctx, B, d):
    """the held squelch samples and the held filter input move between the two paths' buffers"""
    x, lv = case_input(17), fsm.levels(17)
    calls = [341, 100, 1500, 900, 150, 2100, 64]
    ref = run(ctx, x, B, d, lv, calls, generic=True)
    for order in ([False, True], [True, False]):
        assert same_bits(run(ctx, x, B, d, lv, calls, generic=order), ref), order


# ---------------------------------------------------------------- 6. reset_channel, reset
@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
def test_fmrx_squelch_reset_channel_and_reset(ctx, generic):
    """B = 64, first call 33 blocks + 48: two AGC blocks out, then the filter holds 1024 + 64 samples and the squelch 48.  reset_channel(1) leaves channel 1
    with zeros in all of them and no history, 48 samples into a squelch block: so is a fresh channel fed 64 + 48 zero samples, which write nothing.  (A zero
    block is silence open or closed; the block under way, 48 zeros and 16 samples, is judged in both.)"""
    import csdr_amd
    B, first = 64, 33 * 64 + 48
    x, lv = case_input(3, seed=3), fsm.levels(3)
    undisturbed = run(ctx, x, B, 1, lv, [first], generic=generic)
    with csdr_amd.FmRx(ctx, 3, max_samples_per_call=x.shape[1], squelch_block=B, levels=lv) as o:
        a = run(ctx, x[:, :first], B, 1, lv, obj=o, generic=generic)
        assert a[2] == [2 * 1024] and o.fill() == fm.PREFIX + 64 and o.squelch_held() == 48 and o.squelch_block_index() == 33
        o.reset_channel(1)
        assert o.fill() == fm.PREFIX + 64 and o.squelch_held() == 48 and o.squelch_block_index() == 33
        b = run(ctx, x[:, first:], B, 1, lv, obj=o, generic=generic)
        fresh = run(ctx, np.concatenate([np.zeros((1, 64 + 48), np.complex64), x[1:2, first:]], axis=1), B, 1, lv[1:2], [64 + 48], generic=generic)
        assert fresh[2] == [0] + b[2]
        assert np.array_equal(b[0][1], fresh[0][0]) and np.array_equal(b[1][1].view(np.uint32), fresh[1][0].view(np.uint32))
        assert np.array_equal(b[3][1].view(np.uint32), fresh[3][0][1:].view(np.uint32)) and np.array_equal(b[4][1], fresh[4][0][1:])
        for c in (0, 2):
            for j in (0, 1, 3, 4):
                assert np.array_equal(np.concatenate([a[j][c], b[j][c]]), undisturbed[j][c]), (c, j)
        o.reset()
        assert o.fill() == fm.PREFIX and o.squelch_held() == 0 and o.squelch_block_index() == 0 and o.get_squelch_level(2) == fsm.ALL_CLOSED
        assert same_bits(run(ctx, x, B, 1, lv, [first], obj=o, generic=generic), undisturbed)


# ---------------------------------------------------------------- 7. shapes that leave the fused path
def test_fmrx_squelch_shapes_that_leave_the_fused_kernel(ctx):
    B, x, lv = 300, case_input(17), fsm.levels(17)
    n = x.shape[1]
    ref = run(ctx, x, B, 1, lv, ragged(B), generic=True)
    odd, even = n | 1, (n + 3) & ~1
    assert same_bits(run(ctx, x, B, 1, lv, ragged(B), kernel=GENERIC, in_pitch=odd), ref)               # rows off 16-byte boundaries
    assert same_bits(run(ctx, x, B, 1, lv, ragged(B), kernel=GENERIC, in_offset=8), ref)                 # the base 8 bytes off
    assert same_bits(run(ctx, x, B, 1, lv, ragged(B), kernel=FUSED, in_pitch=even, in_offset=16), ref)  # (an even pitch on an aligned base stays)
    b512 = run(ctx, x, B, 1, lv, ragged(B), kernel=GENERIC, block=512)                                   # an AGC block that is not the span
    assert same_bits(b512, run(ctx, x, B, 1, lv, ragged(B), generic=True, block=512)) and sum(b512[2]) == 15 * 512
    assert same_bits(b512, composed(ctx, x, B, 1, lv, ragged(B), block=512))


def test_fmrx_squelch_plain_process_is_the_same_call(ctx):
    import csdr_amd
    B, x, lv = 300, case_input(17), fsm.levels(17)
    ref = run(ctx, x, B, 1, lv, ragged(B))
    for generic in (False, True):
        with csdr_amd.FmRx(ctx, 17, max_samples_per_call=x.shape[1], squelch_block=B, levels=lv) as o:
            o.force_generic(generic)
            parts, at = [], 0
            for k in cut(x.shape[1], ragged(B)):
                parts.append(o.process(x[:, at:at + k], with_float=True)); at += k
            assert o.kernel_name() == (GENERIC if generic else FUSED) and o.squelch_block_index() == fsm.N // B
            assert [p[2] for p in parts] == ref[2] and np.array_equal(np.concatenate([p[0] for p in parts], axis=1), ref[0])
            assert np.array_equal(np.concatenate([p[1] for p in parts], axis=1).view(np.uint32), ref[1].view(np.uint32))


# ---------------------------------------------------------------- 8. every CU busy
def test_fmrx_squelch_paths_same_bits_with_every_cu_busy(ctx):
    """512 channels x 24 spans, rows tiled from 16, as tests/test_fmrx_gpu.py::test_fmrx_paths_same_bits_with_every_cu_busy: 768 workgroups of the gated front
    kernel and 12288 of the power kernel"""
    n = fm.n_for_blocks(24, fm.taps_of(RATE).size)
    rows, lv16 = case_input(16, seed=5, n=n), fsm.levels(16)
    x, lv = np.tile(rows, (32, 1)), np.tile(lv16, 32)
    a, b = run(ctx, x, 1024, 1, lv), run(ctx, x, 1024, 1, lv, generic=True)
    assert a[2] == [23 * 1024] and a[3].shape == (512, n // 1024) and same_bits(a, b)
    assert np.array_equal(a[0][:16], a[0][496:]) and not np.array_equal(a[0][0], a[0][1]) and 0 < a[4][0].sum() < a[4][0].size


# ---------------------------------------------------------------- 9. the refusals
def test_fmrx_squelch_refusals(ctx):
    import csdr_amd
    L = ctx.L
    for B, d, msg in ((0, 1, "fmrx: squelch_block should be 1 .. 65536"), (65537, 1, "fmrx: squelch_block"), (-1, 1, "fmrx: squelch_block"), (1024, 0, "fmrx: use_every_nth"),
                      (1024, -3, "fmrx: use_every_nth")):
        assert L.csdr_amd_fmrx_create_squelched(ctx.h, 2, RATE, 1024, 1.0, 1.0, 4096, B, d, None) is None and msg in ctx.err()
    with pytest.raises(csdr_amd.CsdrAmdError, match="fmrx: use_every_nth"):
        csdr_amd.FmRx(ctx, 2, squelch_block=1024, use_every_nth=0)
    with pytest.raises(csdr_amd.CsdrAmdError, match="fmrx: squelch_block"):
        csdr_amd.FmRx(ctx, 2, squelch_block=1 << 17)
    x = fsm.make_input(2, 4096)
    di, ds, dp, dg = ctx.upload(x), ctx.alloc(2 * 2 * 4096 + 256), ctx.alloc(4 * 2 * 16), ctx.alloc(2 * 16)
    with ctx.fm_rx(2, max_samples_per_call=3000, squelch_block=300, levels=[fsm.LEVEL, 0.0]) as o:
        assert o.process_squelched_dev(di.ptr, 4096, 100, ds.ptr, None, 4096, dp.ptr, 0, dg.ptr) == (0, 0) and o.squelch_held() == 100     # (no block: no pitch needed)
        state = (o.fill(), o.squelch_held(), o.squelch_block_index())
        for power, flags in ((dp.ptr, None), (None, dg.ptr), (dp.ptr, dg.ptr)):
            assert L.csdr_amd_fmrx_process_squelched(o.h, di.at(800), 4096, 2900, ds.ptr, None, 4096, power, 9, flags, None) == -3
            assert "fmrx: power_pitch 9 below the 10 squelch blocks of this call" in ctx.err()
        assert L.csdr_amd_fmrx_process_squelched(o.h, di.at(800), 4096, 3001, ds.ptr, None, 4096, None, 0, None, None) == -3 and "fmrx: n_in should be 0 .. " in ctx.err()
        assert L.csdr_amd_fmrx_process_squelched(o.h, di.at(800), 4096, 2900, ds.ptr, None, 2047, None, 0, None, None) == -3 and "fmrx: out_pitch 2047 smaller" in ctx.err()
        assert (o.fill(), o.squelch_held(), o.squelch_block_index()) == state                                       # a refused call changes nothing
        assert o.process_squelched_dev(di.at(800), 4096, 2900, ds.ptr, None, 4096, dp.ptr, 10, dg.ptr) == (3072, 10) and o.squelch_held() == 0
        assert o.max_output(3000) == 3072 and o.max_output(0) == 0
    with ctx.fm_rx(2, max_samples_per_call=3000) as o:                   # an object without a squelch
        state = o.fill()
        assert L.csdr_amd_fmrx_process_squelched(o.h, di.ptr, 4096, 3000, ds.ptr, None, 4096, None, 0, None, None) == -3 and "created without a squelch" in ctx.err()
        assert L.csdr_amd_fmrx_set_squelch_level(o.h, 0, 1.0) == -3 and "created without a squelch" in ctx.err()
        assert L.csdr_amd_fmrx_squelch_held(o.h) == -3 and L.csdr_amd_fmrx_squelch_block_index(o.h) == -3
        for call in (lambda: o.process_squelched(x[:, :3000]), lambda: o.set_squelch_level(0, 1.0), lambda: o.get_squelch_level(0), o.squelch_held, o.squelch_block_index):
            with pytest.raises(csdr_amd.CsdrAmdError, match="created without a squelch"):
                call()
        assert o.fill() == state and o.process_dev(di.ptr, 4096, 3000, ds.ptr, None, 3072) == 3072


# ---------------------------------------------------------------- 10. the two commands
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


def test_fmrx_squelch_cli_bank_equals_python_composition(ctx, tmp_path):
    """`csdr fastddc_nfm_bank_s16 --squelch 300 1 1 <smeter>` on 3 channels at the smallest channelizer geometry against ctx.fastddc_bank -> the squelched FmRx
    with the same blocks per call (fmrx_squelch_model.bank_composition), which runs in a process of its own without torch (tests/test_fmrx_gpu.py's bank test
    says why).  Channel 0's audio goes to a fifo: once the first batch's bytes have arrived the command waits for input, and the level line written then is
    applied in front of the second batch, as it is in the composition, with 284 samples of a block held: that block stays open, the later ones of channel 1
    close.  The audio files byte for byte, the S-meter lines against report_replay over the composition's powers."""
    import math
    assert os.path.exists(CSDR), "csdr_amd/csrc not built (make -C csdr_amd/csrc)"
    D, tbw, rates, B, every = 2, 0.05, [-0.1, 0.2, -0.3], 300, 1
    ddc, _ = ctx.fastddc_init(tbw, D, 0.0)
    inp = ddc.input_size
    per = 1024 // math.gcd(inp, 1024)
    rng = np.random.default_rng(77)
    t = np.arange(2 * per * inp)
    x = sum(0.3 * fm.fm_baseband(rng, t.size, dev=5e3 / 96e3) * np.exp(-2j * np.pi * r * t) for r in rates).astype(np.complex64)
    env = {k: v for k, v in os.environ.items() if k != "CSDR_AMD_WORLD"}
    np.savez(str(tmp_path / "in.npz"), x=x, tbw=tbw, decimation=D, rates=rates, per=per, B=B, d=1, level_channel=1, level=fsm.ALL_CLOSED)
    c = subprocess.run(["timeout", "-k", "5", "120", sys.executable, os.path.join(ROOT, "tests", "fmrx_squelch_model.py"), str(tmp_path / "in.npz"), str(tmp_path / "want.npz")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, CSDR_AMD_NO_TORCH_PRELOAD="1"), timeout=150)
    assert c.returncode == 0, c.stderr.decode()
    w = np.load(str(tmp_path / "want.npz"))
    want = [w["first"], w["second"]]
    assert not w["torch_loaded"]
    assert want[0].shape[1] > 0 and want[1].shape[1] > 0 and want[0].shape[1] + want[1].shape[1] >= 6 * 1024
    outs = [str(tmp_path / ("audio%d" % k)) for k in range(3)]
    ctl, smeter = str(tmp_path / "ctl"), str(tmp_path / "smeter")
    os.mkfifo(outs[0]); os.mkfifo(ctl)
    fo, fc = os.open(outs[0], os.O_RDWR | os.O_NONBLOCK), os.open(ctl, os.O_RDWR | os.O_NONBLOCK)
    args = ["timeout", "-k", "5", "90", CSDR, "fastddc_nfm_bank_s16", "--squelch", B, 1, every, smeter, D, tbw, "HAMMING", 48000, ctl]
    for path, r in zip(outs, rates):
        args += [path, r]
    p = subprocess.Popen([str(a) for a in args], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, CSDR_AMD_BLOCK=str(per * inp)))
    try:
        p.stdin.write(x[:per * inp].tobytes()); p.stdin.flush()
        first = read_exactly(fo, 2 * want[0].shape[1])
        os.write(fc, ("1 squelch %g\n" % fsm.ALL_CLOSED).encode())
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
    powers = w["powers"]
    assert powers.shape[0] == 3 and powers.shape[1] >= 20 and open(smeter).read() == fsm.smeter_lines(powers, every)
    # the level line did something: channel 1 falls silent, the others are what they are without it
    plain = w["plain"]
    assert np.array_equal(plain[0], want_all[0]) and np.array_equal(plain[2], want_all[2]) and not np.array_equal(plain[1], want_all[1])
    assert plain[1][-256:].any() and not want_all[1][-256:].any()          # (fastagc_ff writes a block two blocks late)


def test_fmrx_squelch_cli_single_stream(ctx, tmp_path):
    """`csdr nfm_rx_cc_s16 --squelch --fifo <ctl> --outfifo <path> 1 1` with the level waiting in the fifo against `csdr squelch_and_smeter_cc --fifo <ctl>
    --outfifo <path> 1 1 | csdr nfm_rx_cc_s16` of the same binary: the same audio bytes and the same report lines; and against the Python object"""
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
        for line in ("%s nfm_rx_cc_s16 --squelch %s" % (CSDR, sq), "%s squelch_and_smeter_cc %s | %s nfm_rx_cc_s16" % (CSDR, sq, CSDR)):
            os.write(fc, ("%g\n" % fsm.LEVEL).encode())
            p = subprocess.run(["timeout", "-k", "5", "90", "sh", "-c", line], input=x.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
            assert p.returncode == 0, p.stderr.decode()
            got.append((p.stdout, reports()))
    finally:
        os.close(fc); os.close(fr)
    assert got[0] == got[1]
    with csdr_amd.FmRx(ctx, 1, max_samples_per_call=x.size, squelch_block=1024, levels=fsm.LEVEL) as o:
        s16, count, pw, fl = o.process_squelched(x)
    assert count == 7 * 1024 and 0 < fl.sum() < fl.size and got[0][0] == s16[0].tobytes()
    assert got[0][1] == "".join("%g\n" % pw[0, k] for k in sm.report_replay(1, pw.shape[1])) and len(got[0][1].split()) == 2
