"""The frame synchroniser on the GPU: both kernels against the CPU walk (the definition's step function, equal to the Python model by test_framesync_cpu) to
the byte -- payload, counts, positions and final state -- over shapes, channel counts, per-channel lengths, rows on odd byte offsets and every channels-per-wave
setting; the tiled kernel's tile edges; cut invariance; alternating kernels; reset_channel and a short pitch; the command through a pipe and inside `csdr
chain`; the loop back through the transmit and receive objects."""
import os
import subprocess

import numpy as np
import pytest

import framesync_model as fm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
TILED, GENERIC = "k_framesync_tiled", "k_framesync_generic"
SHAPES = [(1, 0, 0), (1, 5, 0), (2, 1, 0), (5, 7, 1), (16, 64, 0), (33, 300, 3), (1024, 8, 0)]
CHANNELS = [1, 3, 17, 70]
# channels per wave that the object accepts: k_framesync_generic 1 .. 64 (0: automatic); k_framesync_tiled always runs one channel per wave
LANES = {False: [0], True: [0, 1, 7, 64]}


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def walked(pat, V, m, x, count=None):
    import csdr_amd
    st, w = csdr_amd.FrameSyncChan(), np.zeros(len(pat), np.uint8)
    out, pos = csdr_amd.framesync_debug_walk(pat, V, x[:x.size if count is None else count], m, (), st, w)
    return out, pos, st.astuple()


def batch(rng, L, V, n_ch, n, alphabet=2):
    """one pattern, n_ch rows of n bytes with it planted at random gaps, and per-channel lengths that differ, a 0 among them"""
    pat = rng.integers(0, alphabet, L).astype(np.uint8)
    x = rng.integers(0, alphabet, (n_ch, n)).astype(np.uint8)
    for c in range(n_ch):
        at = int(rng.integers(0, 2 * L + 3))
        while at + L <= n:
            x[c, at:at + L] = pat
            if L > 8 and rng.integers(0, 3) == 0:
                x[c, at + int(rng.integers(0, L))] ^= 1                 # a damaged pattern: found only with an allowance
            at += L + int(rng.integers(0, 3 * (L + V) + 2))
    counts = np.array([n - (c * 37) % min(500, n) for c in range(n_ch)])
    if n_ch > 1:
        counts[1] = 0
    return pat, x, counts


def check(o, pat, V, m, x, counts, got, kernel):
    assert o.kernel_name() == kernel
    for c in range(x.shape[0]):
        out, pos, st = walked(pat, V, m, x[c], int(counts[c]))
        assert np.array_equal(got[c][0], out), (c, "payload")
        assert np.array_equal(got[c][1], pos), (c, "positions")
        assert o.get_channel(c)[0].astuple() == st, (c, "state")


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_walk(ctx, shape, forced):
    L, V, m = shape
    rng = np.random.default_rng(100 + L)
    n = 3000 if L < 1024 else 5000
    frames = 0
    for n_ch in CHANNELS:
        pat, x, counts = batch(rng, L, V, n_ch, n)
        with ctx.frame_sync(pat, V, n_ch, m) as o:
            o.force_generic(forced)
            for lanes in LANES[forced]:
                o.reset()
                o.set_lanes(lanes)
                got = o.process(x, counts, True, pitch=n + 13)          # rows 13 bytes past a multiple of 16 apart: odd byte offsets
                check(o, pat, V, m, x, counts, got, GENERIC if forced else TILED)
            frames += sum(len(g[1]) for g in got)
    assert frames > 4


def tile_rows(TILE, pat, V, ends, n):
    """rows of zeros (the pattern begins with 1) with a pattern ending at each index of `ends`"""
    x = np.zeros((len(ends), n), np.uint8)
    for c, es in enumerate(ends):
        for e in es:
            x[c, e - len(pat) + 1:e + 1] = pat
    return x


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("pitch_extra", [0, 5])
def test_tile_edges(ctx, forced, pitch_extra):
    import csdr_amd
    TILE = csdr_amd.framesync_tile()
    pat, L, V = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1], np.uint8), 9, 7
    n = 3 * TILE + 100
    # a pattern ending at TILE-1, at TILE and at TILE+L-2 (it straddles the tile edge by every amount between); a match whose payload ends at TILE-3, so that
    # the restarted searcher's dropped byte (L bytes on) lies in the next tile, with a pattern right behind that payload and one further on; with a misaligned
    # row (pitch_extra) the same indexes fall elsewhere in the tiles, so the rows repeat them shifted by the row's offset
    base = [[TILE - 1], [TILE], [TILE + L - 2], [TILE - 3 - V, TILE - 3 + L + 1, TILE + 60], [TILE - 3 - V, TILE - 2 + L - 1, TILE + 60],
            [2 * TILE - 1, 2 * TILE + L + V + 20]]
    ends = base + [[e + s for e in es] for s in (5, 10) for es in base]
    x = tile_rows(TILE, pat, V, ends, n)
    counts = np.full(len(ends), n)
    with ctx.frame_sync(pat, V, len(ends)) as o:
        o.force_generic(forced)
        got = o.process(x, counts, True, pitch=n + pitch_extra + (16 - n % 16) % 16)
        check(o, pat, V, 0, x, counts, got, GENERIC if forced else TILED)
        assert all(len(g[1]) >= 1 for g in got)


@pytest.mark.parametrize("forced", [False, True])
def test_long_payload_and_match_at_a_calls_last_byte(ctx, forced):
    import csdr_amd
    TILE = csdr_amd.framesync_tile()
    pat, V = np.array([1, 1, 0, 1], np.uint8), 2 * TILE + 3
    rng = np.random.default_rng(8)
    n = 3 * TILE + 500
    x = np.zeros((2, n), np.uint8)
    for c, e in enumerate((40, TILE - 1)):
        x[c, e - 3:e + 1] = pat
        x[c, e + 1:e + 1 + V] = rng.integers(0, 256, V)
        x[c, e + V + 30:e + V + 34] = pat                                # the next frame; its payload is cut by the end of the input
    with ctx.frame_sync(pat, V, 2) as o:
        o.force_generic(forced)
        one = o.process(x, None, True)
        check(o, pat, V, 0, x, [n, n], one, GENERIC if forced else TILED)
        assert [len(g[1]) for g in one] == [2, 2] and one[0][0].size > V
        o.reset()
        cut = o.process(x, None, True, calls=[41, 1, n - 42])           # channel 0's match is the first call's last byte: its payload arrives in the next calls
        for a, b in zip(one, cut):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def cut_calls(L, V, n, p):
    sets = [[0, 1, 0, 1], [L - 1, 1, 1], [L, 1, L, 1], [L + 1], [2 * L, 1], [2 * L + 1, 0, 1], [1] * (3 * L + 4), [p + V // 2, 1], [p + V - 1, 1], [p + V]]
    return [s + [n - sum(s)] for s in sets if sum(s) <= n]


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("shape", [(5, 7, 0), (16, 64, 1)])
def test_cut_invariance(ctx, shape, forced):
    L, V, m = shape
    rng = np.random.default_rng(31 + L)
    pat, x, _ = batch(rng, L, V, 3, 700)
    with ctx.frame_sync(pat, V, 3, m) as o:
        o.force_generic(forced)
        one = o.process(x, None, True)
        check(o, pat, V, m, x, [700] * 3, one, GENERIC if forced else TILED)
        p = int(one[0][1][0])
        for calls in cut_calls(L, V, 700, p):
            o.reset()
            got = o.process(x, None, True, calls=calls)
            check(o, pat, V, m, x, [700] * 3, got, GENERIC if forced else TILED)


def test_calls_may_alternate_between_the_kernels(ctx):
    """the tiled kernel turns its stream of stored bytes back into the ring at a call's end, and takes the ring up at the next call's start"""
    rng = np.random.default_rng(77)
    for L, V in ((5, 7), (16, 3), (33, 40)):
        pat, x, _ = batch(rng, L, V, 4, 900)
        want = [walked(pat, V, 0, x[c]) for c in range(4)]
        with ctx.frame_sync(pat, V, 4) as o:
            parts, at = [[[], []] for _ in range(4)], 0
            for k, cnt in enumerate([L - 2, 3, L, 1, 2 * L, 57, 1, 200, 900]):
                cnt = min(cnt, 900 - at)
                o.force_generic(k % 2 == 1)
                got = o.process(x[:, at:at + cnt], None, True)
                for c in range(4):
                    parts[c][0].append(got[c][0]); parts[c][1].append(got[c][1])
                at += cnt
            for c in range(4):
                assert np.array_equal(np.concatenate(parts[c][0]), want[c][0]) and np.array_equal(np.concatenate(parts[c][1]), want[c][1]), (L, c)
                assert o.get_channel(c)[0].astuple() == want[c][2]


@pytest.mark.parametrize("forced", [False, True])
def test_reset_channel_state_and_a_short_pitch(ctx, forced):
    import csdr_amd
    pat, V = np.array([1, 0, 1, 1], np.uint8), 50
    x = np.zeros((3, 400), np.uint8)
    x[:, 20:24] = pat
    x[:, 24:74] = np.arange(50) + 1
    x[:, 200:204] = pat
    x[:, 204:254] = np.arange(50) + 101
    with ctx.frame_sync(pat, V, 3) as o:
        o.force_generic(forced)
        a = o.process(x[:, :50])                                        # the call ends inside the first payload
        assert all(np.array_equal(r, x[0, 24:50]) for r in a) and o.get_channel(1)[0].remain == V - 26
        o.reset_channel(1)
        st, w = o.get_channel(0)
        b = o.process(x[:, 50:], None, True)
        assert np.array_equal(b[0][0], np.r_[x[0, 50:74], x[0, 204:254]]) and b[0][1].tolist() == [204]
        assert np.array_equal(b[1][0], x[1, 204:254]) and b[1][1].tolist() == [204 - 50]      # channel 1 started over at the call's first byte
        assert np.array_equal(b[2][0], b[0][0])
        # a record and its ring move to another channel: the second half of a stream continues there
        o.reset()
        o.process(x[:, :210])
        st, w = o.get_channel(0)
        o.reset_channel(2)
        o.set_channel(2, st, w)
        c = o.process(x[:, 210:], None, True)
        assert np.array_equal(c[2][0], c[0][0]) and c[0][0].size == 44 and o.get_channel(2)[0].astuple() == o.get_channel(0)[0].astuple()
        bad = csdr_amd.FrameSyncChan(fill=2, index=1)
        with pytest.raises(csdr_amd.CsdrAmdError):
            o.set_channel(0, bad)
        # a short out_pitch or frame_pitch is an error that consumes nothing
        o.reset()
        d_in, d_out, d_cnt, d_pos = ctx.upload(x), ctx.alloc(3 * 400), ctx.alloc(256), ctx.alloc(8 * 3 * 400)
        before = o.get_channel(0)[0].astuple()
        with pytest.raises(csdr_amd.CsdrAmdError, match="out_pitch"):
            o.process_dev(d_in.ptr, 400, 400, d_out.ptr, 399, d_cnt.ptr)
        with pytest.raises(csdr_amd.CsdrAmdError, match="frame_pitch"):
            o.process_dev(d_in.ptr, 400, 400, d_out.ptr, 400, d_cnt.ptr, None, d_pos.ptr, o.max_frames(400) - 1)
        assert o.get_channel(0)[0].astuple() == before == (0, 0, 0, 0, 0)
        assert o.max_out(400) == 400 and o.max_frames(400) == 400 // 5 + 1
        full = o.process(x, None, True)
        assert np.array_equal(full[0][0], np.r_[x[0, 24:74], x[0, 204:254]]) and full[0][1].tolist() == [24, 204]


def test_create_errors(ctx):
    import csdr_amd
    for pat, V, m in (([], 1, 0), ([0] * 1025, 1, 0), ([1, 2], -1, 0), ([1, 2], (1 << 30) + 1, 0), ([1, 2], 1, 2), ([1, 256], 1, 0)):
        with pytest.raises(csdr_amd.CsdrAmdError):
            ctx.frame_sync(pat, V, 1, m)
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.frame_sync([1, 2], 1, 0)


def test_stateless_call(ctx):
    rng = np.random.default_rng(3)
    pat, x, _ = batch(rng, 6, 9, 1, 2000)
    assert np.array_equal(ctx.pattern_search(x[0], pat, 9), walked(pat, 9, 0, x[0])[0])


def _run(argv, data, block=None):
    env = dict(os.environ)
    if block:
        env["CSDR_AMD_BLOCK"] = str(block)
    p = subprocess.run(argv, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


def test_cli_command_through_a_pipe(ctx):
    rng = np.random.default_rng(12)
    pat, x, _ = batch(rng, 16, 64, 1, 40000)
    args = [str(int(v)) for v in pat]
    for block in (None, 4096):                                           # one pass, and several with the searcher's state carried between them
        rc, out, err = _run([CSDR, "pattern_search_u8_u8", "64"] + args, x[0].tobytes(), block)
        assert rc == 0 and "one device frame synchroniser" in err
        want = walked(pat, 64, 0, x[0])[0]
        assert out == want.tobytes() and want.size > 64 * 20           # a payload cut by the end of the input is written as far as it arrived, nothing behind it
    rc, out, err = _run([CSDR, "pattern_search_u8_u8", "--mismatch", "1", "64"] + args, x[0].tobytes())
    want1 = walked(pat, 64, 1, x[0])[0]
    assert rc == 0 and out == want1.tobytes() and want1.size > want.size
    rc, out, err = _run([CSDR, "pattern_search_u8_u8", "4", "1", "300"], x[0].tobytes())
    assert rc != 0 and out == b"" and "above 255" in err
    rc, out, err = _run([CSDR, "pattern_search_u8_u8", "4"], b"")
    assert rc != 0 and "need required parameter (pattern_values" in err


def test_cli_chain_keeps_the_stage_on_the_device(ctx):
    """generic_slicer_f_u8 in front of it inside `csdr chain`: one process, the sliced bytes never leave the device; the stage says what it is"""
    rng = np.random.default_rng(13)
    pat, x, _ = batch(rng, 13, 32, 1, 20000)
    soft = ((2.0 * x[0] - 1.0) * rng.uniform(0.2, 1.5, x[0].size)).astype(np.float32)
    rc, out, err = _run([CSDR, "chain", "generic_slicer_f_u8 2 | pattern_search_u8_u8 32 " + " ".join(str(int(v)) for v in pat)], soft.tobytes(), 8192)
    assert rc == 0 and "csdr pattern_search_u8_u8: one device frame synchroniser (13 pattern values, 32 after, 0 may differ)" in err
    want = walked(pat, 32, 0, x[0])[0]
    assert out == want.tobytes() and want.size > 32 * 20


BARKER13 = np.array([1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1], np.uint8)


@pytest.mark.parametrize("forced", [False, True])
def test_loopback_through_the_transmit_and_receive_objects(ctx, forced):
    """PulseTx (BPSK, 8 samples per symbol, RRC 65) -> delays of 3, 4, 5 samples -> PulseRx to sliced bits -> FrameSync.  The geometry is
    test_loopback_through_the_transmit_object's: symbol m peaks at sample 8 m - 64 behind both filters, so the receiver's index j belongs to symbol
    round((j + 64) / 8) and the symbols 8 .. n - 9 are in reach.  BPSK symbol v is cos(pi v): bit 0 -> +1 -> slice 1, so the receive side sees the bits
    inverted and searches the inverted word.  Filler of 60 .. 90 bits between the frames is longer than the 2 L + 1 bytes a restart can affect."""
    import csdr_amd
    I, T, L, V = 8, 65, 13, 64
    taps = csdr_amd.firdes_rrc_f(T, I, 0.35)
    rng = np.random.default_rng(41)
    bits, starts = [], []
    for ch in range(3):
        row, st = [], []
        for _ in range(3):
            row.append(rng.integers(0, 2, int(rng.integers(60, 91))).astype(np.uint8))
            st.append(sum(r.size for r in row) + L)                      # the payload's first symbol
            row += [BARKER13, rng.integers(0, 2, V).astype(np.uint8)]
        row.append(rng.integers(0, 2, 700 - sum(r.size for r in row)).astype(np.uint8))
        bits.append(np.concatenate(row)); starts.append(st)
    bits = np.stack(bits)
    n = bits.shape[1]
    word = 1 - BARKER13
    for ch in range(3):                                                  # the streams hold the word nowhere else
        assert fm.search(word, V, 1 - bits[ch])[1].tolist() == starts[ch]
    with ctx.pulse_tx(3, 2, I, taps) as tx:
        y = tx.process(bits)
    scale, delays = 8.0, (3, 4, 5)
    x = np.zeros((3, y.shape[1] + 8), np.complex64)
    for ch, d in enumerate(delays):
        x[ch, d:d + y.shape[1]] = scale * y[ch]
    peak = float(np.sum(taps.astype(np.float64) ** 2))
    p = csdr_amd.pulserx_params(taps, "GARDNER", I, 0.5, 2.0, True, 1.0 / (scale * peak), 2, False)
    with ctx.pulse_rx(p, 3, "filter", "timing") as o:
        timing = o.process(x, with_extras=True)
    with ctx.pulse_rx(p, 3, "filter", "slice") as o:
        sliced = o.process(x)
    counts = np.array([s.size for s in sliced])
    rows = np.zeros((3, counts.max()), np.uint8)
    for ch in range(3):
        rows[ch, :counts[ch]] = sliced[ch]
    with ctx.frame_sync(word, V, 3) as fs:
        fs.force_generic(forced)
        got = fs.process(rows, counts, True)
    for ch, d in enumerate(delays):
        m = np.rint((timing[ch][2].astype(np.int64) - d + 64) / I).astype(np.int64)     # the transmitted symbol behind each received bit
        assert m.size == counts[ch]
        payload, pos = got[ch]
        assert all(8 <= s and s + V <= n - 8 for s in starts[ch])       # every frame is in reach
        assert m[pos].tolist() == starts[ch], ch
        assert np.array_equal(payload, np.concatenate([1 - bits[ch, s:s + V] for s in starts[ch]])), ch
