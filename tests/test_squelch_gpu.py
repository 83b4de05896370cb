"""GPU checks of the squelch and S-meter (squelch.hip): the object against the CPU run of the same step function bit for bit (every kernel instance, the
generic kernel, pitches, call cuts, 1 / 3 / 257 channels), against the reference library outside the undecidable blocks, levels (per channel, changed
between calls, 0), Inf / NaN inputs, reset_channel, the stateless and drop-in calls, the CLI command against oracle/_ref/csdr through pipes and fifos, and
the command as a resident `csdr chain` stage."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import squelch_model as sm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_CSDR = os.path.join(ROOT, "oracle", "_ref", "csdr")
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
LEVEL = 1e-3


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _hook(x, B, d, levels):
    """the expected (out, power, flags) per channel from csdr_amd_debug_squelch_power"""
    import csdr_amd
    return [sm.stream(x[c], B, d, levels[c], power=lambda b, dd: csdr_amd.squelch_debug_power(b, dd)) for c in range(x.shape[0])]


def _same(got, want, what):
    """bit for bit, channel by channel: outputs, powers, flags"""
    for c, (wo, wp, wf) in enumerate(want):
        assert got[1][c].tobytes() == wp.tobytes(), (what, c, "power")
        assert np.array_equal(got[2][c], wf), (what, c, "flags")
        assert got[0][c].tobytes() == wo.tobytes(), (what, c, "out")


# B at both sides of each kernel boundary (one wave: <= 512, <= 2048; one workgroup: <= 4096, <= 8192, <= 16384; generic above, and for odd B)
CASES = [(64, 3, 9, 1, "k_squelch_wave<4>"), (512, 257, 3, 1, "k_squelch_wave<4>"), (514, 3, 4, 3, "k_squelch_wave<16>"), (2048, 3, 4, 1, "k_squelch_wave<16>"),
         (2050, 3, 3, 16, "k_squelch_wg<8>"), (4096, 1, 3, 1, "k_squelch_wg<8>"), (4098, 3, 2, 1, "k_squelch_wg<16>"), (8192, 3, 2, 1000, "k_squelch_wg<16>"),
         (8194, 1, 2, 1, "k_squelch_wg<32>"), (16384, 3, 3, 1, "k_squelch_wg<32>"), (16386, 3, 2, 1, "k_squelch_generic"), (1001, 3, 5, 1, "k_squelch_generic"),
         (1024, 257, 4, 1, "k_squelch_wave<16>")]


def _case(B, n_ch, nb, d):
    """n_ch channels of nb near-threshold blocks and a tail of B / 3 samples that stays in the object, their levels, and the CPU hook's results.
    d = 1: powers within 2 % of the channel's level, alternately above and below it.  d > 1: the decimated sum sees n / B of the terms and scatters with
    their number, so the level sits at that share of the mean power and the powers spread by half of it"""
    rng = np.random.default_rng(B * 7 + n_ch)
    lv = LEVEL * rng.uniform(0.5, 2.0, n_ch)
    rows, lvd = [], []
    for c in range(n_ch):
        if d == 1:
            powers = lv[c] * (1 + 0.02 * rng.uniform(0.01, 1, nb) * np.where((np.arange(nb) + c) % 2, 1, -1))
            lvd.append(float(np.float32(lv[c])))
        else:
            powers = lv[c] * (1 + 0.5 * rng.uniform(-1, 1, nb))
            lvd.append(float(np.float32(lv[c] * sm.n_terms(B, d) / B)))
        rows.append(np.concatenate([sm.noise_blocks(rng, nb, B, powers), np.zeros(B // 3, np.complex64)]))
    x = np.stack(rows)
    return x, lvd, _hook(x, B, d, lvd)


@pytest.mark.parametrize("B,n_ch,nb,d,kernel", CASES)
def test_object_vs_hook(ctx, B, n_ch, nb, d, kernel):
    """powers, flags and outputs equal the CPU hook's bit for bit on near-threshold blocks (half of them closed): the one-pass kernel of this B, the
    generic kernel, pitches larger than the row, and calls cut at random points (inside a block, shorter than B); open blocks are the input's bytes,
    closed blocks all-zero bytes"""
    x, lvd, want = _case(B, n_ch, nb, d)
    fl = np.concatenate([w[2] for w in want])
    assert 0 < fl.sum() < fl.size
    for c, (wo, wp, wf) in enumerate(want):
        blocks_in, blocks_out = x[c, :nb * B].reshape(nb, B), wo.reshape(nb, B)
        assert blocks_out[wf == 1].tobytes() == blocks_in[wf == 1].tobytes()
        assert not blocks_out[wf == 0].view(np.uint8).any()
    rng = np.random.default_rng(B)
    n = x.shape[1]
    even = n + (n & 1)                                                   # the one-pass kernels take 16-byte aligned rows: even pitches
    o = ctx.squelch(n_ch, B, d, lvd)
    _same(o.process(x, in_pitch=even), want, "one call")
    assert o.kernel_name() == kernel
    o.reset(); o.force_generic(True)
    _same(o.process(x, in_pitch=even), want, "generic")
    assert o.kernel_name() == "k_squelch_generic"
    o.force_generic(False); o.reset()
    _same(o.process(x, in_pitch=even + 6, out_pitch=(nb + 1) * B + 10), want, "pitched")
    assert o.kernel_name() == kernel
    o.reset()
    _same(o.process(x, in_pitch=even + 7, out_pitch=(nb + 1) * B + 9), want, "odd pitches")
    assert o.kernel_name() == "k_squelch_generic"
    cuts = sorted(int(v) for v in rng.integers(0, n, 5))
    calls = [b - a for a, b in zip([0] + cuts, cuts + [n])] if n_ch < 100 else [B // 2 + 1, n - B // 2 - 1]
    o.reset()
    _same(o.process(x, calls), want, "cut")
    assert o.block_index(0) == nb and o.block_index(n_ch - 1) == nb
    calls = [1] * 3 + [B // 5] * 4
    calls.append(n - sum(calls))
    if n_ch < 100:
        o.reset()
        _same(o.process(x, calls), want, "short calls")
    o.close()


@pytest.mark.parametrize("B,spread,nb", [(1024, 0.01, 300), (16384, 0.10, 100)])
def test_object_vs_reference(ctx, B, spread, nb):
    """decisions equal the reference's outside the undecidable blocks (|P - level| within the gate; at most 5 % of the blocks, the reference alone first),
    powers within the gate of the float64 power; then blocks in two classes 6 dB apart: all decisions equal"""
    L = sm.ref_lib()
    if L is None:
        pytest.skip("reference library not built")
    rng = np.random.default_rng(B + 1)
    x = sm.near_threshold(rng, nb, B, LEVEL, spread)
    P = np.array([sm.power64(x[k * B:(k + 1) * B]) for k in range(nb)])
    gate = np.array([sm.bound(B, 1, p) for p in P])
    und = np.abs(P - LEVEL) <= gate
    assert und.sum() <= 0.05 * nb
    _, rp, rf = sm.ref_stream(L, x, B, 1, LEVEL)
    assert np.all(np.abs(rp.astype(np.float64) - P) <= gate)
    assert np.array_equal(rf[~und], (P >= LEVEL)[~und])
    o = ctx.squelch(1, B, 1, [LEVEL])
    out, pw, fl = o.process(x)
    assert np.all(np.abs(pw.astype(np.float64) - P) <= gate)
    assert np.array_equal(fl[~und], rf[~und])
    assert 0.3 * nb < fl.sum() < 0.7 * nb
    x2, _ = sm.two_class(rng, 24, B, LEVEL)
    ro, _, rf2 = sm.ref_stream(L, x2, B, 1, LEVEL)
    o.reset()
    out2, _, fl2 = o.process(x2)
    assert np.array_equal(fl2, rf2) and out2.tobytes() == ro.tobytes() and 0 < fl2.sum() < 24
    o.close()


def test_levels_between_calls(ctx):
    """per-channel levels; set_level between calls takes effect from the next block a later call starts (a block already begun keeps its level); level 0
    opens everything; channel -1 sets all"""
    B, nb = 1024, 8
    rng = np.random.default_rng(11)
    x = np.stack([sm.two_class(rng, nb, B, LEVEL)[0] for _ in range(3)])
    lv = [LEVEL, LEVEL * 100, 0.0]
    o = ctx.squelch(3, B, 1, lv)
    assert [o.get_level(c) for c in range(3)] == [float(np.float32(v)) for v in lv]
    # call 1 ends inside block 1, call 2 inside block 2: the level set in front of call 1 holds from block 2, the one in front of call 2 from block 3
    calls = [1500, 1000, nb * B - 2500]
    got = o.process(x, calls, levels_between={1: [(0, LEVEL * 100), (1, 0.0)], 2: [(-1, LEVEL)]})
    want = [sm.stream(x[0], B, 1, lv[0], {1: LEVEL * 100, 2: LEVEL}), sm.stream(x[1], B, 1, lv[1], {1: 0.0, 2: LEVEL}), sm.stream(x[2], B, 1, lv[2], {2: LEVEL})]
    _same(got, want, "levels")
    assert not want[0][2][2] and want[1][2][2] and want[2][2][:3].all() and not want[1][2][:2].any()
    # a level set when no block is open applies to the very next block
    o.reset(); o.set_level(-1, LEVEL * 100)
    assert not o.process(x[:, :2 * B])[2][0].any()
    o.close()


def test_inf_nan_inputs(ctx):
    """a NaN power closes the gate unless the level is 0; an infinite power passes; open blocks keep the input's bytes"""
    B = 2048
    rng = np.random.default_rng(12)
    x = sm.noise_blocks(rng, 6, B, np.full(6, LEVEL * 4))
    x[B + 17] = complex(np.nan, 1.0)
    x[2 * B + 600] = complex(np.inf, 0.0)
    x[3 * B + 1999] = complex(0.0, -np.inf)
    x[4 * B + 5] = complex(np.inf, np.nan)
    x = np.stack([x, x])
    o = ctx.squelch(2, B, 1, [LEVEL, 0.0])
    for gen in (False, True):
        o.reset(); o.force_generic(gen)
        out, pw, fl = o.process(x)
        assert list(fl[0]) == [1, 0, 1, 1, 0, 1] and fl[1].all()
        assert np.isnan(pw[0][[1, 4]]).all() and np.isposinf(pw[0][[2, 3]]).all() and pw[0].tobytes() == pw[1].tobytes()
        assert out[1].tobytes() == x[1].tobytes()
        assert out[0].reshape(6, B)[fl[0] == 1].tobytes() == x[0].reshape(6, B)[fl[0] == 1].tobytes()
        assert not out[0].reshape(6, B)[fl[0] == 0].view(np.uint8).any()
    o.close()


def test_reset_channel(ctx):
    """reset_channel drops one channel's held samples and block count: its blocks restart at the next call's first sample, the others carry on"""
    B = 1024
    rng = np.random.default_rng(13)
    x = np.stack([sm.two_class(rng, 7, B, LEVEL)[0] for _ in range(3)])
    o = ctx.squelch(3, B, 1, [LEVEL] * 3)
    first = o.process(x[:, :1500])
    o.reset_channel(1)
    assert o.block_index(1) == 0 and o.block_index(0) == 1
    second = o.process(x[:, 1500:], [3000, 1, x.shape[1] - 4501])
    whole = _hook(x, B, 1, [LEVEL] * 3)
    fresh = _hook(x[1:2, 1500:], B, 1, [LEVEL])[0]
    for c in (0, 2):
        for j in range(3):
            assert np.concatenate([first[j][c], second[j][c]]).tobytes() == whole[c][j].tobytes(), (c, j)
    for j in range(3):
        assert second[j][1].tobytes() == fresh[j].tobytes(), j
    assert o.block_index(0) == 7 and o.block_index(1) == fresh[1].size
    o.close()


def test_stateless_and_dropin_vs_reference(ctx):
    """csdr_amd_get_power_c / _f give the object's bits and lie, as the drop-in get_power_c / get_power_f, within the gate that the reference passes too"""
    import csdr_amd
    L = sm.ref_lib()
    if L is None:
        pytest.skip("reference library not built")
    A = C.CDLL(csdr_amd.lib()._name)
    for f in (A.get_power_c, A.get_power_f):
        f.restype = C.c_float
        f.argtypes = [C.c_void_p, C.c_int, C.c_int]
    rng = np.random.default_rng(14)
    for B, d in ((1000, 1), (1024, 3), (16384, 16), (70, 1000)):
        x = (0.2 * (rng.standard_normal((3, 4 * B)) + 1j * rng.standard_normal((3, 4 * B)))).astype(np.complex64)
        for v, fn in ((x, ctx.get_power_c), (x.real.copy(), ctx.get_power_f)):
            pw = fn(v, B, d)
            assert pw.shape == (3, 4)
            for s in range(3):
                for k in range(4):
                    blk = v[s, k * B:(k + 1) * B]
                    P = sm.power64(blk, d)
                    g = sm.bound(B, d, P)
                    assert pw[s, k].tobytes() == csdr_amd.squelch_debug_power(blk, d).tobytes()
                    assert abs(float(sm.ref_power(L, blk, d)) - P) <= g
                    assert abs(float(pw[s, k]) - P) <= g
            blk = v[1, B:2 * B]
            assert sm.ref_power(A, blk, d).tobytes() == pw[1, 1].tobytes()
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.squelch(1, 0, 1)
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.squelch(1, 1024, 0)
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.squelch(0, 1024, 1)
    o = ctx.squelch(2, 1024, 1)
    d_in = ctx.upload(np.zeros(2 * 4096, np.complex64)); d_out = ctx.alloc(8 * 2 * 4096)
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.process_dev(d_in.ptr, 2048, 2047, d_out.ptr, 4096)              # in_pitch below the row
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.process_dev(d_in.ptr, 2048, 4096, d_out.ptr, 2047)              # out_pitch below the blocks
    o.close()


class _Fifos:
    """a control fifo with a level waiting in it and an out fifo with a reader attached (the reference's open of it blocks otherwise)"""

    def __init__(self, tmp_path):
        self.ctl, self.out = str(tmp_path / "ctl"), str(tmp_path / "out")
        os.mkfifo(self.ctl); os.mkfifo(self.out)
        self.fc = os.open(self.ctl, os.O_RDWR)
        self.fo = os.open(self.out, os.O_RDONLY | os.O_NONBLOCK)

    def level(self, v):
        os.write(self.fc, ("%g\n" % v).encode())

    def reports(self):
        data = b""
        try:
            while True:
                b = os.read(self.fo, 65536)
                if not b:
                    break
                data += b
        except BlockingIOError:
            pass
        return [float(t) for t in data.decode().split()]

    def close(self):
        os.close(self.fc); os.close(self.fo)


def _env(bufsize=None):
    e = dict(os.environ)
    e.pop("CSDR_DYNAMIC_BUFSIZE_ON", None)
    if bufsize:
        e["CSDR_FIXED_BUFSIZE"] = str(bufsize)
    return e


def test_cli_vs_reference(ctx, tmp_path):
    """csdr squelch_and_smeter_cc against oracle/_ref/csdr through pipes, a control fifo and an out fifo: the same stdout bytes for a fixed level at two
    CSDR_FIXED_BUFSIZE values, the same number of report lines at the same blocks (values within the gate and the 6-digit %g rounding), the same error exits"""
    if not os.path.exists(REF_CSDR):
        pytest.skip("reference binary not built")
    f = _Fifos(tmp_path)
    rng = np.random.default_rng(15)
    every, nb = 2, 21                                                    # reports at blocks 3, 7, .. 19; the reference's stale block 21 at EOF reports nothing
    for B in (512, 2048):
        x, _ = sm.two_class(rng, nb, B, LEVEL)
        P = np.array([sm.power64(x[k * B:(k + 1) * B]) for k in range(nb)])
        due = sm.report_replay(every, nb)
        args = ["squelch_and_smeter_cc", "--fifo", f.ctl, "--outfifo", f.out, "1", str(every)]
        outs, reps = [], []
        for exe in (REF_CSDR, CSDR):
            f.level(LEVEL)
            r = subprocess.run([exe] + args, input=x.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=_env(B))
            assert r.returncode == 0, r.stderr.decode()[-2000:]
            outs.append(r.stdout); reps.append(f.reports())
        want = sm.stream(x, B, 1, LEVEL)[0].tobytes()
        # (the reference repeats its last buffer once at EOF: its stream is ours plus at most that stale block)
        assert outs[1] == want and outs[0][:len(want)] == want and len(outs[0]) - len(want) in (0, 8 * B)
        assert len(reps[0]) == len(reps[1]) == len(due) == 5
        for k, a, b in zip(due, reps[0], reps[1]):
            tol = sm.bound(B, 1, P[k]) + 5e-6 * P[k]
            assert abs(a - P[k]) <= tol and abs(b - P[k]) <= tol, (B, k, a, b, P[k])
    for args in ([], ["--fifo", f.ctl], ["--fifo", f.ctl, "--outfifo", f.out], ["--fifo", f.ctl, "--outfifo", f.out, "1"],
                 ["--fifo", f.ctl, "--outfifo", f.out, "0", "5"], ["--fifo", f.ctl, "--outfifo", f.out, "1", "0"]):
        rcs = []
        for exe in (REF_CSDR, CSDR):
            f.level(LEVEL)
            r = subprocess.run([exe, "squelch_and_smeter_cc"] + args, input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, env=_env())
            rcs.append(r.returncode)
        assert rcs[0] == rcs[1] != 0, (args, rcs)
    f.close()


def test_chain_stage(ctx, tmp_path):
    """`csdr chain` with the command between two existing stages (input and output resident in HBM) equals the three separate processes"""
    f = _Fifos(tmp_path)
    rng = np.random.default_rng(16)
    x, _ = sm.two_class(rng, 40, 1024, LEVEL)
    sq = "squelch_and_smeter_cc --fifo %s --outfifo %s 1 3" % (f.ctl, f.out)
    f.level(LEVEL)
    a = subprocess.run([CSDR, "chain", "shift_addition_cc 0.05 | %s | realpart_cf" % sq], input=x.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120, env=_env())
    assert a.returncode == 0, a.stderr.decode()[-2000:]
    ra = f.reports()
    f.level(LEVEL)
    b = subprocess.run(["sh", "-c", "%s shift_addition_cc 0.05 | %s %s | %s realpart_cf" % (CSDR, CSDR, sq, CSDR)], input=x.tobytes(), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120, env=_env())
    assert b.returncode == 0, b.stderr.decode()[-2000:]
    rb = f.reports()
    assert len(a.stdout) == 4 * x.size and a.stdout == b.stdout
    assert ra == rb and len(ra) == len(sm.report_replay(3, 40))
    y = np.frombuffer(a.stdout, np.float32).reshape(40, 1024)
    fl = sm.stream(x, 1024, 1, LEVEL)[2]
    assert 0 < fl.sum() < 40 and not y[fl == 0].any() and y[fl == 1].any(axis=1).all()
    f.close()
