"""The noise sources and the AWGN channel on the GPU: the kernels against the CPU walk of the same header (csdr_amd_debug_noise_walk, held to the model by
test_noise_cpu.py) bit for bit, the flat awgn_cc against the model, the measurements against numpy, and one loop through the pulse-shaped modem."""
import functools

import numpy as np
import pytest

import noise_model as nm
import pulse_model as pm
import pulserx_model as rm

pytestmark = pytest.mark.gpu

u32, f32, c64 = np.uint32, np.float32, np.complex64
SEED = 0x1234567887654321
CHANNELS = [1, 3, 65]
LENGTHS = [1, 2, 3, 63, 64, 65, 4097]            # 4097: more than one workgroup (2048 Philox blocks each) for both kinds
POSITIONS = [0, 1, 2, 3, (1 << 32) - 1, (1 << 33) + 1]


def bits(a):
    return np.ascontiguousarray(a).view(u32)


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def walk(kind, stream_id, pos, n):
    """the CPU walk of one channel, computed once per (kind, id, position, length) and left unchanged"""
    import csdr_amd
    w = csdr_amd.noise_debug_walk(kind, SEED, stream_id, pos, n)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def signal(rows, n):
    rng = np.random.default_rng(rows * 10007 + n)
    x = (rng.uniform(-1, 1, (rows, n)) + 1j * rng.uniform(-1, 1, (rows, n))).astype(c64)
    x.setflags(write=False)
    return x


def mixed(x_row, stream_id, pos, snr_db):
    import csdr_amd
    return csdr_amd.noise_debug_walk("gaussian", SEED, stream_id, pos, x=x_row, snr_db=snr_db)


@pytest.mark.parametrize("kind", ["gaussian", "uniform"])
@pytest.mark.parametrize("N", CHANNELS)
def test_generate_equals_the_walk(ctx, kind, N):
    """every length, a pitch larger than n (odd, so that rows start off 16-byte alignment), custom stream ids, a second call from where the first ended"""
    ids = (np.arange(N) * 7 + 3).astype(u32)
    with ctx.noise(N, kind, SEED, stream_ids=ids) as o:
        at = 0
        for n in LENGTHS:
            pitch = n + 3
            y = o.generate(n, out_pitch=pitch)
            assert o.kernel_name() == ("k_noise_gauss" if kind == "gaussian" else "k_noise_uniform")
            for ch in range(N):
                assert np.array_equal(bits(y[ch]), bits(walk(kind, int(ids[ch]), at, n))), (n, ch)
            at += n
            assert o.position(0) == at and o.position(N - 1) == at
        assert np.array_equal(o.generate(0), np.zeros((N, 0), o.dtype)) and o.position(0) == at


@pytest.mark.parametrize("N", CHANNELS)
def test_fused_awgn_equals_the_walk(ctx, N):
    snr = np.linspace(-10, 40, N).astype(f32) if N > 1 else np.array([6.0], f32)
    with ctx.noise(N, "gaussian", SEED, snr_db=snr) as o:
        at = 0
        for n in LENGTHS:
            x = signal(N, n)
            y = o.awgn_cc(x, in_pitch=n + 1, out_pitch=n + 5)
            assert o.kernel_name() == "k_noise_gauss<awgn>"
            for ch in range(N):
                assert np.array_equal(bits(y[ch]), bits(mixed(x[ch], ch, at, float(snr[ch])))), (n, ch)
            at += n
        for ch in (0, N - 1):
            a, g = o.get_gains(ch)
            ma, mg = nm.awgn_gains(snr[ch])
            assert bits(f32(a)) == bits(f32(ma)) and bits(f32(g)) == bits(f32(mg))


def test_a_channel_is_its_stream_id_wherever_it_sits(ctx):
    with ctx.noise(7, "gaussian", SEED) as seven, ctx.noise(1, "gaussian", SEED, stream_ids=[5]) as one:
        assert np.array_equal(bits(seven.generate(777)[5]), bits(one.generate(777)[0]))
    with ctx.noise(7, "uniform", SEED) as seven, ctx.noise(1, "uniform", SEED, stream_ids=[5]) as one:
        assert np.array_equal(bits(seven.generate(777)[5]), bits(one.generate(777)[0]))


@pytest.mark.parametrize("kind", ["gaussian", "uniform"])
def test_positions_per_channel(ctx, kind):
    N, n = len(POSITIONS), 131
    with ctx.noise(N, kind, SEED) as o:
        for ch, p in enumerate(POSITIONS):
            o.set_position(ch, p)
        y = o.generate(n)
        for ch, p in enumerate(POSITIONS):
            assert np.array_equal(bits(y[ch]), bits(walk(kind, ch, p, n))), p
            assert o.position(ch) == p + n
        if kind == "gaussian":
            o.set_snrs(3.0)
            x = signal(N, n)
            z = o.awgn_cc(x)
            for ch, p in enumerate(POSITIONS):
                assert np.array_equal(bits(z[ch]), bits(mixed(x[ch], ch, p + n, 3.0))), p


@pytest.mark.parametrize("kind", ["gaussian", "uniform"])
def test_two_calls_equal_one(ctx, kind):
    with ctx.noise(3, kind, SEED) as o:
        o.set_position(1, 1); o.set_position(2, 3)
        whole = o.generate(4097)
        o.reset()
        assert o.position(1) == 0
        o.set_position(1, 1); o.set_position(2, 3)
        parts = np.concatenate([o.generate(1001), o.generate(3096)], 1)
        assert np.array_equal(bits(parts), bits(whole))
    if kind == "gaussian":
        x = signal(3, 4097)
        with ctx.noise(3, kind, SEED, snr_db=[0.0, 10.0, 20.0]) as o:
            whole = o.awgn_cc(x)
            o.reset()
            parts = np.concatenate([o.awgn_cc(x[:, :1001]), o.awgn_cc(x[:, 1001:])], 1)
            assert np.array_equal(bits(parts), bits(whole))


def test_reset_channel_touches_only_its_channel(ctx):
    with ctx.noise(4, "gaussian", SEED, snr_db=[1.0, 2.0, 3.0, 4.0]) as o:
        o.generate(100)
        o.reset_channel(2)
        assert [o.position(ch) for ch in range(4)] == [100, 100, 0, 100]
        assert bits(f32(o.get_gains(2)[0])) == bits(f32(nm.awgn_gains(3.0)[0]))           # ids and gains stay
        y = o.generate(50)
        for ch in range(4):
            assert np.array_equal(bits(y[ch]), bits(walk("gaussian", ch, 0 if ch == 2 else 100, 50)))
        x = signal(4, 50)
        z = o.awgn_cc(x)
        assert np.array_equal(bits(z[2]), bits(mixed(x[2], 2, 50, 3.0)))


def test_in_place(ctx):
    x = signal(3, 4097)
    with ctx.noise(3, "gaussian", SEED, snr_db=6.0) as o:
        want = o.awgn_cc(x)
        o.reset()
        assert np.array_equal(bits(o.awgn_cc(x, in_place=True)), bits(want))
        o.reset(); o.set_position(0, 1)
        got = o.awgn_cc(x, in_place=True, in_pitch=4099)
        assert np.array_equal(bits(got[0]), bits(mixed(x[0], 0, 1, 6.0))) and np.array_equal(bits(got[1:]), bits(want[1:]))


def test_arguments(ctx):
    import csdr_amd
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.noise(0)
    with pytest.raises(csdr_amd.CsdrAmdError):
        ctx.noise(1, 2)
    with ctx.noise(2, "uniform", SEED) as o:
        with pytest.raises(csdr_amd.CsdrAmdError):
            o.awgn_cc(signal(2, 8))
        with pytest.raises(csdr_amd.CsdrAmdError):
            o.set_snr_db(0, 3.0)
        with pytest.raises(csdr_amd.CsdrAmdError):
            o.set_position(2, 0)
        with pytest.raises(csdr_amd.CsdrAmdError):
            o.set_position(0, -1)
        with pytest.raises(csdr_amd.CsdrAmdError):
            o.generate(8, out_pitch=7)


# ---------------------------------------------------------------- the flat call, snr_out, the measurements
def test_fused_equals_generate_then_flat(ctx):
    N, n = 5, 4097
    snr = np.array([-10.0, 0.0, 6.0, 20.0, 40.0], f32)
    x = signal(N, n)
    with ctx.noise(N, "gaussian", SEED, snr_db=snr) as o:
        o.set_position(1, 1); o.set_position(3, (1 << 33) + 1)
        fused = o.awgn_cc(x)
        o.reset(); o.set_position(1, 1); o.set_position(3, (1 << 33) + 1)
        noise = o.generate(n)
        gains = [o.get_gains(ch) for ch in range(N)]
    flat = ctx.awgn_cc(x, noise, [a for a, _ in gains], [g for _, g in gains])
    assert np.array_equal(bits(flat), bits(fused))


def test_flat_equals_the_model_on_recorded_noise(ctx):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "awgn_ref_vectors.npz"))
    x, nf, B = g["x"], g["noise_file"].view(c64), int(g["bufsize"])
    noise = nm.awgnfile_noise(nf, B, 4)
    gains = [nm.awgn_gains(s) for s in g["snr_db"]]
    y = ctx.awgn_cc(np.stack([x] * 3), np.stack([noise] * 3), [a for a, _ in gains], [b for _, b in gains])
    for k in range(3):
        assert np.array_equal(bits(y[k]), bits(nm.awgn_mix(x, noise, *gains[k])))
        assert np.array_equal(bits(y[k]), bits(g["y%d" % k][:4 * B]))                  # the reference binary's bytes


def test_snr_out(ctx):
    """within 1e-4 dB of float64 on the same split signal; the output is the same with and without it"""
    N, n = 3, 5000
    snr = np.array([-10.0, 6.0, 40.0], f32)
    x = signal(N, n)
    with ctx.noise(N, "gaussian", SEED, snr_db=snr) as o:
        y, got = o.awgn_cc(x, with_snr=True)
        assert o.kernel_name() == "k_noise_gauss<awgn+snr>"
        o.reset()
        assert np.array_equal(bits(o.awgn_cc(x)), bits(y))
    for ch in range(N):
        a, g = nm.awgn_gains(snr[ch])
        sig = (x[ch].view(f32) * a).astype(f32).view(c64)
        noi = (walk("gaussian", ch, 0, n).view(f32) * g).astype(f32).view(c64)
        want = nm.total_logpower_cf(sig) - nm.total_logpower_cf(noi)
        print("snr_out channel %d: %.6f dB, float64 %.6f dB" % (ch, got[ch], want))
        assert abs(float(got[ch]) - want) < 1e-4


def test_total_logpower(ctx):
    for rows, n in ((1, 1), (3, 2049), (5, 10000)):
        x = signal(rows, n)
        got = ctx.total_logpower_cf(x)
        for r in range(rows):
            want = nm.total_logpower_cf(x[r])
            assert abs(float(got[r]) - want) <= 1e-5 + 2 * np.spacing(f32(abs(want))), (rows, n, r)


def test_count_errors_and_timing_variance(ctx):
    """uneven counts, one of 1 and one of 0.  A count of 1 divides 0 by 0 as the reference does: NaN"""
    rng = np.random.default_rng(3)
    N, La, Lb = 6, 3000, 2500
    a = rng.integers(0, 4, (N, La)).astype(np.uint8)
    lags = np.array([0, 1, 8, 17, 499, 0], np.int32)
    counts = np.array([2500, 1, 0, 777, 2500, 2499], np.int32)
    b = np.stack([a[c, lags[c]:lags[c] + Lb] for c in range(N)]).copy()
    flip = rng.uniform(size=b.shape) < 0.1
    b[flip] ^= 1
    got = ctx.count_errors_u8(a, b, lags, counts)
    want = [int(np.sum(a[c, lags[c]:lags[c] + counts[c]] != b[c, :counts[c]])) for c in range(N)]
    assert list(got) == want and want[0] > 100 and want[2] == 0
    assert list(ctx.count_errors_u8(a, b[:, :100])) == [int(np.sum(a[c, :100] != b[c, :100])) for c in range(N)]
    assert list(ctx.count_errors_u8(a[:, :50], b, counts=counts)) == [int(np.sum(a[c, :min(50, counts[c])] != b[c, :min(50, counts[c])])) for c in range(N)]   # cut to the row
    sps, off = 8, 3
    idx = (off + sps * np.arange(600)[None, :] + rng.integers(-4, 5, (5, 600))).astype(u32)
    cnt = np.array([600, 1, 0, 77, 2], np.int32)
    v = ctx.normalized_timing_variance_u32_f(idx, sps, off, cnt)
    for r in range(5):
        want = nm.normalized_timing_variance_u32_f(idx[r, :cnt[r]], sps, off)
        assert bits(f32(v[r])) == bits(f32(want)) or (np.isnan(v[r]) and np.isnan(want)), r
    assert np.isnan(v[1]) and v[2] == 0 and v[0] > 0
    assert bits(ctx.normalized_timing_variance_u32_f(idx[0], sps, off))[0] == bits(f32(nm.normalized_timing_variance_u32_f(idx[0], sps, off)))


# ---------------------------------------------------------------- one loop through the pulse-shaped modem
LOOP_SEED = 77
DECODE = np.full(9, 255, np.uint8)                                             # (I level, Q level) of the three-level slicers -> symbol; anything else: 255
for sym, (u, v) in enumerate(((2, 1), (1, 2), (0, 1), (1, 0))):
    DECODE[3 * u + v] = sym


def test_loopback_through_the_pulse_modem(ctx):
    """PulseTx (QPSK, 8 samples per symbol, RRC 65 taps) -> awgn_cc -> PulseRx (same taps, a three-level slicer per component) -> count_errors_u8, 16
    channels of 4096 symbols, channel c delayed by 3 + c % 3 samples so that the loop starts near the symbol peaks.  Symbol m peaks at sample 8 m - 64
    behind both filters, so the receiver's first symbol is transmit symbol 8: the lag.  The last 8 symbols are left out (their pulses are cut off).
    40 dB: no errors.  0 dB: the count of the float64 model's noise (rounded to float32) through pulse_model / pulserx_model, channel by channel."""
    import csdr_amd
    I, T, n, S, lag = 8, 65, 4096, 16, 8
    taps = csdr_amd.firdes_rrc_f(T, I, 0.35)
    idx = np.random.default_rng(5).integers(0, 4, (S, n)).astype(np.uint8)
    with ctx.pulse_tx(S, 4, I, taps) as tx:
        y = np.stack(tx.process(idx))
    assert np.array_equal(bits(y), bits(pm.shape32(pm.symbols(4)[idx], I, taps)))
    x = np.zeros((S, y.shape[1] + 8), c64)
    for c in range(S):
        x[c, 3 + c % 3:3 + c % 3 + y.shape[1]] = f32(8) * y[c]
    peak = float(np.sum(taps.astype(np.float64) ** 2))
    lags = np.full(S, lag, np.int32)

    def decoded(byte_rows):
        d = [DECODE[3 * b.reshape(-1, 2)[:, 0] + b.reshape(-1, 2)[:, 1]] for b in byte_rows]
        counts = np.array([min(r.size, n - 8 - lag) for r in d], np.int32)
        rows = np.full((S, max(r.size for r in d)), 255, np.uint8)
        for c, r in enumerate(d):
            rows[c, :r.size] = r
        return rows, counts

    errors = {}
    with ctx.noise(S, "gaussian", LOOP_SEED) as ch:
        for snr in (40.0, 0.0):
            ch.reset(); ch.set_snrs(snr)
            a_signal = float(ch.get_gains(0)[0])
            noisy = ch.awgn_cc(x)
            p = csdr_amd.pulserx_params(taps, "GARDNER", I, 0.5, 2.0, True, 1.0 / (8 * peak * a_signal), 3, True)
            with ctx.pulse_rx(p, S, "filter", "slice") as rx:
                rows, counts = decoded(rx.process(noisy))
            assert counts.min() > n - 30
            errors[snr] = ctx.count_errors_u8(idx, rows, lags, counts)
            if snr == 0.0:
                a, g = nm.awgn_gains(snr)
                model_in = np.stack([nm.awgn_mix(x[c], nm.gaussian(LOOP_SEED, c, 0, x.shape[1]).astype(c64), a, g) for c in range(S)])
                res = rm.receive(model_in, taps, I, rm.GARDNER, True, 0.5, 2.0, rm.FILTER, rm.SLICE, 1.0 / (8 * peak * float(a)), 3, True)
                mrows, mcounts = decoded([r["bytes"] for r in res])
                want = [int(np.sum(idx[c, lag:lag + mcounts[c]] != mrows[c, :mcounts[c]])) for c in range(S)]
    print("loopback errors at 40 dB:", list(errors[40.0]), "at 0 dB:", list(errors[0.0]), "model at 0 dB:", want)
    assert list(errors[40.0]) == [0] * S
    assert all(e > 0 for e in errors[0.0])
    assert list(errors[0.0]) == want
