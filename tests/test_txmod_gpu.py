"""GPU checks of the transmit side (txmod.hip): fmmod_fc against the float32 model (phases bit for bit, outputs within G), cut and batch-position
invariance, the elementwise operators, the drop-in calls, the CLI commands and `csdr chain` stages, and the fused transmit bank against the composition of
the models with the existing yardsticks: output count, gates per format, cut invariance across the 1024-output chunk edges, retune, reset, kernel choice,
lifecycle and argument errors."""
import ctypes as C
import functools
import os
import subprocess
import numpy as np
import pytest

import txmod_model as tm
from resampler_model import relrms
from test_txmod_cpu import G, CUTS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
FLOAT_GATE = 1e-5                           # the project's gate for float paths: relative RMS against the expected stream
U8_SHARE = 1e-3                             # u8: every byte within 1, and at most this share of the bytes differing


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _calls_of(cuts, n):
    """per-call counts out of a cut list: the cuts, clipped to n, and the rest"""
    calls, left = [], n
    for k in cuts:
        k = min(k, left); calls.append(k); left -= k
    calls.append(left)
    return calls


# ------------------------------------------------------------------ fmmod_fc
@pytest.mark.parametrize("n_streams", [1, 3, 65])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_fmmod_shapes(ctx, n_streams, n):
    """stream s runs FM case s mod 6: phase_io bit-equal to the model, outputs within G; in and out pitches larger than n"""
    X = np.stack([tm.fm_input(s % 6)[:n] for s in range(n_streams)])
    y, last = ctx.fmmod_fc(X, in_pitch=n + 3, out_pitch=n + 5)
    for s in range(n_streams):
        out, ph, _ = tm.fm_model(s % 6)
        assert last[s].view(np.uint32) == ph[n - 1].view(np.uint32), (s, float(last[s]), float(ph[n - 1]))
        dev = tm.maxdev(y[s], out[:n])
        assert dev <= G["fmmod"], (s, dev)


@pytest.mark.parametrize("case", range(len(tm.FM_CASES)))
def test_fmmod_cut_invariance(ctx, case):
    x = tm.fm_input(case)
    _, ph, last_want = tm.fm_model(case)
    whole, last = ctx.fmmod_fc(x)
    assert last.view(np.uint32) == last_want.view(np.uint32)
    for cuts in CUTS[1:]:
        y, l2 = ctx.fmmod_fc(x, calls=_calls_of(cuts, x.size))
        assert tm.words_differing(y, whole) == 0 and l2.view(np.uint32) == last.view(np.uint32), cuts[:4]
    # a phase handed in is where the walk starts
    y, l3 = ctx.fmmod_fc(x[:1000], phase=[1.25])
    want = tm.model_fmmod(x[:1000], 1.25)
    assert l3.view(np.uint32) == want[2].view(np.uint32) and tm.maxdev(y, want[0]) <= G["fmmod"]


def test_fmmod_batch_position_invariance(ctx):
    n = 1500
    rows = [tm.fm_input(c)[:n] for c in (0, 1, 5, 2)]
    alone = [ctx.fmmod_fc(r) for r in rows]
    for order in ([0, 1, 2, 3] * 5, [3, 2, 1, 0] * 17 + [1]):
        y, last = ctx.fmmod_fc(np.stack([rows[k] for k in order]))
        for pos, k in enumerate(order):
            assert tm.words_differing(y[pos], alone[k][0]) == 0 and last[pos].view(np.uint32) == alone[k][1].view(np.uint32), (pos, k)


# ------------------------------------------------------------------ the elementwise operators
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_elementwise_operators(ctx, n):
    z = tm.elementwise_input(n, n, zeros=True)
    x = np.ascontiguousarray(z.real)
    assert tm.words_differing(ctx.dsb_fc(x, 0.25), tm.dsb(x, 0.25)) == 0
    assert tm.words_differing(ctx.dsb_fc(x), tm.dsb(x)) == 0
    assert tm.words_differing(ctx.add_dcoffset_cc(z), tm.add_dcoffset(z)) == 0
    assert np.array_equal(ctx.convert_f_samplerf(x, 123456789), tm.samplerf(x, 123456789))
    got, want = ctx.fixed_amplitude_cc(z, 0.7), tm.fixed_amplitude(z, 0.7)
    dev = tm.maxdev(got, want)
    assert dev <= G["fixed_amplitude"], dev
    assert np.all(got[z == 0] == 0)


# ------------------------------------------------------------------ the drop-in
def test_dropin(ctx):
    import csdr_amd
    A = tm.bind(C.CDLL(csdr_amd.lib()._name))
    for case in (0, 3, 5):
        x = tm.fm_input(case)[:5000]
        out, ph, _ = tm.fm_model(case)
        y, last = tm.lib_fmmod(A, x, 0.0, [1024, 1024, 1024, 1024, 904])
        assert last.view(np.uint32) == ph[4999].view(np.uint32)
        assert tm.maxdev(y, out[:5000]) <= G["fmmod"]
    z = tm.elementwise_input(3001, 5, zeros=True)
    assert tm.words_differing(tm.lib_add_dcoffset(A, z), tm.add_dcoffset(z)) == 0
    assert tm.maxdev(tm.lib_fixed_amplitude(A, z, 0.7), tm.fixed_amplitude(z, 0.7)) <= G["fixed_amplitude"]


# ------------------------------------------------------------------ the CLI
def _run(cmd, data, timeout=120):
    r = subprocess.run(cmd, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


def test_cli_commands(ctx):
    x = tm.fm_input(0)[:5000]                                       # not a multiple of the 1024-sample buffer: the tail is processed too
    out, ph, _ = tm.fm_model(0)
    y = np.frombuffer(_run([CSDR, "fmmod_fc"], x.tobytes()), np.complex64)
    assert y.size == 5000 and tm.maxdev(y, out[:5000]) <= G["fmmod"]
    y = np.frombuffer(_run([CSDR, "dsb_fc"], x.tobytes()), np.complex64)
    assert tm.words_differing(y, tm.dsb(x)) == 0
    y = np.frombuffer(_run([CSDR, "dsb_fc", "0.5"], x.tobytes()), np.complex64)
    assert tm.words_differing(y, tm.dsb(x, 0.5)) == 0
    z = tm.elementwise_input(5000, 9, zeros=True)
    y = np.frombuffer(_run([CSDR, "add_dcoffset_cc"], z.tobytes()), np.complex64)
    assert tm.words_differing(y, tm.add_dcoffset(z)) == 0
    y = np.frombuffer(_run([CSDR, "fixed_amplitude_cc", "0.7"], z.tobytes()), np.complex64)
    assert y.size == 5000 and tm.maxdev(y, tm.fixed_amplitude(z, 0.7)) <= G["fixed_amplitude"]
    y = np.frombuffer(_run([CSDR, "convert_f_samplerf", "4000"], x.tobytes()), np.uint8)
    assert np.array_equal(y, tm.samplerf(x, 4000))


def test_cli_chain_stages(ctx, port):
    x = tm.fm_input(1)
    out, ph, _ = tm.fm_model(1)
    y = np.frombuffer(_run([CSDR, "chain", "gain_ff 1 | fmmod_fc | add_dcoffset_cc"], x.tobytes()), np.complex64)      # the phase is carried across the passes
    assert y.size == x.size and tm.maxdev(y, tm.add_dcoffset(out)) <= G["fmmod"]
    # the AM line of qtcsdr: convert_i16_f | dsb_fc | add_dcoffset_cc
    a = tm.bank_audio(1, 6000, 3)[0]
    y = np.frombuffer(_run([CSDR, "chain", "convert_i16_f | dsb_fc | add_dcoffset_cc"], a.tobytes()), np.complex64)
    assert tm.words_differing(y, tm.add_dcoffset(tm.dsb(port.convert_s16_f(a)))) == 0
    y = np.frombuffer(_run([CSDR, "chain", "convert_i16_f | gain_ff 0.5 | convert_f_samplerf 1000"], a.tobytes()), np.uint8)
    assert np.array_equal(y, tm.samplerf(port.gain_ff(port.convert_s16_f(a), 0.5), 1000))


def test_cli_ssb_transmit_chain(ctx, port):
    """dsb_fc | bandpass_fir_fft_cc 0 0.1 0.01 | gain_ff 2 | shift_addition_cc 0.2 as one resident chain against the oracle's stages"""
    a = port.convert_s16_f(tm.bank_audio(1, 40000, 4)[0])
    got = np.frombuffer(_run([CSDR, "chain", "dsb_fc | bandpass_fir_fft_cc 0 0.1 0.01 | gain_ff 2 | shift_addition_cc 0.2"], a.tobytes()), np.complex64)
    nt = port.firdes_filter_len(0.01); fft = port.next_pow2(nt)
    if fft - nt < 200:
        fft *= 2                                                    # csdr.c:1834-1836
    bp = port.bandpass_fir_fft_cc(tm.dsb(a), port.firdes_bandpass_c(nt, 0.0, 0.1), fft)
    want, _ = port.shift_addition_cc(port.gain_ff(np.ascontiguousarray(bp).view(np.float32), 2.0).view(np.complex64), 0.2)
    m = min(got.size, want.size)
    assert m >= 40000 - 2 * fft and m > 20000, (got.size, want.size)
    err = relrms(got[:m], want[:m])
    assert err <= FLOAT_GATE, err


def test_cli_bad_argv(ctx):
    def fails(args, message):
        r = subprocess.run([CSDR] + args, input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
    fails(["fixed_amplitude_cc"], b"need required parameter (new_amplitude)")
    fails(["convert_f_samplerf"], b"need required parameter (wait_for_this_sample)")
    fails(["chain", "dsb_fc | fixed_amplitude_cc"], b"need required parameter (new_amplitude)")


# ------------------------------------------------------------------ the bank
def _rates(n_streams):
    return np.array([0.11, -0.2, 0.37, -0.013, 0.45, -0.41, 0.05, 0.29, -0.33, 0.17, -0.07, 0.41, -0.27, 0.02, 0.23, -0.49, 0.31][:n_streams], np.float32)


@functools.lru_cache(maxsize=None)
def _taps(I, T):
    import oracle
    t = oracle.port().firdes_lowpass_f(T, 0.5 / max(I, 2))
    t.setflags(write=False)
    return t


def _check_format(got, want, fmt, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if fmt == "u8":
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        share = float(np.mean(d != 0)) if d.size else 0.0
        print("%s: u8 bytes differing %.3g, largest difference %d" % (what, share, d.max(initial=0)))
        assert d.max(initial=0) <= 1 and share <= U8_SHARE, (what, int(d.max(initial=0)), share)
    else:
        err = relrms(got, want)
        print("%s: cf32 relative RMS %.3g" % (what, err))
        assert err <= FLOAT_GATE, (what, err)


CALLS = [1000, 0, 1, 2048, 1, 0, 1000]      # n_in per call out of {0, 1, 1000, 2048}
BANK_SHAPES = [(4, 79, 1, "fm", "cf32"), (8, 79, 5, "fm", "u8"), (50, 801, 17, "fm", "u8"), (50, 801, 1, "fm", "cf32"), (8, 79, 5, "am", "cf32"),
               (4, 79, 17, "am", "u8"), (50, 801, 5, "dsb", "cf32"), (8, 79, 1, "dsb", "u8"), (4, 79, 17, "dsb", "cf32")]


@pytest.mark.parametrize("I,T,n_streams,mode,fmt", BANK_SHAPES)
def test_bank_vs_expected(ctx, port, I, T, n_streams, mode, fmt):
    n = sum(CALLS)
    gain, q = (0.8, 0.0) if mode == "fm" else (1.5, 0.125)
    x = tm.bank_audio(n_streams, n, I + n_streams)
    rates = _rates(n_streams)
    taps = _taps(I, T)
    o = ctx.txbank(n_streams, mode, I, taps, rates, gain=gain, q_value=q, out_format=fmt, max_in_samples=2048)
    got = o.process(x, CALLS)
    assert o.kernel_name() == "k_tx_up"
    assert got.shape[1] == tm.bank_n_out(n, I, T) == o.max_out(n) - I * ((T - 1 + I - 1) // I)
    for s in range(n_streams):
        want = tm.bank_expected(port, x[s], mode, gain, q, I, taps, [(None, float(rates[s]))], fmt)
        _check_format(got[s], want, fmt, "I %d T %d %s stream %d rate %g" % (I, T, mode, s, rates[s]))
    o.close()


@pytest.mark.parametrize("I,T,edge_calls", [(1, 79, [78 + 1023, 1, 1]), (4, 79, [20 + 255, 1, 1]), (3, 40, [13 + 340, 1, 1])])
@pytest.mark.parametrize("fmt", ["cf32", "u8"])
def test_bank_cut_invariance_and_count(ctx, I, T, edge_calls, fmt):
    """one call against calls that end at 1023, 1024 and 1025 outputs (I = 1), 1020, 1024 and 1028 (I = 4), 1020, 1023 and 1026 (I = 3), 0-sample and
    1-sample calls, both kernels: the same bits; the count after every call is the formula's"""
    n, s = 3000, 3
    x = tm.bank_audio(s, n, 40 + I)
    taps = _taps(I, T)

    def run(calls, generic=False):
        o = ctx.txbank(s, "fm", I, taps, _rates(s), gain=0.9, out_format=fmt, max_in_samples=n)
        o.force_generic(generic)
        total, counts, parts = 0, [], []
        for k in calls:
            parts.append(o.process(x[:, total:total + k])); total += k
            counts.append(sum(p.shape[1] for p in parts))
            assert counts[-1] == tm.bank_n_out(total, I, T), (calls, total)
        assert o.kernel_name() == ("k_tx_up_generic" if generic else "k_tx_up")
        o.close()
        return np.concatenate(parts, axis=1)
    whole = run([n])
    assert whole.shape[1] == tm.bank_n_out(n, I, T) > 2048
    rest = n - sum(edge_calls)
    for calls in (edge_calls + [0, rest], [1] * 30 + [0, 0, 7] + [n - 37], _calls_of(CUTS[1], n)):
        assert np.array_equal(run(calls).view(np.uint8), whole.view(np.uint8)), calls[:5]
    assert np.array_equal(run(edge_calls + [rest], generic=True).view(np.uint8), whole.view(np.uint8))


@pytest.mark.parametrize("fmt", ["cf32", "u8"])
def test_bank_retune_and_reset(ctx, port, fmt):
    I, T, s, n1, n2, n3 = 8, 79, 5, 700, 1, 1500
    x = tm.bank_audio(s, n1 + n2 + n3, 77)
    rates = _rates(s)
    taps = _taps(I, T)
    o = ctx.txbank(s, "fm", I, taps, rates, gain=0.8, out_format=fmt, max_in_samples=2048)
    o.set_rate(4, 0.25)                                             # before any output: the rate of the first segment
    a = o.process(x[:, :n1])
    o.set_rate(2, -0.31); o.set_rate(0, 0.5); o.set_rate(0, -0.05)  # the last one set counts
    b = o.process(x[:, n1:n1 + n2])
    o.set_rate(2, 0.123)
    c = o.process(x[:, n1 + n2:])
    assert [o.get_rate(k) for k in range(s)] == [float(np.float32(v)) for v in (-0.05, rates[1], 0.123, rates[3], 0.25)]
    got = np.concatenate([a, b, c], axis=1)
    na, nb = a.shape[1], b.shape[1]
    assert na == tm.bank_n_out(n1, I, T) and nb == I
    segs = {0: [(na, rates[0]), (None, -0.05)], 1: [(None, rates[1])], 2: [(na, rates[2]), (nb, -0.31), (None, 0.123)], 3: [(None, rates[3])], 4: [(None, 0.25)]}
    for k in range(s):
        want = tm.bank_expected(port, x[k], "fm", 0.8, 0.0, I, taps, [(cnt, float(np.float32(r))) for cnt, r in segs[k]], fmt)
        _check_format(got[k], want, fmt, "retune stream %d" % k)
    # reset: the fresh state, with the rates as they are now
    o.reset()
    again = o.process(x[:, :n1 + n2 + n3], [n1, n2 + n3])
    f = ctx.txbank(s, "fm", I, taps, [o.get_rate(k) for k in range(s)], gain=0.8, out_format=fmt, max_in_samples=4096)
    fresh = f.process(x)
    assert np.array_equal(again.view(np.uint8), fresh.view(np.uint8))
    o.close(); f.close()


@pytest.mark.parametrize("fmt", ["cf32", "u8"])
def test_bank_kernel_choice(ctx, fmt):
    """the fused kernel on aligned rows, the generic one on an unaligned pitch or pointer; the same bits"""
    I, T, s, n = 8, 79, 3, 1200
    x = tm.bank_audio(s, n, 5)
    o = ctx.txbank(s, "am", I, _taps(I, T), _rates(s), gain=1.2, q_value=0.1, out_format=fmt, max_in_samples=n)
    no = tm.bank_n_out(n, I, T)
    a = o.process(x); assert o.kernel_name() == "k_tx_up"
    o.reset(); b = o.process(x, out_pitch=no + 1); assert o.kernel_name() == "k_tx_up_generic"
    o.reset(); c = o.process(x, out_byte_offset=8 if fmt == "cf32" else 2); assert o.kernel_name() == "k_tx_up_generic"
    o.reset(); o.force_generic(True); d = o.process(x); assert o.kernel_name() == "k_tx_up_generic"
    for other in (b, c, d):
        assert np.array_equal(other.view(np.uint8), a.view(np.uint8))
    o.close()


def test_bank_lifecycle_no_growth(ctx):
    import torch
    x = tm.bank_audio(4, 512, 1)
    taps = _taps(8, 79)

    def cycle():
        o = ctx.txbank(4, "fm", 8, taps, _rates(4), out_format="u8", max_in_samples=512)
        o.process(x)
        o.close()
    cycle()
    ctx.sync()
    f0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(200):
        cycle()
    f1 = torch.cuda.mem_get_info(0)[0]
    assert f1 >= f0 - (4 << 20)


def test_bank_argument_errors(ctx):
    import csdr_amd
    L = ctx.L
    taps = np.ascontiguousarray(_taps(8, 79)); rates = _rates(2)
    tp, rp = taps.ctypes.data_as(C.c_void_p), rates.ctypes.data_as(C.c_void_p)
    bad_rates = np.array([0.1, 0.7], np.float32)
    for args in ((0, 0, 1.0, 0.0, 8, tp, 79, rp, 0, 1024), (2, 3, 1.0, 0.0, 8, tp, 79, rp, 0, 1024), (2, 0, 1.0, 0.0, 0, tp, 79, rp, 0, 1024),
                 (2, 0, 1.0, 0.0, 8, None, 79, rp, 0, 1024), (2, 0, 1.0, 0.0, 8, tp, 1, rp, 0, 1024), (2, 0, 1.0, 0.0, 8, tp, 79, None, 0, 1024),
                 (2, 0, 1.0, 0.0, 8, tp, 79, rp, 2, 1024), (2, 0, 1.0, 0.0, 8, tp, 79, rp, 0, 0), (2, 0, float("nan"), 0.0, 8, tp, 79, rp, 0, 1024),
                 (2, 0, 1.0, 0.0, 8, tp, 79, bad_rates.ctypes.data_as(C.c_void_p), 0, 1024)):
        assert not L.csdr_amd_txbank_create(ctx.h, *args), args
        assert b"txbank" in L.csdr_amd_last_error()
    o = ctx.txbank(2, "fm", 8, taps, rates, max_in_samples=1024)
    x = ctx.upload(np.zeros((2, 1024), np.int16)); y = ctx.alloc(2 * 8192 * 8 + 64)
    no = C.c_longlong(-1)
    assert L.csdr_amd_txbank_process(o.h, x.ptr, 1024, 1025, y.ptr, 8192, C.byref(no)) == -3 and b"max_in_samples" in L.csdr_amd_last_error()
    assert L.csdr_amd_txbank_process(o.h, x.ptr, 1024, -1, y.ptr, 8192, C.byref(no)) == -3
    assert L.csdr_amd_txbank_process(o.h, x.ptr, 100, 1024, y.ptr, 8192, C.byref(no)) == -3          # in_pitch < n_in
    assert L.csdr_amd_txbank_process(o.h, x.ptr, 1024, 1024, y.ptr, 100, C.byref(no)) == -3         # out_pitch < outputs
    assert L.csdr_amd_txbank_process(o.h, x.ptr, 1024, 1024, None, 8192, C.byref(no)) == -3
    assert L.csdr_amd_txbank_process(o.h, None, 1024, 1024, y.ptr, 8192, C.byref(no)) == -3
    assert L.csdr_amd_txbank_process(o.h, x.ptr, 1024, 0, None, 0, C.byref(no)) == 0 and no.value == 0      # a 0-sample call is a no-op
    assert L.csdr_amd_txbank_process(None, x.ptr, 1024, 0, None, 0, C.byref(no)) == -3
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.set_rate(2, 0.1)
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.set_rate(0, 0.75)
    with pytest.raises(csdr_amd.CsdrAmdError):
        o.set_rate(0, float("nan"))
    assert L.csdr_amd_txbank_process(o.h, x.ptr, 1024, 1024, y.ptr, 8192, C.byref(no)) == 0 and no.value == (1024 - 10) * 8      # the refused calls left the state alone
    ctx.sync()
    o.close()
    ph = ctx.upload(np.zeros(2, np.float32))
    assert L.csdr_amd_fmmod_fc(ctx.h, x.ptr, y.ptr, 0, 64, 64, 64, ph.ptr) == -3 and b"fmmod_fc" in L.csdr_amd_last_error()
    assert L.csdr_amd_fmmod_fc(ctx.h, x.ptr, y.ptr, 2, 64, 63, 64, ph.ptr) == -3
    assert L.csdr_amd_fmmod_fc(ctx.h, x.ptr, y.ptr, 2, 64, 64, 64, None) == -3
    assert L.csdr_amd_dsb_fc(ctx.h, None, y.ptr, 64, 0.0) == -3
    assert L.csdr_amd_fixed_amplitude_cc(ctx.h, x.ptr, None, 64, 1.0) == -3
