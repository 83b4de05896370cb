"""GPU checks of the complex-tap FIR (cfir.hip): the matrix-core kernel, the generic kernel, the CPU walk and the float32 model bit for bit at every
filter length class, around the tile size, with several tiles per wave, per-channel taps, padded and 8-byte-odd rows; streaming, reset and retune;
the stateless call; the reference's golden vectors; the CLI command, alone and in `csdr chain`; the Python wrapper and the drop-in symbol.
Inputs are finite everywhere: Inf / NaN is the documented exception to bit equality on the matrix cores."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import cfir_model as cm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_CSDR = os.path.join(ROOT, "oracle", "_ref", "csdr")
CSDR = os.path.join(ROOT, "csdr_amd", "csdr")
TO = 512                  # outputs per tile of k_cfir_mfma
MFMA, GENERIC = "k_cfir_mfma", "k_cfir_generic"


@pytest.fixture(scope="module")
def ctx():
    import csdr_amd
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _bits(y):
    return np.ascontiguousarray(y, np.complex64).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _inputs(n_ch, n, seed):
    return np.stack([cm.signal(n, seed + k) for k in range(n_ch)])


def _taps(n_ch, T, seed):
    return np.stack([cm.random_taps(T, seed + k) for k in range(n_ch)])


def _bank(ctx, h, generic=False):
    o = ctx.cfir(h.shape[0], h.shape[1])
    o.set_taps(h)
    if generic:
        o.force_generic(True)
    return o


@pytest.mark.parametrize("T,kernel", [(1, MFMA), (2, MFMA), (7, MFMA), (101, MFMA), (255, MFMA), (256, MFMA), (257, GENERIC)])
def test_bits_equal_model_every_length(ctx, T, kernel):
    """both kernels, the CPU walk and cfir32 agree to the bit; filters above 256 taps take the generic kernel by themselves"""
    import csdr_amd
    x, h = _inputs(3, 2600, T), _taps(3, T, 100 + T)
    a = _bank(ctx, h)
    ya = a.process(x)
    assert a.kernel_name() == kernel
    g = _bank(ctx, h, generic=True)
    yg = g.process(x)
    assert g.kernel_name() == GENERIC
    for k in range(3):
        want = cm.cfir32(x[k], h[k])
        assert want.size == 2600 - T + 1
        assert _same(ya[k], want) and _same(yg[k], want) and _same(csdr_amd.cfir_debug_walk(h[k], x[k]), want), (T, k)


@pytest.mark.parametrize("n_out", [1, TO - 1, TO, TO + 1, 3 * TO + 5])
def test_output_counts_around_the_tile(ctx, n_out):
    T = 7
    x, h = _inputs(2, n_out + T - 1, n_out), _taps(2, T, 9)
    a = _bank(ctx, h)
    y = a.process(x)
    assert a.kernel_name() == MFMA
    for k in range(2):
        assert _same(y[k], cm.cfir32(x[k], h[k])), (n_out, k)


def test_several_tiles_per_wave_partial_last_tile(ctx):
    """8 channels x 1 100 013 samples: 2149 tiles per channel, so the launch gives a wave 2 tiles (tiles x channels / 8192) and the last wave of a
    channel one, partial, tile.  Rows 0, 3 and 7 are compared at both ends, across tile and wave boundaries and in the partial tile."""
    T, n_ch, n = 33, 8, 1100013
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((n_ch, n), np.float32) + 1j * rng.standard_normal((n_ch, n), np.float32)).astype(np.complex64)
    h = _taps(n_ch, T, 40)
    a = _bank(ctx, h)
    y = a.process(x)
    assert a.kernel_name() == MFMA
    n_out = n - T + 1
    assert (n_out + TO - 1) // TO == 2149
    spans = [(0, 2100), (TO - 50, TO + 50), (2 * TO - 50, 2 * TO + 50), (1074 * 2 * TO - 300, n_out), (n_out - 1500, n_out)]
    for k in (0, 3, 7):
        assert y[k].size == n_out
        for lo, hi in spans:
            assert _same(y[k][lo:hi], cm.cfir32(x[k, lo:hi + T - 1], h[k])), (k, lo)


@pytest.mark.parametrize("n_ch", [1, 3, 65])
def test_taps_per_channel(ctx, n_ch):
    """every channel its own taps; one channel all-zero taps, one a pure delay (a tap at T - 1 only): a row taken from the wrong channel shows"""
    T, n = 31, 1700
    x, h = _inputs(n_ch, n, 300), _taps(n_ch, T, 400)
    zero, delay = n_ch // 2, n_ch - 1
    h[delay] = 0; h[delay, T - 1] = 1
    if n_ch > 1:
        h[zero] = 0
    for generic in (False, True):
        o = _bank(ctx, h, generic)
        y = o.process(x)
        assert o.kernel_name() == (GENERIC if generic else MFMA)
        for k in range(n_ch):
            assert _same(y[k], cm.cfir32(x[k], h[k])), (n_ch, k)
        assert _same(y[delay], x[delay, T - 1:])
        if n_ch > 1:
            assert not y[zero].view(np.uint32).any()


def test_padded_rows_and_odd_row_offsets(ctx):
    """in_pitch / out_pitch above n, odd, and both buffers starting an odd number of samples into their allocations: rows alternate between 16-byte
    aligned and 8 bytes off, so the 16-byte stores and the 8-byte stores both run; what lies between the rows is not written"""
    T, n_ch, n = 21, 5, 2 * TO + 77
    x, h = _inputs(n_ch, n, 500), _taps(n_ch, T, 600)
    ip, op, n_out = n + 3, n + 5, n - T + 1
    for off in (1, 2):
        for generic in (False, True):
            hin = np.zeros(off + n_ch * ip, np.complex64)
            for k in range(n_ch):
                hin[off + k * ip: off + k * ip + n] = x[k]
            sentinel = np.complex64(-7.5 + 3.25j)
            hout = np.full(off + n_ch * op, sentinel, np.complex64)
            di, do, dc = ctx.upload(hin), ctx.upload(hout), ctx.alloc(4 * n_ch + 64)
            o = _bank(ctx, h, generic)
            o.process_dev(di.at(8 * off), n, ip, do.at(8 * off), op, dc.ptr)
            got = ctx.download(do, np.complex64, hout.size)
            assert list(ctx.download(dc, np.int32, n_ch)) == [n_out] * n_ch
            assert o.kernel_name() == (GENERIC if generic else MFMA)
            assert np.all(got[:off] == sentinel)
            for k in range(n_ch):
                row = got[off + k * op: off + (k + 1) * op]
                assert _same(row[:n_out], cm.cfir32(x[k], h[k])), (off, generic, k)
                assert np.all(row[n_out:] == sentinel), (off, generic, k)


@pytest.mark.parametrize("T", [7, 101])
def test_streaming_counts_and_reset_channel(ctx, T):
    """three calls equal one call, per channel, with the right counts; reset_channel restarts one channel only"""
    n_ch = 3
    for calls in ([T - 2, 1, 2000], [5, 0, 1999]):
        n = sum(calls)
        x, h = _inputs(n_ch, n, 700 + T), _taps(n_ch, T, 800)
        for generic in (False, True):
            whole = _bank(ctx, h, generic).process(x)
            o = _bank(ctx, h, generic)
            di, do, dc = ctx.upload(x), ctx.alloc(8 * n_ch * n + 64), ctx.alloc(4 * n_ch + 64)
            at, parts, held = 0, [[] for _ in range(n_ch)], 0
            for m in calls:
                o.process_dev(di.at(8 * at), m, n, do.ptr, n, dc.ptr)
                cnt = ctx.download(dc, np.int32, n_ch)
                want = max(0, held + m - T + 1)
                assert list(cnt) == [want] * n_ch, (calls, m)
                y = ctx.download(do, np.complex64, n_ch * n).reshape(n_ch, n)
                for k in range(n_ch):
                    parts[k].append(y[k, :want].copy())
                held = min(T - 1, held + m)
                at += m
            for k in range(n_ch):
                assert _same(np.concatenate(parts[k]), whole[k]) and _same(whole[k], cm.cfir32(x[k], h[k])), (calls, generic, k)
    # reset_channel
    o = _bank(ctx, h)
    first = o.process(x[:, :900])
    o.reset_channel(1)
    second = o.process(x[:, 900:])
    assert _same(second[1], cm.cfir32(x[1, 900:], h[1]))
    for k in (0, 2):
        assert _same(np.concatenate([first[k], second[k]]), cm.cfir32(x[k], h[k]))
    o.reset()
    assert _same(o.process(x[:, 900:])[2], cm.cfir32(x[2, 900:], h[2]))


def test_retune_between_calls(ctx):
    """set_peaks on one channel between two calls: the second call's outputs are the new taps over the kept history and the new input, no gap and no
    repeat; the other channels go on as they were"""
    import csdr_amd
    T, n_ch, n1, n2 = 101, 3, 1500, 1800
    x = _inputs(n_ch, n1 + n2, 900)
    old = [csdr_amd.firdes_peaks_c(T, [0.05 * (k + 1)]) for k in range(n_ch)]
    new = csdr_amd.firdes_peaks_c(T, [0.11, -0.3])
    for generic in (False, True):
        o = ctx.cfir(n_ch, T)
        if generic:
            o.force_generic(True)
        for k in range(n_ch):
            o.set_peaks([0.05 * (k + 1)], channel=k)
        first = o.process(x[:, :n1])
        o.set_peaks([0.11, -0.3], channel=1)
        second = o.process(x[:, n1:])
        assert first[1].size == n1 - T + 1 and second[1].size == n2
        assert _same(first[1], cm.cfir32(x[1, :n1], old[1]))
        assert _same(second[1], cm.cfir32(x[1, n1 - (T - 1):], new))
        for k in (0, 2):
            assert _same(np.concatenate([first[k], second[k]]), cm.cfir32(x[k], old[k]))
    # set_peaks for every channel at once, and set_taps of one channel
    o = ctx.cfir(2, T)
    o.set_peaks([0.11, -0.3])
    o.set_taps(old[0], channel=1)
    y = o.process(x[:2, :n1])
    assert _same(y[0], cm.cfir32(x[0, :n1], new)) and _same(y[1], cm.cfir32(x[1, :n1], old[0]))


def test_stateless_call(ctx):
    """csdr_amd_apply_fir_cc with one tap row for all streams (taps_pitch 0) and with a row per stream equals the object; short rows give nothing"""
    T, n_ch, n = 64, 4, TO + 300
    x, h = _inputs(n_ch, n, 1000), _taps(n_ch, T, 1100)
    per = _bank(ctx, h).process(x)
    shared = _bank(ctx, np.repeat(h[:1], n_ch, axis=0)).process(x)
    for generic in (False, True):
        y = ctx.apply_fir_cc(x, h, force_generic=generic)
        assert ctx.last_apply_fir_kernel == (GENERIC if generic else MFMA)
        ys = ctx.apply_fir_cc(x, h[0], force_generic=generic)
        for k in range(n_ch):
            assert _same(y[k], per[k]) and _same(ys[k], shared[k]) and _same(ys[k], cm.cfir32(x[k], h[0]))
    assert ctx.apply_fir_cc(x[:, :T - 1], h).shape == (n_ch, 0)
    assert _same(ctx.apply_fir_cc(x[0], cm.random_taps(300, 5)), cm.cfir32(x[0], cm.random_taps(300, 5))) and ctx.last_apply_fir_kernel == GENERIC


def test_reference_golden_vectors(ctx):
    """the device's outputs are within the gate of the reference's committed outputs"""
    z = np.load(cm.GOLDEN)
    for k in range(3):
        x, h, yref = z["x%d" % k], z["h%d" % k], z["y%d" % k]
        for generic in (False, True):
            y = ctx.apply_fir_cc(x, h, force_generic=generic)
            assert cm.within(y, yref.astype(np.complex128), cm.cfir_gate(x, h)), (k, generic)


def test_object_refusals(ctx):
    import csdr_amd
    L = ctx.L
    for n_ch, T, msg in [(1, 0, "taps_length should be 1 .. 65536"), (1, 65537, "taps_length should be 1 .. 65536"), (0, 11, "n_channels should be"),
                         (1 << 20, 4096, "n_channels x taps_length")]:
        with pytest.raises(csdr_amd.CsdrAmdError, match=msg):
            ctx.cfir(n_ch, T)
    o = ctx.cfir(2, 11)
    h = np.ones(11, np.complex64)
    r = np.array([0.1], np.float32)
    for call, msg in [(lambda: L.csdr_amd_cfir_set_taps(o.h, 2, cm._p(h)), "channel out of range"), (lambda: L.csdr_amd_cfir_set_taps(o.h, -2, cm._p(h)), "channel out of range"),
                      (lambda: L.csdr_amd_cfir_set_taps(o.h, 0, None), "null taps"), (lambda: L.csdr_amd_cfir_set_peaks(o.h, 0, None, 1, 2), "null rates"),
                      (lambda: L.csdr_amd_cfir_set_peaks(o.h, 0, cm._p(r), 0, 2), "at least one peak rate"), (lambda: L.csdr_amd_cfir_set_peaks(o.h, 5, cm._p(r), 1, 2), "channel out of range"),
                      (lambda: L.csdr_amd_cfir_reset_channel(o.h, 2), "channel out of range"), (lambda: L.csdr_amd_cfir_process(o.h, None, 10, 10, None, 10, None), "need in_pitch >= n"),
                      (lambda: L.csdr_amd_apply_fir_cc(ctx.h, None, None, 1, 10, 10, 10, None, 0, 3, 0), "null or unaligned taps"),
                      (lambda: L.csdr_amd_apply_fir_cc(ctx.h, None, None, 1, 10, 10, 10, cm._p(h), 0, 0, 0), "taps_length should be")]:
        assert call() < 0 and msg in ctx.err(), msg
    # taps start all-zero
    assert not o.process(np.ones((2, 50), np.complex64))[0].view(np.uint32).any()


def _run(cmd, data, timeout=120):
    r = subprocess.run(cmd, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


def test_cli_peaks_fir_cc(ctx):
    """`csdr peaks_fir_cc 31 0.1 -0.2` through a pipe equals the model with those taps byte for byte, also as stages of `csdr chain`; the reference
    binary agrees on its whole-block prefix; the reference's refusals"""
    import csdr_amd
    x = cm.signal(8192, 1200)
    h = csdr_amd.firdes_peaks_c(31, [0.1, -0.2])
    want = cm.cfir32(x, h)
    out = _run([CSDR, "peaks_fir_cc", "31", "0.1", "-0.2"], x.tobytes())
    assert out == want.tobytes()
    h2 = csdr_amd.firdes_peaks_c(7, [0.05])
    out2 = _run([CSDR, "chain", "peaks_fir_cc 31 0.1 -0.2 | peaks_fir_cc 7 0.05"], x.tobytes())
    assert out2 == cm.cfir32(want, h2).tobytes()
    for args, msg in ((["peaks_fir_cc"], "(taps_length)"), (["peaks_fir_cc", "31"], "(peak_rate)"), (["peaks_fir_cc", "1024", "0.1"], "decrease taps_length"),
                      (["peaks_fir_cc", "0", "0.1"], "at least 1")):
        r = subprocess.run([CSDR] + args, input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode != 0 and msg in r.stderr.decode(), (args, r.stderr.decode()[-300:])
    L = cm.ref_lib()
    if not os.path.exists(REF_CSDR) or L is None:
        return
    yr = np.frombuffer(subprocess.run([REF_CSDR, "peaks_fir_cc", "31", "0.1", "-0.2"], input=x.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                      timeout=120).stdout, np.complex64)
    # the reference stops at its last whole buffer (its feof check follows the short read): a prefix of the stream's valid output
    assert want.size - 1024 < yr.size <= want.size
    href = cm.ref_peaks(L, 31, [0.1, -0.2])
    assert cm.within(yr, cm.cfir64(x, href)[:yr.size], tuple(g[:yr.size] for g in cm.cfir_gate(x, href)))
    # ours against it: each within its own gate of float64, whose two filters differ by the taps' few ulp
    dh = np.correlate(np.abs(x.real) + np.abs(x.imag), np.abs(h.astype(np.complex128) - href).astype(np.float64) * np.sqrt(2), "valid")[:yr.size]
    bound = tuple(a[:yr.size] + b[:yr.size] + dh for a, b in zip(cm.cfir_gate(x, h), cm.cfir_gate(x, href)))
    assert cm.within(want[:yr.size], yr.astype(np.complex128), bound)


def test_python_wrapper_and_dropin(ctx):
    """CFir as a context manager, the module functions, and the drop-in apply_fir_cc as a client of the reference's header calls it"""
    import csdr_amd
    x = cm.signal(3000, 1300)
    h = csdr_amd.firdes_peaks_c(101, [0.07], window="HAMMING")
    assert np.array_equal(_bits(h), _bits(csdr_amd.firdes_peak_c(101, 0.07)))            # one peak: firdes_peak_c into zeroed taps
    want = cm.cfir32(x, h)
    with ctx.cfir(1, 101) as o:
        assert isinstance(o, csdr_amd.CFir) and o.max_out(500) == 500 and o.kernel_name() == MFMA
        o.set_peaks([0.07])
        assert _same(o.process(x, [100, 900, 2000]), want)
    assert _same(csdr_amd.apply_fir_cc(x, h, ctx=ctx), want)
    assert _same(csdr_amd.apply_fir_cc(x, h), want)                                     # on a context of its own
    A = C.CDLL(csdr_amd.lib()._name)
    A.apply_fir_cc.restype = C.c_int
    A.apply_fir_cc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    y = np.zeros(x.size, np.complex64)
    assert A.apply_fir_cc(cm._p(x), cm._p(y), x.size, cm._p(h), h.size) == want.size
    assert _same(y[:want.size], want)
    assert A.apply_fir_cc(cm._p(x), cm._p(y), 100, cm._p(h), h.size) == 0
