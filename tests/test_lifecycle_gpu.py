"""Repeated create -> process -> destroy of every stateful library object in one process: device memory must not grow with the number of cycles.

Each object is built and torn down 20 times; free device memory after the last cycle must be within one cycle's footprint of its value after the first
(a leaked state buffer would show as 19 footprints).  Footprints below FLOOR are taken as FLOOR, so that small objects are not judged against the noise of
other work on the card."""
import ctypes as C

import numpy as np
import pytest

import csdr_amd

pytestmark = pytest.mark.gpu

CYCLES = 20
FLOOR = 64 << 20
MIB = 1 << 20


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def ctx():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    c = csdr_amd.Context(0)
    yield c
    c.close()


def _free():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def _cycles(ctx, one):
    """one(ctx) creates, processes and destroys one object; it returns the free memory it saw while the object was alive."""
    after = []; footprint = 0
    for _ in range(CYCLES):
        before = _free()
        alive = one(ctx)
        ctx.sync()
        after.append(_free())
        footprint = max(footprint, before - alive)
    grow = after[0] - after[-1]
    assert grow <= max(footprint, FLOOR), "device memory grew by %d MiB over %d cycles (footprint %d MiB)" % (grow // MIB, CYCLES, footprint // MIB)
    return footprint


def _check(ctx, rc, what):
    if rc < 0:
        raise AssertionError("%s: %s" % (what, ctx.err()))
    return rc


def _wfm(ctx, per_stream):
    L = ctx.L
    S, T = 4096, 16384
    taps = np.asarray(ctx.firdes_lowpass_f(79, 0.05), np.float32)
    rates = np.full(S, -0.085, np.float32)
    di = ctx.alloc(S * 2 * T); ctx.check(L.csdr_amd_memset(ctx.h, di.ptr, 0x80, S * 2 * T), "memset")
    pitch = (T // 50 + 64 + 63) // 64 * 64; ds = ctx.alloc(2 * S * pitch)

    def one(c):
        if per_stream:
            w = L.csdr_amd_wfm_create_rates(c.h, S, _p(rates), 10, _p(taps), taps.size, 5, 50e-6, 48000, 1 << 24)
        else:
            w = L.csdr_amd_wfm_create(c.h, S, -0.085, 10, _p(taps), taps.size, 5, 50e-6, 48000, 1 << 24)
        assert w, c.err()
        _check(c, L.csdr_amd_wfm_set_profiling(w, 1), "wfm_set_profiling")
        for _ in range(2):
            _check(c, L.csdr_amd_wfm_process(w, di.ptr, 2 * T, T, ds.ptr, None, pitch), "wfm_process")
        ms = C.c_double(); n = C.c_long()
        _check(c, L.csdr_amd_wfm_kernel_time(w, C.byref(ms), C.byref(n)), "wfm_kernel_time")
        assert n.value == 2 and ms.value > 0
        alive = _free()
        L.csdr_amd_wfm_destroy(w)
        return alive
    _cycles(ctx, one)


def test_wfm_shared_rate_cycles(ctx):
    _wfm(ctx, False)


def test_wfm_rate_per_stream_cycles(ctx):
    _wfm(ctx, True)


def test_wfm_ring_cycles(ctx):
    L = ctx.L
    S, T, N = 1024, 65536, 16                       # the ring's limits: blocks up to 65536 samples, up to 64 slots
    taps = np.asarray(ctx.firdes_lowpass_f(79, 0.05), np.float32)

    def one(c):
        r = L.csdr_amd_wfm_ring_create(c.h, S, -0.085, 10, _p(taps), taps.size, 5, 50e-6, 48000, T, N)
        assert r, c.err()
        seq = _check(c, L.csdr_amd_wfm_ring_submit(r), "wfm_ring_submit")
        _check(c, L.csdr_amd_wfm_ring_wait(r, seq, 10.0), "wfm_ring_wait")
        alive = _free()
        L.csdr_amd_wfm_ring_destroy(r)
        return alive
    _cycles(ctx, one)


def test_ddc_cycles(ctx):
    L = ctx.L
    S, T = 4096, 16384
    taps = np.asarray(ctx.firdes_lowpass_f(801, 0.01), np.float32)
    di = ctx.alloc(S * 2 * T); ctx.check(L.csdr_amd_memset(ctx.h, di.ptr, 0x80, S * 2 * T), "memset")
    opitch = T // 50 + 64; do = ctx.alloc(8 * S * opitch)

    def one(c):
        d = L.csdr_amd_ddc_create(c.h, S, -0.085, 50, _p(taps), taps.size, 1 << 24)
        assert d, c.err()
        _check(c, L.csdr_amd_ddc_set_profiling(d, 1), "ddc_set_profiling")
        _check(c, L.csdr_amd_ddc_process(d, di.ptr, 2 * T, T, do.ptr, opitch), "ddc_process")
        ms = C.c_double(); n = C.c_long()
        _check(c, L.csdr_amd_ddc_kernel_time(d, C.byref(ms), C.byref(n)), "ddc_kernel_time")
        alive = _free()
        L.csdr_amd_ddc_destroy(d)
        return alive
    _cycles(ctx, one)


def test_nfm_cycles(ctx):
    L = ctx.L
    S, T = 1024, 16384
    taps = np.asarray(ctx.firdes_lowpass_f(801, 0.01), np.float32)
    di = ctx.alloc(S * 2 * T); ctx.check(L.csdr_amd_memset(ctx.h, di.ptr, 0x80, S * 2 * T), "memset")
    apitch = 4096; ds = ctx.alloc(2 * S * apitch)

    def one(c):
        w = L.csdr_amd_nfm_create(c.h, S, -0.085, 50, _p(taps), taps.size, 48000, 1024, 0.2, 1.0, 1 << 22)      # ~1.3 GiB of state
        assert w, c.err()
        _check(c, L.csdr_amd_nfm_process(w, di.ptr, 2 * T, T, ds.ptr, None, apitch), "nfm_process")
        alive = _free()
        L.csdr_amd_nfm_destroy(w)
        return alive
    assert _cycles(ctx, one) >= 1 << 30


@pytest.mark.parametrize("fft", [8192, 16384])      # the one-pass kernel (1024 .. 8192) and the generic framing + hipFFT path
def test_waterfall_cycles(ctx, fft):
    L = ctx.L
    S, n_in = 4096, 16384
    fmt = "cf32" if fft > 8192 else "u8"
    nb = S * n_in * (8 if fmt == "cf32" else 2)
    x = ctx.alloc(nb); ctx.check(L.csdr_amd_memset(ctx.h, x.ptr, 0 if fmt == "cf32" else 0x80, nb), "memset")
    out_pitch = 4 * fft * ((n_in + fft) // 4096 + 2); out = ctx.alloc(S * out_pitch)        # rows of fft float dB values, Waterfall.max_rows() of them

    def one(c):
        w = csdr_amd.Waterfall(c, fft, 4096, 2, 0.0, "HAMMING", fmt, "db", S, n_in)
        w.process_dev(x.ptr, n_in, n_in, out.ptr, out_pitch)
        alive = _free()
        w.close()
        return alive
    _cycles(ctx, one)


def test_fftfilt_cycles(ctx):
    L = ctx.L
    S, B, fft = 64, 64, 16384
    taps = np.zeros(8001, np.complex64); taps[4000] = 1                 # too long for the one-pass LDS kernel: the full-size transform path
    inp = fft - taps.size + 1
    x = ctx.alloc(8 * S * B * inp); ctx.check(L.csdr_amd_memset(ctx.h, x.ptr, 0, 8 * S * B * inp), "memset")
    y = ctx.alloc(8 * S * B * inp)

    def one(c):
        f = L.csdr_amd_fftfilt_create(c.h, fft, _p(taps), taps.size, S, B)      # 1 GiB of spectra
        assert f, c.err()
        _check(c, L.csdr_amd_fftfilt_process(f, x.ptr, y.ptr, B, B * inp, B * inp), "fftfilt_process")
        alive = _free()
        L.csdr_amd_fftfilt_destroy(f)
        return alive
    assert _cycles(ctx, one) >= 1 << 30


def test_fastddc_bank_cycles(ctx):
    L = ctx.L
    nc, nb = 256, 64
    rates = np.linspace(-0.4, 0.4, nc).astype(np.float32)

    def one(c):
        bk = L.csdr_amd_fastddc_bank_create(c.h, 0.001, 256, _p(rates), nc, 2, nb)      # bench_fastddc.py's geometry: the matrix-core path
        assert bk, c.err()
        inv = L.csdr_amd_fastddc_bank_inverse(bk)
        _check(c, L.csdr_amd_fastddc_inv_set_profiling(inv, 2), "fastddc_inv_set_profiling")
        inp = L.csdr_amd_fastddc_bank_input_size(bk); ovl = L.csdr_amd_fastddc_bank_overlap(bk)
        x = c.alloc(8 * (nb * inp + ovl)); c.check(L.csdr_amd_memset(c.h, x.ptr, 0, 8 * (nb * inp + ovl)), "memset")
        opitch = L.csdr_amd_fastddc_bank_max_output(bk, nb) + 64
        y = c.alloc(8 * nc * opitch)
        _check(c, L.csdr_amd_fastddc_bank_process(bk, x.ptr, nb, y.ptr, opitch, None), "fastddc_bank_process")
        ms = C.c_double(); n = C.c_long()
        for stage in (1, 2):
            _check(c, L.csdr_amd_fastddc_inv_stage_time(inv, stage, C.byref(ms), C.byref(n)), "fastddc_inv_stage_time")
            assert n.value == 1
        alive = _free()
        L.csdr_amd_fastddc_bank_destroy(bk)
        del x, y
        return alive
    _cycles(ctx, one)


def test_fracdec_cycles(ctx):
    L = ctx.L
    S, n = 256, 1 << 20
    x = ctx.alloc(4 * S * n); ctx.check(L.csdr_amd_memset(ctx.h, x.ptr, 0, 4 * S * n), "memset")
    y = ctx.alloc(4 * S * n)

    def one(c):
        d = L.csdr_amd_fracdec_create(3.7, 12, None, 0)
        assert d, c.err()
        done = C.c_int()
        _check(c, L.csdr_amd_fractional_decimator_ff(c.h, d, x.ptr, y.ptr, S, n, n, n, C.byref(done)), "fractional_decimator_ff")
        c.sync()
        alive = _free()
        L.csdr_amd_fracdec_destroy(d)
        return alive
    _cycles(ctx, one)


def test_fftcc_cycles(ctx):
    L = ctx.L
    fft, frames = 65536, 2048
    x = ctx.alloc(8 * fft * 8); ctx.check(L.csdr_amd_memset(ctx.h, x.ptr, 0, 8 * fft * 8), "memset")
    y = ctx.alloc(8 * fft * 8)

    def one(c):
        f = L.csdr_amd_fftcc_create(c.h, fft, fft, 2, frames)          # 1 GiB frame buffer
        assert f, c.err()
        used = C.c_size_t()
        _check(c, L.csdr_amd_fftcc_process(f, x.ptr, 8 * fft, y.ptr, C.byref(used)), "fftcc_process")
        alive = _free()
        L.csdr_amd_fftcc_destroy(f)
        return alive
    assert _cycles(ctx, one) >= 1 << 30


# ---- the stateful wrapper objects, each at the smallest shape of its own test file: created with `with`, two calls, gone at the end of the block
def _object_cycles(ctx, make, x):
    def one(c):
        with make(c) as o:
            o.process(x); o.process(x)
            alive = _free()
        assert o.h is None
        return alive
    _cycles(ctx, one)


def _noise(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.complex64:
        return (0.3 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))).astype(np.complex64)
    return (0.3 * rng.standard_normal(shape)).astype(dtype)


def test_resampler_cycles(ctx):
    taps = csdr_amd.rational_resampler_get_lowpass_f(80, 3, 2)
    _object_cycles(ctx, lambda c: csdr_amd.Resampler(c, 3, 2, taps, 2), _noise((2, 1024), np.float32, 1))


def test_interpolator_cycles(ctx):
    taps = csdr_amd.fir_interpolate_lowpass_f(81, 4)
    _object_cycles(ctx, lambda c: csdr_amd.Interpolator(c, 4, taps, 2), _noise((2, 1024), np.complex64, 2))


def test_psk31_cycles(ctx):
    _object_cycles(ctx, lambda c: csdr_amd.Psk31(c, csdr_amd.psk31_params(), 2), _noise((2, 4096), np.complex64, 3))


def test_psk31tx_cycles(ctx):
    x = np.frombuffer((b"CQ CQ DE TEST PSE K " * 4)[:64], np.uint8).reshape(2, 32)
    _object_cycles(ctx, lambda c: csdr_amd.Psk31Tx(c, 2, 2, 256), x)


def test_rtty_cycles(ctx):
    _object_cycles(ctx, lambda c: csdr_amd.Rtty(c, csdr_amd.rtty_params(cli_bufsize=4096), 2), _noise((2, 4096), np.complex64, 4))


def test_squelch_cycles(ctx):
    _object_cycles(ctx, lambda c: csdr_amd.Squelch(c, 2, 1024, 1, [0.01, 0.01], 4096), _noise((2, 2048), np.complex64, 5))


def test_carrier_cycles(ctx):
    _object_cycles(ctx, lambda c: csdr_amd.Carrier(c, csdr_amd.costas_params(0.05, 0.707, True), 2), _noise((2, 1024), np.complex64, 6))


def test_txbank_cycles(ctx):
    taps = ctx.firdes_lowpass_f(79, 0.5 / 8)
    x = (8000 * _noise((2, 1024), np.float32, 7)).astype(np.int16)
    _object_cycles(ctx, lambda c: csdr_amd.TxBank(c, 2, "fm", 8, taps, [0.1, -0.2], max_in_samples=1024), x)


# ---- a Context method whose call fails half way: the C object it made is destroyed on that path too
@pytest.mark.parametrize("chain", ["wfm_chain", "ddc_u8"])
def test_failed_retune_leaves_no_object_behind(ctx, chain):
    """A retune of stream 99 out of 4: csdr_amd_wfm_set_rate / csdr_amd_ddc_set_rate return -3 (an error return on the host, no kernel runs)."""
    S, T = 4, 16384
    iq = np.full((S, 2 * T), 0x80, np.uint8)
    rates = np.linspace(-0.1, 0.1, S).astype(np.float32)
    if chain == "wfm_chain":
        args = (10, np.asarray(ctx.firdes_lowpass_f(79, 0.05), np.float32))
    else:
        args = (50, np.asarray(ctx.firdes_lowpass_f(801, 0.01), np.float32))

    def one(c):
        with pytest.raises(csdr_amd.CsdrAmdError, match="set_rate"):
            getattr(c, chain)(iq, rates, *args, block=T, retunes={0: [(99, 0.1)]})
        return _free()
    _cycles(ctx, one)
